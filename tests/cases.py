"""The CPU side of fhecore.polyeval / fhecore.bootstrap and the cases the CPU and GPU tests share.

CpuBackend is the one backend over (2, l, N) object arrays: every method a call into pyoracle (and
encode_ref for a factor's diagonals).  world() builds a case's key material -- the secret, the
relinearisation key, the rotation keys, sk in NTT form -- from pyoracle with fixed seeds,
consuming each generator in one fixed order; a Case states what differs between the five
cases as data; setup() and run_cpu() compute a case's keys and inputs, and its evaluation on the
CPU backend, once per process.  tests/golden/op_refs.json pins all of it
(tests/test_op_refs_cpu.py)."""
import dataclasses
import functools
import math
import random
from typing import Callable

import numpy as np

import bootstrap_ref as br
import encode_ref
import pyoracle
import refs
import sparse_pack_ref as sp


class CpuBackend:
    """The backend of fhecore.polyeval and fhecore.bootstrap over (2, l, N) object arrays (a leading
    batch dimension is looped over).  relin_key: (evk_b, evk_a); rot_keys: {Galois element:
    (rot_b, rot_a)}."""

    def __init__(self, log_n, qs, ps, dnum, relin_key, rot_keys=None):
        self.log_n, self.dnum = log_n, dnum
        self.moduli, self.ps = [int(q) for q in qs], [int(p) for p in ps]
        self.relin_key, self.rot_keys = relin_key, rot_keys or {}
        self.chain = (self.moduli, self.ps, dnum)

    @staticmethod
    def _batched(fn, *xs):
        xs = [np.asarray(x) for x in xs]
        if xs[0].ndim == 3:
            return fn(*xs)
        return np.stack([fn(*[x[i] for x in xs]) for i in range(xs[0].shape[0])])

    def _key(self, elt):
        return None if elt == 1 else self.rot_keys[elt]

    def mul_relin(self, a, b, rescale):
        return self._batched(lambda x, y: pyoracle.mul_relin(
            x, y, *self.relin_key, *self.chain, rescale, level=x.shape[-2], ntt=refs.c_ntt()), a, b)

    def mul_sum_relin(self, as_, bs, rescale, level):
        n = len(as_)
        return self._batched(lambda *xs: pyoracle.mul_sum_relin(
            xs[:n], xs[n:], *self.relin_key, *self.chain, rescale, level=level, ntt=refs.c_ntt()),
            *as_, *bs)

    def lincomb(self, cts, scalars, const, rescale, level):
        n = len(cts)
        return self._batched(lambda *xs: pyoracle.lincomb(
            xs, scalars[:n], self.moduli, level=level, const=scalars[n] if const else None,
            rescale=rescale, ntt=refs.c_ntt()), *cts)

    def drop_level(self, a, level):
        return np.asarray(a)[..., :level, :]

    def mod_raise(self, a, level):
        return pyoracle.mod_raise(a, self.moduli, np.asarray(a).shape[-2], level, ntt=refs.c_ntt())

    def load_factor(self, z, baby, giant, delta):
        """z [n2, n1, n_s] diagonals, tiled to the full ring (once for full packing)."""
        n = 1 << self.log_n
        z = np.asarray(z)
        enc = encode_ref.encode(np.tile(z, (n // 2) // z.shape[-1]), delta, self.log_n,
                                self.moduli + self.ps).astype(object)
        be = [pyoracle.galois_elt(s, n) for s in baby]
        ge = [pyoracle.galois_elt(s, n) for s in giant]
        pts = [[enc[g, b] for b in range(len(be))] for g in range(len(ge))]
        return (be, [self._key(e) for e in be], ge, [self._key(e) for e in ge], pts)

    def linear_transform(self, a, factor):
        baby, bkeys, giant, gkeys, pts = factor
        return self._batched(lambda x: pyoracle.linear_transform(
            x, baby, bkeys, giant, gkeys, pts, *self.chain, self.log_n, level=x.shape[-2],
            ntt=refs.c_ntt()), a)

    def rescale(self, a):
        return self._batched(
            lambda x: pyoracle.rescale_ct(x, self.moduli[:x.shape[-2]], refs.c_ntt()), a)

    def _galois(self, a, elt):
        return self._batched(lambda x: pyoracle.rotate(
            x, elt, *self.rot_keys[elt], *self.chain, self.log_n, level=x.shape[-2],
            ntt=refs.c_ntt()), a)

    def conjugate(self, a):
        return self._galois(a, (2 << self.log_n) - 1)

    def rotate(self, a, step):
        return self._galois(a, pyoracle.galois_elt(step, 1 << self.log_n))

    def conj_split(self, a, c):
        return pyoracle.conj_split(a, c, self.moduli, level=np.asarray(a).shape[-2],
                                   ntt=refs.c_ntt())

    def conj_merge(self, a, b):
        return pyoracle.conj_merge(a, b, self.moduli, level=np.asarray(a).shape[-2],
                                   ntt=refs.c_ntt())

    def stack(self, a, b):
        return np.stack([a, b])

    def unstack(self, x):
        return x[0], x[1]


# ---- the case builder -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _keys(log_n, qs, ps, dnum, secret, key_seed):
    rng = random.Random(key_seed)
    if secret is None:
        s = [rng.randrange(-1, 2) for _ in range(1 << log_n)]
    else:
        s = [int(v) for v in pyoracle.sparse_secret_coefficients(*secret, log_n)]
    relin = pyoracle.gen_relin_key(s, list(qs), list(ps), dnum, rng)
    return s, relin, rng.getstate()


@functools.lru_cache(maxsize=None)
def world(log_n, qs, ps, dnum, secret, key_seed, rot_elts=(), rot_seed=None):
    """Keys from pyoracle with fixed seeds.  qs, ps tuples; secret None (ternary, the first draws
    of random.Random(key_seed)) or (seed, h) of pyoracle.sparse_secret_coefficients.  The
    generator is consumed in this order: the secret, the relinearisation key, the rotation keys in
    sorted element order -- those from random.Random(rot_seed) instead where rot_seed is given
    (a case that shares another's secret and relinearisation key).  -> dict(qs, ps, relin, rot,
    sk_ntt, decrypt); decrypt(data, level) is the plaintext (level, N) in NTT form."""
    s, relin, state = _keys(log_n, qs, ps, dnum, secret, key_seed)
    qs, ps = list(qs), list(ps)
    rng = random.Random(rot_seed)
    if rot_seed is None:
        rng.setstate(state)
    rot = {k: pyoracle.gen_rot_key(s, k, qs, ps, dnum, rng) for k in sorted(rot_elts)}
    sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, qs + ps), qs + ps)

    def decrypt(data, level):
        return pyoracle.decrypt(np.asarray(data).astype(object), sk_ntt, qs[:level])

    return dict(qs=qs, ps=ps, relin=relin, rot=rot, sk_ntt=sk_ntt, decrypt=decrypt)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    log_n: int
    L: int
    nspecial: int
    dnum: int
    bits: int          # of the chain's primes (moduli: another rule)
    delta: float       # the scale the input is encoded at
    key_seed: int
    inputs: Callable   # (case, encrypt) -> dict; encrypt(z, seed) -> (pt, ct)
    run: Callable      # (case, backend, su, arg) -> polyeval.Ct
    target: Callable   # (su, arg) -> the slots the result should hold
    moduli: Callable = None  # () -> (qs, ps); None: the L + nspecial largest primes below 2^bits
    real: bool = False       # decode: the real parts only
    log_slots: int = None    # None: the host Encoder; else encode_ref on 2^log_slots slots
    secret: tuple = None     # world()'s secret
    rot: Callable = None     # () -> Galois elements of the rotation keys
    rot_seed: int = None
    params: dict = None      # of the Bootstrapper

    def chain(self):
        if self.moduli:
            return self.moduli()
        m = [int(q) for q in pyoracle.gen_moduli(self.log_n, self.L + self.nspecial, bits=self.bits)]
        return m[:self.L], m[self.L:]


def _encoder(case):
    from fhecore.ckks import Encoder

    return Encoder(1 << case.log_n)


def encode(case, z, scale, qs):
    """Slots -> NTT-form plaintext rows over qs, with the case's encoder."""
    if case.log_slots is not None:
        return sp.encode(z, scale, case.log_n, case.log_slots, qs)
    import coracle
    from fhecore.ckks import to_rns

    return coracle.ntt_fwd(to_rns(_encoder(case).encode(z, scale), qs), qs)


def decode(case, dec, level, scale):
    """A decrypted plaintext (level, N), NTT form -> the case's slots."""
    qs = case.chain()[0]
    dec = np.asarray(dec).astype(np.uint64)
    if case.log_slots is not None:
        return sp.decode(dec, float(scale), case.log_n, case.log_slots, qs, level)
    import coracle
    from fhecore.ckks import from_rns

    z = _encoder(case).decode(from_rns(coracle.ntt_inv(dec, qs[:level]), qs[:level]), float(scale))
    return z.real if case.real else z


@functools.lru_cache(maxsize=None)
def setup(case):
    """world() of the case plus what case.inputs returns: dict of host arrays."""
    qs, ps = case.chain()
    w = world(case.log_n, tuple(qs), tuple(ps), case.dnum, case.secret, case.key_seed,
              tuple(case.rot()) if case.rot else (), case.rot_seed)

    def encrypt(z, seed):
        pt = encode(case, z, case.delta, qs)
        return pt, pyoracle.encrypt_sk(seed, pt, w["sk_ntt"], qs, case.log_n)

    return dict(w, **case.inputs(case, encrypt))


def backend(case):
    su = setup(case)
    return CpuBackend(case.log_n, su["qs"], su["ps"], case.dnum, su["relin"], su["rot"])


def decrypt_decode(case, data, level, scale):
    return decode(case, setup(case)["decrypt"](data, level), level, scale)


def slot_error(case, ct, arg=None):
    """Maximum slot error of a polyeval.Ct (host data) against the case's target."""
    got = decrypt_decode(case, ct.data, ct.level, ct.scale)
    return float(np.abs(got - case.target(setup(case), arg)).max())


@functools.lru_cache(maxsize=None)
def run_cpu(case, arg=None, run=None):
    """case.run (or `run`) on the CPU backend: (Ct with an object array, max slot error)."""
    out = (run or case.run)(case, backend(case), setup(case), arg)
    return out, slot_error(case, out, arg)


def _ct(data, level, scale):
    from fhecore.polyeval import Ct

    return Ct(data, level, scale)


# ---- Chebyshev: log_n = 10, L = 8, K = 2, dnum = 4, a 50-bit chain, delta = 2^50; 512 real slots
# uniform in [-1, 1]; arg = the degree of the interpolant of cos(2x)

def cheb_coeffs(degree):
    """Chebyshev interpolant of cos(2x) on [-1, 1]."""
    return np.polynomial.chebyshev.chebinterpolate(lambda t: np.cos(2 * t), degree)


def _cheb_inputs(case, encrypt):
    x = np.random.default_rng(5).uniform(-1, 1, 1 << (case.log_n - 1))
    return dict(x=x, ct=encrypt(x, 77)[1])


def _cheb_run(case, be, su, degree):
    from fhecore import polyeval

    return polyeval.chebyshev_eval(be, _ct(su["ct"], case.L, case.delta), cheb_coeffs(degree))


CHEB = Case("cheb", 10, 8, 2, 4, 50, 2.0 ** 50, 1234, _cheb_inputs, _cheb_run,
            lambda su, degree: np.polynomial.chebyshev.chebval(su["x"], cheb_coeffs(degree)),
            real=True)
# maximum slot error of chebyshev_eval on the CPU backend against chebval, measured once
# (deterministic under the seeds above): degree 7 and degree 15 of cos(2x)
CHEB_ERR_DEG7 = 2.06e-12
CHEB_ERR_DEG15 = 2.03e-12


# ---- EvalMod (fhecore.polyeval.eval_mod): log_n = 10, L = 12, 3 special primes, dnum = 4, a 50-bit
# chain, delta = 2^50; mod-range K = 16 (eval_mod's parameter, not the special-prime count), degree
# 31, 3 double angles: 6 + 3 = 9 levels, so the result is at level 3; slots v = (I + eps) / 16, I
# uniform in [-15, 15], eps uniform in [-2^-8, 2^-8].  The result's slots hold
# sin(2 pi K v) / (2 pi), which is eps up to (2 pi)^2 |eps|^3 / 6.
K, DEGREE, DOUBLE_ANGLES = 16, 31, 3
EPS_MAX = 2.0 ** -8
# the cubic term the choice of eps accepts: EvalMod's own error must stay below it (a condition,
# not a measurement)
CAP = (2 * math.pi) ** 2 * EPS_MAX ** 3 / 6
# maximum slot error of eval_mod on the CPU backend against float64 sin(2 pi K v) / (2 pi),
# measured once (deterministic under the seeds below).  In plain float64 the polynomial and the
# double angles alone give 5.5e-10 at these parameters; the rest is the evaluator's scale drift
# (the primes sit ~2^-30 off delta, chebyshev_eval's docstring) and the encryption and rescale
# noise, doubled by each of the three double-angle steps.
EVALMOD_ERR = 1.051e-08
# over the constant: float differences between numpy builds in the decode only
MARGIN = 1.05


def evalmod_slots(count):
    """(v, eps): v = (I + eps) / K."""
    g = np.random.default_rng(6)
    big_i = g.integers(-(K - 1), K, count)
    eps = g.uniform(-EPS_MAX, EPS_MAX, count)
    return (big_i + eps) / K, eps


def evalmod_target(v):
    return np.sin(2 * np.pi * K * v) / (2 * np.pi)


def _evalmod_inputs(case, encrypt):
    v, eps = evalmod_slots(1 << (case.log_n - 1))
    pt, ct = encrypt(v, 78)
    return dict(v=v, eps=eps, pt=pt, ct=ct)


def _evalmod_run(case, be, su, _):
    from fhecore import polyeval

    return polyeval.eval_mod(be, _ct(su["ct"], case.L, case.delta), K, DEGREE, DOUBLE_ANGLES)


EVALMOD = Case("evalmod", 10, 12, 3, 4, 50, 2.0 ** 50, 4321,
               _evalmod_inputs, _evalmod_run, lambda su, _: evalmod_target(su["v"]), real=True)


# ---- the sum of products: log_n = 10, L = 4, K = 2, dnum = 2, a 50-bit chain, delta = 2^40; 2 x 16
# vectors of 512 complex slots uniform in the unit square; arg = the number of terms
COUNTS = (4, 16)
# Maximum slot error against numpy's sum_i z_i w_i on the CPU reference, measured once
# (deterministic under the seeds below).  FUSED: inner_product (one key-switch, one rescale);
# COMPOSED: mul_relin(rescale) per term, then the sum of the rescaled ciphertexts.
FUSED_ERR = {4: 9.72e-7, 16: 6.96e-7}
COMPOSED_ERR = {4: 1.57e-6, 16: 3.44e-6}  # the fused form: 0.62x and 0.20x of these


def _mulsum_inputs(case, encrypt):
    g = np.random.default_rng(9)
    half = 1 << (case.log_n - 1)

    def fresh(seed):
        z = g.uniform(0, 1, half) + 1j * g.uniform(0, 1, half)  # the unit square
        return z, np.asarray(encrypt(z, seed)[1], dtype=np.uint64)

    xs = [fresh(100 + i) for i in range(max(COUNTS))]
    ys = [fresh(200 + i) for i in range(max(COUNTS))]
    return dict(z=[x[0] for x in xs], w=[y[0] for y in ys], x=[x[1] for x in xs],
                y=[y[1] for y in ys])


def mulsum_operands(count, wrap=lambda x: x):
    """The two Ct lists of the case at `count` terms; wrap moves a host array to the backend."""
    su = setup(MULSUM)
    return ([_ct(wrap(t), MULSUM.L, MULSUM.delta) for t in su["x"][:count]],
            [_ct(wrap(t), MULSUM.L, MULSUM.delta) for t in su["y"][:count]])


def _fused(case, be, su, count):
    from fhecore import polyeval

    return polyeval.inner_product(be, *mulsum_operands(count))


def composed(case, be, su, count):
    """The composed form: mul_relin(rescale) per term, then the sum of the rescaled ciphertexts."""
    xs, ys = mulsum_operands(count)
    L = case.L
    col = pyoracle._mods_col(su["qs"][:L - 1])
    acc = 0
    for x, y in zip(xs, ys):
        acc = (acc + be.mul_relin(x.data, y.data, True)) % col
    return _ct(acc, L - 1, xs[0].scale * ys[0].scale / su["qs"][L - 1])


MULSUM = Case("mulsum", 10, 4, 2, 2, 50, 2.0 ** 40, 4321, _mulsum_inputs,
              _fused, lambda su, count: sum(z * w for z, w in zip(su["z"][:count], su["w"][:count])))


# ---- bootstrap and sparse bootstrap: bootstrap_ref's and sparse_pack_ref's chains, parameters and
# rotation elements; the input dropped to level 1 and refreshed to level 3

def _model_inputs(seed, enc_seed):
    def inputs(case, encrypt):
        z = br.model_slots(1 << case.log_slots, seed)
        pt, ct = encrypt(z, enc_seed)
        return dict(z=z, pt=pt, ct=ct)
    return inputs


def _bootstrap_run(case, be, su, _):
    from fhecore import bootstrap as bs

    return bs.Bootstrapper(be, **case.params).bootstrap(
        _ct(np.asarray(su["ct"])[:, :1], 1, case.delta))


BOOTSTRAP = Case("bootstrap", br.LOG_N, br.L, br.NSPECIAL, br.DNUM, br.BITS, br.DELTA, 2718,
                 _model_inputs(9, 79), _bootstrap_run, lambda su, _: su["z"], moduli=br.moduli,
                 log_slots=br.LOG_N - 1, secret=(br.SK_SEED, br.HAMMING), rot=br.rotation_elements,
                 params=br.PARAMS)
# Maximum slot error of Bootstrapper.bootstrap on the CPU backend against the input slots, measured
# once (deterministic under the seeds above).  It consists of EvalMod's cubic term (model(): 2.7e-5
# at this q_0 for these slots) and of the noise in front of SlotToCoeff -- eval_mod's own
# (EVALMOD_ERR's size; the key-switch noise of the CoeffToSlot rotations and of the conjugation is
# divided by K q_0 and so negligible) -- times q_0 / delta = 2^5 and summed over the 1024
# coefficients behind a slot.  Under a secret of weight 28 the integer polynomial I is smaller than
# the model's uniform draw, which is why the measured value sits below the model's 4.0e-5.
BOOTSTRAP_ERR = 2.833e-05

# bootstrap's chain, secret and relinearisation key; rotation keys and input with seeds of their own
SPARSE = dataclasses.replace(
    BOOTSTRAP, name="sparse", delta=sp.IN_SCALE, inputs=_model_inputs(11, 83),
    log_slots=sp.LOG_SLOTS, rot=sp.rotation_elements, rot_seed=31415, params=sp.PARAMS)
# Maximum slot error of the sparse Bootstrapper.bootstrap on the CPU backend against the input
# slots, measured once (deterministic under the seeds above).  At bootstrap's message ratio the
# cubic term is full packing's (cubic_term: 2.47e-5 for these slots), and the noise in front
# of SlotToCoeff is summed over 128 coefficients and not 1024.
SPARSE_BOOTSTRAP_ERR = 2.442e-05

CASES = {c.name: c for c in (CHEB, EVALMOD, MULSUM, BOOTSTRAP, SPARSE)}
RUNS = [(CHEB, 7, None), (CHEB, 15, None), (EVALMOD, None, None), (MULSUM, 4, None),
        (MULSUM, 16, None), (MULSUM, 4, composed), (MULSUM, 16, composed), (BOOTSTRAP, None, None),
        (SPARSE, None, None)]


def case_digests(setup_of=setup, run_of=run_cpu):
    """{"case/<name>/...": value}: SHA-256 of every array of each case's setup() and of every CPU
    result's data words, with its level, scale and error written out."""
    import hashlib

    def sha(x):
        x = np.asarray(x)
        raw = x if x.dtype.kind in "fc" else refs.words(x)
        return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()

    out = {}
    for name, case in CASES.items():
        su = setup_of(case)
        for key, val in su.items():
            if key == "rot":
                val = [np.stack(val[k]) for k in sorted(val)]
            if key == "relin":
                val = np.stack(val)
            if callable(val):
                continue
            parts = val if isinstance(val, list) and key not in ("qs", "ps") else [val]
            out[f"case/{name}/setup/{key}"] = hashlib.sha256(
                "".join(sha(p) for p in parts).encode()).hexdigest()
    for case, arg, run in RUNS:
        ct, err = run_of(case, arg, run)
        tag = f"case/{case.name}/{'composed' if run else 'cpu'}/{arg}"
        out[tag + "/data"] = sha(ct.data)
        out[tag + "/level"] = str(ct.level)
        out[tag + "/scale"] = str(ct.scale)
        out[tag + "/err"] = float(err).hex()
    return out
