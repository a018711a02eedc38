"""References for fhecore.bootstrap: the float64 plaintext model of the pipeline, the CPU backend of
the Bootstrapper (plain_ref.CpuBackend plus pyoracle at a level, modraise_ref, conj_ref and
encode_ref), and the case the CPU and GPU tests share, computed once per process:

  log_n = 10, L = 18, 5 special primes, dnum = 4; q_0 the largest 55-bit prime of the ring, the
  other 22 primes the 50-bit chain, delta = 2^50; a secret of Hamming weight 28 (sparse_ref);
  K = 16, degree 31, 3 double angles, 3 + 3 factors: 3 + 9 + 3 levels, the result at level 3;
  512 slots uniform in the square [-1, 1]^2, fixed seeds, keys from pyoracle.

The size of q_0 over delta = 2^50 is chosen with `model` below.  EvalMod returns m / q_0 with its
own cubic term (2 pi)^2 (m / q_0)^3 / 6, and SlotToCoeff multiplies every error in it by q_0 / delta:
a larger q_0 shrinks the cubic term (by 4 per bit, after the multiplication) and grows the
evaluator's noise (by 2 per bit).  model() at log_n = 10, seed 3, maximum slot error:

    q_0 bits   exact sine     interpolant     exact sine + 1e-8      interpolant + 1e-8
       54       1.07e-04       1.07e-04            1.08e-04               1.08e-04
       55       2.67e-05       2.68e-05            4.02e-05               4.03e-05
       56       6.68e-06       6.83e-06            5.48e-05               5.51e-05
       58       4.18e-07       3.75e-06            2.23e-04               2.25e-04
       60       2.61e-08       1.46e-05            8.94e-04               8.99e-04

(1e-8: normal noise of that deviation on every EvalMod output, the size of evalmod_ref.EVALMOD_ERR.)
With the evaluator's noise the minimum is at 55 bits: that is the choice."""
import functools
import random

import numpy as np

import conj_ref
import encode_ref
import modraise_ref
import plain_ref
import pyoracle
import refs
import sparse_ref

LOG_N, L, NSPECIAL, DNUM = 10, 18, 5, 4
Q0_BITS, BITS = 55, 50
DELTA = 2.0 ** 50
HAMMING = 28
SK_SEED = 31
PARAMS = dict(K=16, degree=31, double_angles=3, cts_groups=3, stc_groups=3, delta=DELTA,
              hamming_weight=HAMMING)
OUT_LEVEL = 3
# Maximum slot error of Bootstrapper.bootstrap on the CPU backend against the input slots, measured
# once (deterministic under the seeds below).  It consists of EvalMod's cubic term (model(): 2.7e-5
# at this q_0 for these slots) and of the noise in front of SlotToCoeff -- eval_mod's own
# (EVALMOD_ERR's size; the key-switch noise of the CoeffToSlot rotations and of the conjugation is
# divided by K q_0 and so negligible) -- times q_0 / delta = 2^5 and summed over the 1024
# coefficients behind a slot.  Under a secret of weight 28 the integer polynomial I is smaller than
# the model's uniform draw, which is why the measured value sits below the model's 4.0e-5.
BOOTSTRAP_ERR = 2.833e-05
# over the constant on the CPU: float differences between numpy builds in encode / decode only
MARGIN = 1.05


def apply_factors(factors, v, const=1.0):
    for f in factors:
        v = sum(d * const * np.roll(v, -k) for k, d in f.items())
    return v


def model_slots(count, seed):
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, count) + 1j * g.uniform(-1, 1, count)


def model(log_n, q0, delta=DELTA, K=16, degree=31, double_angles=3, groups=3, exact_sine=True,
          noise=0.0, seed=3):
    """The pipeline on float64 slot vectors with the Bootstrapper's constants: slots uniform in
    [-1, 1]^2, I uniform in [-(K-1), K-1], t = m + q_0 I, CoeffToSlot with delta / (2 n K q_0)
    (the declared scale delta divided out), the split, sin(2 pi K v) / (2 pi) exactly or by
    eval_mod's interpolant and double angles, optional normal noise on its output, the merge,
    SlotToCoeff with q_0 / delta.  Returns the maximum slot error."""
    from fhecore import bootstrap as bs

    n = 1 << (log_n - 1)
    g = np.random.default_rng(seed)
    z = g.uniform(-1, 1, n) + 1j * g.uniform(-1, 1, n)
    cts, stc = bs.dft_factors(log_n, groups, True), bs.dft_factors(log_n, groups, False)
    w = apply_factors(cts, z) * delta / n  # c_k + i c_{k+n}, in the network's order
    m = np.rint(w.real) + 1j * np.rint(w.imag)
    big_i = g.integers(-(K - 1), K, n) + 1j * g.integers(-(K - 1), K, n)
    raw = apply_factors(stc, m + q0 * big_i)  # the raised ciphertext's slots times its scale
    y = apply_factors(cts, raw, (1 / (2.0 * n * K * q0)) ** (1 / groups))

    def eval_mod(v):
        if exact_sine:
            e = np.sin(2 * np.pi * K * v) / (2 * np.pi)
        else:
            c = np.polynomial.chebyshev.chebinterpolate(
                lambda x: np.cos((2 * np.pi * K * x - np.pi / 2) / 2 ** double_angles), degree)
            e = np.polynomial.chebyshev.chebval(v, c)
            for _ in range(double_angles):
                e = 2 * e * e - 1
            e = e / (2 * np.pi)
        return e + g.normal(0, noise, n) if noise else e

    merged = eval_mod(2 * y.real) + 1j * eval_mod(2 * y.imag)
    out = apply_factors(stc, merged, (q0 / delta) ** (1 / groups))
    return float(np.abs(out - z).max())


# ---- the CPU backend ------------------------------------------------------------------------------

class CpuBackend(plain_ref.CpuBackend):
    """fhecore.bootstrap's backend over (2, l, N) object arrays (a leading batch dimension is
    looped over).  rot_keys: {Galois element: (rot_b, rot_a)}."""

    def __init__(self, log_n, qs, ps, dnum, relin_key, rot_keys):
        super().__init__(qs, ps, dnum, relin_key[0], relin_key[1])
        self.log_n, self.rot_keys = log_n, rot_keys

    @staticmethod
    def _batched(fn, *xs):
        xs = [np.asarray(x) for x in xs]
        if xs[0].ndim == 3:
            return fn(*xs)
        return np.stack([fn(*[x[i] for x in xs]) for i in range(xs[0].shape[0])])

    def mul_relin(self, a, b, rescale):
        return self._batched(lambda x, y: plain_ref.CpuBackend.mul_relin(self, x, y, rescale), a, b)

    def lincomb(self, cts, scalars, const, rescale, level):
        return self._batched(
            lambda *xs: plain_ref.CpuBackend.lincomb(self, list(xs), scalars, const, rescale, level),
            *cts)

    def drop_level(self, a, level):
        return np.asarray(a)[..., :level, :]

    def mod_raise(self, a, level):
        a = np.asarray(a)
        return modraise_ref.mod_raise(a, self.moduli, a.shape[-2], level)

    def _key(self, elt):
        return None if elt == 1 else self.rot_keys[elt]

    def load_factor(self, z, baby, giant, delta):
        n = 1 << self.log_n
        enc = encode_ref.encode(z, delta, self.log_n, self.moduli + self.ps).astype(object)
        be = [pyoracle.galois_elt(s, n) for s in baby]
        ge = [pyoracle.galois_elt(s, n) for s in giant]
        pts = [[enc[g, b] for b in range(len(be))] for g in range(len(ge))]
        return (be, [self._key(e) for e in be], ge, [self._key(e) for e in ge], pts)

    def linear_transform(self, a, factor):
        baby, bkeys, giant, gkeys, pts = factor
        return self._batched(lambda x: pyoracle.linear_transform(
            x, baby, bkeys, giant, gkeys, pts, self.moduli, self.ps, self.dnum, self.log_n,
            level=x.shape[-2], ntt=refs.c_ntt()), a)

    def rescale(self, a):
        return self._batched(lambda x: plain_ref._rescale(x, self.moduli[:x.shape[-2]]), a)

    def conjugate(self, a):
        elt = (2 << self.log_n) - 1
        kb, ka = self.rot_keys[elt]
        return self._batched(lambda x: pyoracle.rotate(
            x, elt, kb, ka, self.moduli, self.ps, self.dnum, self.log_n, level=x.shape[-2],
            ntt=refs.c_ntt()), a)

    def conj_split(self, a, c):
        return conj_ref.conj_split(a, c, self.moduli, np.asarray(a).shape[-2])

    def conj_merge(self, a, b):
        return conj_ref.conj_merge(a, b, self.moduli, np.asarray(a).shape[-2])

    def stack(self, a, b):
        return np.stack([a, b])

    def unstack(self, x):
        return x[0], x[1]


# ---- the shared case ------------------------------------------------------------------------------

def moduli():
    q0 = [int(q) for q in pyoracle.gen_moduli(LOG_N, 1, bits=Q0_BITS)]
    rest = [int(q) for q in pyoracle.gen_moduli(LOG_N, L - 1 + NSPECIAL, bits=BITS)]
    return q0 + rest[:L - 1], rest[L - 1:]


def rotation_elements():
    """The Galois elements of every baby / giant step of the six factors, and the conjugation."""
    from fhecore import bootstrap as bs

    n = 1 << LOG_N
    steps = set()
    for inverse, groups in ((True, PARAMS["cts_groups"]), (False, PARAMS["stc_groups"])):
        for n1, n2, stride, offset in bs.factor_layouts(LOG_N, groups, inverse):
            steps |= {stride * (b + offset) for b in range(n1)} | {stride * g * n1 for g in range(n2)}
    return sorted({pyoracle.galois_elt(s, n) for s in steps if s % (n // 2)} | {2 * n - 1})


@functools.lru_cache(maxsize=None)
def setup():
    """Keys and the encrypted input from pyoracle with fixed seeds: dict of host arrays."""
    n = 1 << LOG_N
    qs, ps = moduli()
    m = qs + ps
    s = [int(v) for v in sparse_ref.coefficients(SK_SEED, HAMMING, LOG_N)]
    rng = random.Random(2718)
    relin = pyoracle.gen_relin_key(s, qs, ps, DNUM, rng)
    rot = {k: pyoracle.gen_rot_key(s, k, qs, ps, DNUM, rng) for k in rotation_elements()}
    sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, m), m)
    z = model_slots(n // 2, 9)
    pt = encode_ref.encode(z, DELTA, LOG_N, qs)
    ct = pyoracle.encrypt_sk(79, pt, sk_ntt, qs, LOG_N)
    return dict(qs=qs, ps=ps, relin=relin, rot=rot, sk_ntt=sk_ntt, z=z, pt=pt, ct=ct)


def backend():
    su = setup()
    return CpuBackend(LOG_N, su["qs"], su["ps"], DNUM, su["relin"], su["rot"])


def decode(dec, level, scale):
    """A decrypted plaintext (level, N), NTT form -> complex slots."""
    return encode_ref.decode(np.asarray(dec).astype(np.uint64), float(scale), LOG_N,
                             setup()["qs"], level)


def decrypt_decode(data, level, scale):
    su = setup()
    dec = pyoracle.decrypt(np.asarray(data).astype(object), su["sk_ntt"], su["qs"][:level])
    return decode(dec, level, scale)


@functools.lru_cache(maxsize=None)
def bootstrap_cpu():
    """Bootstrapper.bootstrap on the CPU backend, from the input dropped to level 1:
    (Ct with a (2, 3, N) object array, max slot error)."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    su = setup()
    boot = bs.Bootstrapper(backend(), **PARAMS)
    out = boot.bootstrap(Ct(np.asarray(su["ct"])[:, :1], 1, DELTA))
    got = decrypt_decode(out.data, out.level, out.scale)
    return out, float(np.abs(got - su["z"]).max())
