"""Reference for the sum of ciphertext products with one relinearisation (fhe_mul_sum_relin_level;
include/fhecore.h), built from pyoracle's tensor, key-switch and rescale in exact Python-integer
arithmetic; the CPU backend method of fhecore.polyeval.inner_product; and the decrypt case the CPU
and GPU tests share (computed once per process)."""
import functools
import random

import numpy as np

import plain_ref
import pyoracle
import refs


def tensor_sum(As, Bs, qs, level):
    """(D_0, D_1, D_2) = sum_i tensor_ntt(As[i] | level, Bs[i] | level) mod q_j: (3, level, N)."""
    ql = [int(q) for q in qs[:level]]
    col = pyoracle._mods_col(ql)
    D = 0
    for a, b in zip(As, Bs):
        D = (D + pyoracle.tensor_ntt(np.asarray(a)[:, :level], np.asarray(b)[:, :level], ql)) % col
    return D


def relin(D, evk_b, evk_a, qs, ps, dnum, level, rescale):
    """(D_0 + KS0(D_2), D_1 + KS1(D_2)) of a summed tensor (3, level, N), then optionally
    rescale_ntt: the tail of pyoracle.mul_relin."""
    ql = [int(q) for q in qs[:level]]
    col = pyoracle._mods_col(ql)
    ks0, ks1 = pyoracle.keyswitch(D[2], evk_b, evk_a, qs, ps, dnum, level=level, ntt=refs.c_ntt())
    out = np.stack([(D[0] + ks0) % col, (D[1] + ks1) % col])
    return rescaled(out, qs, level) if rescale else out


def rescaled(x, qs, level):
    """rescale_ntt of both polynomials of x (2, level, N) -> (2, level - 1, N)."""
    ql = [int(q) for q in qs[:level]]
    return np.stack([pyoracle.rescale_ntt(x[0], ql, refs.c_ntt()),
                     pyoracle.rescale_ntt(x[1], ql, refs.c_ntt())])


def mul_sum_relin(As, Bs, evk_b, evk_a, qs, ps, dnum, level, rescale):
    """[rescale]( Relin( sum_i As[i] x Bs[i] ) ) at `level`: As[i], Bs[i] (2, l_i >= level, N) NTT
    form, cut to `level` limbs.  -> (2, level, N), or (2, level - 1, N), object arrays."""
    return relin(tensor_sum(As, Bs, qs, level), evk_b, evk_a, qs, ps, dnum, level, rescale)


class CpuBackend(plain_ref.CpuBackend):
    """plain_ref's backend with the method fhecore.polyeval.inner_product calls."""

    def mul_sum_relin(self, as_, bs, rescale, level):
        return mul_sum_relin(as_, bs, self.evk_b, self.evk_a, self.moduli, self.ps, self.dnum,
                             level, rescale)


# ---- the shared decrypt case: log_n = 10, L = 4, K = 2, dnum = 2, a 50-bit chain, delta = 2^40
LOG_N, L, K, DNUM, BITS = 10, 4, 2, 2, 50
DELTA = 2.0 ** 40
COUNTS = (4, 16)
# Maximum slot error against numpy's sum_i z_i w_i on the CPU reference, measured once
# (deterministic under the seeds below).  FUSED: inner_product (one key-switch, one rescale);
# COMPOSED: mul_relin(rescale) per term, then the sum of the rescaled ciphertexts.
FUSED_ERR = {4: 9.72e-7, 16: 6.96e-7}
COMPOSED_ERR = {4: 1.57e-6, 16: 3.44e-6}  # the fused form: 0.62x and 0.20x of these


@functools.lru_cache(maxsize=None)
def setup():
    """Keys and 2 x 16 encrypted vectors from pyoracle with fixed seeds: dict of host arrays."""
    import coracle
    from fhecore.ckks import Encoder, to_rns

    n = 1 << LOG_N
    m = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K, bits=BITS)]
    qs, ps = m[:L], m[L:]
    rng = random.Random(4321)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    evk_b, evk_a = pyoracle.gen_relin_key(s, qs, ps, DNUM, rng)
    sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, m), m)
    g = np.random.default_rng(9)
    enc = Encoder(n)

    def fresh(seed):
        z = g.uniform(0, 1, n // 2) + 1j * g.uniform(0, 1, n // 2)  # the unit square
        pt = coracle.ntt_fwd(to_rns(enc.encode(z, DELTA), qs), qs)
        return z, np.asarray(pyoracle.encrypt_sk(seed, pt, sk_ntt, qs, LOG_N), dtype=np.uint64)

    xs = [fresh(100 + i) for i in range(max(COUNTS))]
    ys = [fresh(200 + i) for i in range(max(COUNTS))]
    return dict(qs=qs, ps=ps, evk_b=np.asarray(evk_b, dtype=np.uint64),
                evk_a=np.asarray(evk_a, dtype=np.uint64), sk_ntt=sk_ntt, enc=enc,
                z=[x[0] for x in xs], w=[y[0] for y in ys], x=[x[1] for x in xs],
                y=[y[1] for y in ys])


def decode(data, level, scale):
    """Decrypt (2, level, N), decode: the complex slots."""
    import coracle
    from fhecore.ckks import from_rns

    su = setup()
    ql = su["qs"][:level]
    dec = pyoracle.decrypt(np.asarray(data).astype(object), su["sk_ntt"], ql)
    coef = from_rns(coracle.ntt_inv(np.asarray(dec, dtype=np.uint64), ql), ql)
    return su["enc"].decode(coef, float(scale))


def expected(count):
    su = setup()
    return sum(z * w for z, w in zip(su["z"][:count], su["w"][:count]))


def slot_error(ct, count):
    """Maximum slot error of a polyeval.Ct (host data) against numpy's sum_i z_i w_i."""
    return float(np.abs(decode(ct.data, ct.level, ct.scale) - expected(count)).max())


def operands(count, wrap=lambda x: x):
    """The two Ct lists of the case at `count` terms; wrap moves a host array to the backend."""
    from fhecore import polyeval

    su = setup()
    return ([polyeval.Ct(wrap(t), L, DELTA) for t in su["x"][:count]],
            [polyeval.Ct(wrap(t), L, DELTA) for t in su["y"][:count]])


def backend():
    su = setup()
    return CpuBackend(su["qs"], su["ps"], DNUM, su["evk_b"], su["evk_a"])


@functools.lru_cache(maxsize=None)
def fused_cpu(count):
    """inner_product on the CPU backend: (Ct with a (2, L - 1, N) object array, max slot error)."""
    from fhecore import polyeval

    out = polyeval.inner_product(backend(), *operands(count))
    return out, slot_error(out, count)


@functools.lru_cache(maxsize=None)
def composed_cpu(count):
    """The composed form on the CPU backend: mul_relin(rescale) per term, then the sum of the
    rescaled ciphertexts.  (Ct, max slot error)."""
    from fhecore import polyeval

    be, su = backend(), setup()
    xs, ys = operands(count)
    col = pyoracle._mods_col(su["qs"][:L - 1])
    acc = 0
    for x, y in zip(xs, ys):
        acc = (acc + be.mul_relin(x.data, y.data, True)) % col
    out = polyeval.Ct(acc, L - 1, xs[0].scale * ys[0].scale / su["qs"][L - 1])
    return out, slot_error(out, count)
