"""Reference for the level-aware plaintext arithmetic (fhe_lincomb_level, fhe_mul_plain_level;
include/fhecore.h) in exact Python-integer arithmetic over (2, l, N) object arrays, the CPU backend
of fhecore.polyeval built from it and pyoracle.mul_relin, and the Chebyshev case the CPU and GPU
tests share (computed once per process)."""
import functools
import random

import numpy as np

import pyoracle
import refs


def _rescale(x, ql):
    return np.stack([pyoracle.rescale_ntt(x[0], ql, refs.c_ntt()),
                     pyoracle.rescale_ntt(x[1], ql, refs.c_ntt())])


def lincomb_level(cts, scalars, qs, level, const=None, rescale=False):
    """sum_i scalars[i] cts[i][:, :level] (+ const on every slot of c0) mod q_j, then optionally
    rescale_ntt.  cts[i] (2, l_i >= level, N) NTT form; scalars / const Python integers (reduced
    per limb here).  -> (2, level, N), or (2, level - 1, N), object arrays."""
    ql = [int(q) for q in qs[:level]]
    col = pyoracle._mods_col(ql)
    acc = np.zeros((2, level, np.asarray(cts[0]).shape[-1]), dtype=object)
    for k, ct in zip(scalars, cts):
        kcol = np.array([int(k) % q for q in ql], dtype=object).reshape(-1, 1)
        acc = (acc + np.asarray(ct).astype(object)[:, :level] * kcol) % col
    if const is not None:
        acc[0] = (acc[0] + np.array([int(const) % q for q in ql], dtype=object).reshape(-1, 1)) % col
    return _rescale(acc, ql) if rescale else acc


def mul_plain_level(ct, pt, qs, level, rescale=False):
    """ct (2, level, N) times the first `level` rows of pt (rows >= level, N), NTT form."""
    ql = [int(q) for q in qs[:level]]
    out = np.asarray(ct).astype(object) * np.asarray(pt).astype(object)[:level] % pyoracle._mods_col(ql)
    return _rescale(out, ql) if rescale else out


class CpuBackend:
    """fhecore.polyeval backend over (2, l, N) numpy arrays: pyoracle.mul_relin and the
    functions above."""

    def __init__(self, qs, ps, dnum, evk_b, evk_a):
        self.moduli, self.ps, self.dnum = [int(q) for q in qs], [int(p) for p in ps], dnum
        self.evk_b, self.evk_a = evk_b, evk_a

    def mul_relin(self, a, b, rescale):
        return pyoracle.mul_relin(a, b, self.evk_b, self.evk_a, self.moduli, self.ps, self.dnum,
                                  rescale, level=np.asarray(a).shape[-2], ntt=refs.c_ntt())

    def lincomb(self, cts, scalars, const, rescale, level):
        n = len(cts)
        return lincomb_level(cts, scalars[:n], self.moduli, level,
                             const=scalars[n] if const else None, rescale=rescale)

    def drop_level(self, a, level):
        return np.asarray(a)[:, :level]


# ---- the shared Chebyshev case: log_n = 10, L = 8, K = 2, dnum = 4, a 50-bit chain, delta = 2^50
LOG_N, L, K, DNUM, BITS = 10, 8, 2, 4, 50
DELTA = 2.0 ** 50
# maximum slot error of chebyshev_eval on the CPU backend against chebval, measured once
# (deterministic under the seeds below): degree 7 and degree 15 of cos(2x)
CHEB_ERR_DEG7 = 2.06e-12
CHEB_ERR_DEG15 = 2.03e-12


@functools.lru_cache(maxsize=None)
def cheb_setup():
    """Keys and the encrypted input from pyoracle with fixed seeds: dict of host arrays."""
    import coracle
    from fhecore.ckks import Encoder, to_rns

    n = 1 << LOG_N
    m = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K, bits=BITS)]
    qs, ps = m[:L], m[L:]
    rng = random.Random(1234)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    evk_b, evk_a = pyoracle.gen_relin_key(s, qs, ps, DNUM, rng)
    sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, m), m)
    x = np.random.default_rng(5).uniform(-1, 1, n // 2)
    enc = Encoder(n)
    pt = coracle.ntt_fwd(to_rns(enc.encode(x, DELTA), qs), qs)
    ct = pyoracle.encrypt_sk(77, pt, sk_ntt, qs, LOG_N)
    return dict(qs=qs, ps=ps, evk_b=evk_b, evk_a=evk_a, sk_ntt=sk_ntt, x=x, ct=ct, enc=enc)


def cheb_coeffs(degree):
    """Chebyshev interpolant of cos(2x) on [-1, 1]."""
    return np.polynomial.chebyshev.chebinterpolate(lambda t: np.cos(2 * t), degree)


def cheb_decode(data, level, scale):
    """Decrypt (2, level, N), decode: the real parts of the slots."""
    import coracle
    from fhecore.ckks import from_rns

    su = cheb_setup()
    ql = su["qs"][:level]
    dec = pyoracle.decrypt(np.asarray(data).astype(object), su["sk_ntt"], ql)
    coef = from_rns(coracle.ntt_inv(np.asarray(dec, dtype=np.uint64), ql), ql)
    return su["enc"].decode(coef, float(scale)).real


@functools.lru_cache(maxsize=None)
def cheb_cpu(degree):
    """chebyshev_eval on the CPU backend: (Ct with a (2, l, N) object array, max slot error)."""
    from fhecore import polyeval

    su = cheb_setup()
    be = CpuBackend(su["qs"], su["ps"], DNUM, su["evk_b"], su["evk_a"])
    c = cheb_coeffs(degree)
    out = polyeval.chebyshev_eval(be, polyeval.Ct(su["ct"], L, DELTA), c)
    got = cheb_decode(out.data, out.level, out.scale)
    err = float(np.abs(got - np.polynomial.chebyshev.chebval(su["x"], c)).max())
    return out, err
