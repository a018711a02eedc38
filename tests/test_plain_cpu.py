"""Level-aware plaintext arithmetic and the Chebyshev evaluator without a GPU: the new C entry
points exist and refuse a null context, the reference (pyoracle.lincomb / mul_plain) is pinned
against a direct CRT computation over Z[X]/(X^N + 1), and fhecore.polyeval.chebyshev_eval on the
CPU backend decrypts to the series it was given."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import cases
import coracle
import pyoracle
import refs

CHEB = cases.CHEB


def test_surface():
    from fhecore import _capi

    for name in ("fhe_lincomb_workspace", "fhe_lincomb_level", "fhe_mul_plain_level"):
        assert name in _capi.SIGNATURES
        assert hasattr(_capi.load(), name)


def test_plain_entry_points_refuse_a_null_context():
    from fhecore import _capi

    lib = _capi.load()
    assert lib.fhe_lincomb_level(None, None, None, None, None, 1, 0, 1, 1, 1, 0, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_mul_plain_level(None, None, None, None, 1, 1, 1, 1, 0, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_lincomb_workspace(None, 1) == 0


def _negacyclic(a, b):
    """Exact product in Z[X]/(X^N + 1) of Python-integer coefficient lists."""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * y
                else:
                    out[k - n] -= x * y
    return out


def test_plain_ref_against_direct_crt():
    """k_1 a + k_2 b + k_0 over Z[X]/(X^N + 1) for small-coefficient polynomials lifted to the
    integers, reduced mod each prime, equals pyoracle.lincomb on their NTT forms; after rescale both
    equal floor((X + q/2) / q) of the CRT value X in [0, Q).  mul_plain is the negacyclic
    product.  A 'ciphertext' here is any pair of polynomials: the constant goes to the first."""
    log_n, nl = 10, 3
    n = 1 << log_n
    qs = [int(q) for q in pyoracle.gen_moduli(log_n, nl)]
    Q = math.prod(qs)
    rng = random.Random(3)
    polys = [[[rng.randrange(-1000, 1001) for _ in range(n)] for _ in range(2)] for _ in range(2)]
    k1, k2, k0 = -(1 << 70) + 12345, (1 << 59) + 7, -(1 << 65) + 99

    def ntt(p, ql):
        return coracle.ntt_fwd(np.asarray(pyoracle._to_rns(p, ql), dtype=np.uint64), ql)

    a, b = (np.stack([ntt(p, qs) for p in pair]) for pair in polys)
    direct = [[k1 * x + k2 * y for x, y in zip(polys[0][h], polys[1][h])] for h in range(2)]
    direct[0][0] += k0  # the constant polynomial k_0
    for level in (3, 2):
        ql = qs[:level]
        got = pyoracle.lincomb([a, b], [k1, k2], qs, level=level, const=k0)
        assert got.shape == (2, level, n)
        for h in range(2):
            assert (got[h] == ntt(direct[h], ql).astype(object)).all(), (level, h)
        res = pyoracle.lincomb([a, b], [k1, k2], qs, level=level, const=k0, rescale=True,
                               ntt=refs.c_ntt())
        Ql = math.prod(ql)
        for h in range(2):
            want = [((v % Ql) + ql[-1] // 2) // ql[-1] for v in direct[h]]
            assert (res[h] == ntt(want, ql[:-1]).astype(object)).all(), (level, h, "rescaled")
    # a scalar of zero drops its term; one term with scalar 1 is the slice
    assert (pyoracle.lincomb([a, b], [1, 0], qs, level=2) == a[:, :2].astype(object)).all()
    pt = ntt(polys[1][0], qs)
    prods = [_negacyclic(polys[0][h], polys[1][0]) for h in range(2)]
    got = pyoracle.mul_plain(a[:, :2], pt, qs, level=2)
    for h in range(2):
        assert (got[h] == ntt(prods[h], qs[:2]).astype(object)).all()
    res = pyoracle.mul_plain(a, pt, qs, level=3, rescale=True, ntt=refs.c_ntt())
    for h in range(2):
        want = [((v % Q) + qs[-1] // 2) // qs[-1] for v in prods[h]]
        assert (res[h] == ntt(want, qs[:2]).astype(object)).all()


def test_chebyshev_eval_cpu_backend():
    """Degree 7, cos(2x) interpolated, log_n = 10, L = 8, K = 2, dnum = 4, 50-bit chain, delta =
    2^50, 512 real slots uniform in [-1, 1]: the decrypted, decoded result against
    numpy.polynomial.chebyshev.chebval.  Measured maximum slot error of this run: 2.06e-12 (2^-38.8;
    the level-4 result sits exactly at scale 2^50); asserted below 4x that, the margin covering FFT
    rounding differences between numpy builds only."""
    from fhecore import polyeval

    out, err = cases.run_cpu(CHEB, 7)
    print(f"degree 7: level {out.level}, max slot error {err:.3e}")
    assert out.level == CHEB.L - polyeval.levels_needed(7) == 4
    assert out.scale == Fraction(CHEB.delta)
    assert err < 4 * cases.CHEB_ERR_DEG7


def test_chebyshev_eval_errors():
    from fhecore import polyeval

    su, be = cases.setup(CHEB), cases.backend(CHEB)
    c = cases.cheb_coeffs(7)
    # degree 7 consumes 4 levels and must leave one: level 4 is too low (nothing is computed)
    with pytest.raises(ValueError, match="too few levels"):
        polyeval.chebyshev_eval(be, polyeval.Ct(su["ct"][:, :4], 4, CHEB.delta), c)
    with pytest.raises(ValueError, match="degree"):
        polyeval.chebyshev_eval(be, polyeval.Ct(su["ct"], CHEB.L, CHEB.delta), [1.0] * 65)
    # a scale far from the primes: T_3 = 2 T_2 T_1 - T_1 meets scales 1.37^3 and 1.37 times 2^50
    with pytest.raises(ValueError, match="not an integer"):
        polyeval.chebyshev_eval(be, polyeval.Ct(su["ct"], CHEB.L, 1.37 * CHEB.delta), c)
    assert [polyeval.levels_needed(d) for d in (1, 3, 7, 15, 31, 63)] == [1, 2, 4, 5, 6, 7]
