"""The sum of ciphertext products with one relinearisation without a GPU: the C entry point exists
and refuses a null context, the reference (pyoracle.mul_sum_relin) is pinned against
pyoracle.mul_relin, against a permutation of its terms and against a direct big-integer evaluation
at the accumulators' bound, and fhecore.polyeval.inner_product on the CPU backend decrypts to the inner
product with no more error than the composed form."""
import random
from fractions import Fraction

import numpy as np
import pytest

import cases
import pyoracle
import refs

MS = cases.MULSUM
NTT = refs.c_ntt()


def test_surface():
    from fhecore import _capi

    assert "fhe_mul_sum_relin_level" in _capi.SIGNATURES
    assert hasattr(_capi.load(), "fhe_mul_sum_relin_level")


def test_entry_point_refuses_a_null_context():
    from fhecore import _capi

    lib = _capi.load()
    assert lib.fhe_mul_sum_relin_level(None, None, None, None, None, None, None, None, 1, 1, 1, 0,
                                       None, None) == -1
    assert b"null context" in lib.fhe_last_error()


@pytest.fixture(scope="module")
def world():
    """log_n = 10, L = 4, K = 2, dnum = 2 with a real relinearisation key and five uniform
    ciphertexts, one of them a level lower."""
    n, qs, ps, rng, _, evk_b, evk_a = refs.relin_setup(10, 4, 2, 2, seed=31)

    def uniform(level):
        return np.stack([np.stack([np.array([rng.randrange(q) for _ in range(n)], dtype=object)
                                   for q in qs[:level]]) for _ in range(2)])

    cts = [uniform(4), uniform(4), uniform(3), uniform(4), uniform(4)]
    return dict(qs=qs, ps=ps, dnum=2, evk_b=evk_b, evk_a=evk_a, cts=cts)


def test_one_term_is_mul_relin(world):
    w = world
    a, b = w["cts"][0], w["cts"][1]
    for level, rescale in ((4, False), (4, True), (2, True), (1, False)):
        got = pyoracle.mul_sum_relin([a], [b], w["evk_b"], w["evk_a"], w["qs"], w["ps"], w["dnum"],
                                     rescale, level=level, ntt=NTT)
        want = pyoracle.mul_relin(a[:, :level], b[:, :level], w["evk_b"], w["evk_a"], w["qs"],
                                  w["ps"], w["dnum"], rescale, level=level, ntt=NTT)
        assert got.shape == want.shape and (got == want).all(), (level, rescale)


def test_the_order_of_the_terms_does_not_matter(world):
    w = world
    c = w["cts"]
    As, Bs = [c[0], c[2], c[3], c[0]], [c[1], c[3], c[3], c[4]]  # mixed levels, a square, c0 twice
    tail = (w["evk_b"], w["evk_a"], w["qs"], w["ps"], w["dnum"], True)
    kw = dict(level=3, ntt=NTT)
    want = pyoracle.mul_sum_relin(As, Bs, *tail, **kw)
    assert want.shape == (2, 2, 1 << 10)
    for perm in ((3, 2, 1, 0), (1, 3, 0, 2)):
        got = pyoracle.mul_sum_relin([As[i] for i in perm], [Bs[i] for i in perm], *tail, **kw)
        assert (got == want).all(), perm
    # a x b is b x a term by term
    assert (pyoracle.mul_sum_relin(Bs, As, *tail, **kw) == want).all()


def test_the_bound_of_the_accumulators_against_big_integers():
    """Every residue q_j - 1 in 16 terms on a 62-bit chain: D_0 = D_2 = 16 (q - 1)^2 and D_1 =
    32 (q - 1)^2, the largest sums the definition allows, evaluated directly as Python integers
    (16, 32, 16 mod q_j) and relinearised from there."""
    log_n, L, K, dnum, count = 10, 3, 2, 2, 16
    n = 1 << log_n
    m = [int(q) for q in pyoracle.gen_moduli(log_n, L + K, bits=62)]
    qs, ps = m[:L], m[L:]
    assert all(q >> 61 == 1 for q in m)
    rng = random.Random(5)
    evk_b, evk_a = pyoracle.gen_relin_key([rng.randrange(-1, 2) for _ in range(n)], qs, ps, dnum, rng)
    top = np.stack([np.stack([np.full(n, q - 1, dtype=object) for q in qs])] * 2)
    for level in (3, 2):
        D = pyoracle.tensor_sum([top] * count, [top] * count, qs, level=level)
        direct = np.stack([np.stack([np.full(n, k * count * (q - 1) ** 2 % q, dtype=object)
                                     for q in qs[:level]]) for k in (1, 2, 1)])
        assert (D == direct).all(), level
        assert all(int(direct[k, j, 0]) == (16, 32, 16)[k] for k in range(3) for j in range(level))
        got = pyoracle.mul_sum_relin([top] * count, [top] * count, evk_b, evk_a, qs, ps, dnum, True,
                                     level=level, ntt=NTT)
        want = pyoracle.relin(direct, evk_b, evk_a, qs, ps, dnum, True, level=level, ntt=NTT)
        assert (got == want).all(), level


@pytest.mark.parametrize("count", cases.COUNTS)
def test_inner_product_cpu_backend(count):
    """log_n = 10, L = 4, K = 2, dnum = 2, a 50-bit chain, delta = 2^40, 512 complex slots uniform
    in the unit square: the decrypted, decoded inner product against numpy's sum_i z_i w_i.  The
    fused form (one key-switch, one rescale rounding) must not exceed the composed form (count of
    each), and stays within 1.5x of its recorded error, the margin covering libm differences in
    the encoder only."""
    out, err = cases.run_cpu(MS, count)
    ref, ref_err = cases.run_cpu(MS, count, cases.composed)
    print(f"count {count}: fused max slot error {err:.3e}, composed {ref_err:.3e}")
    qs = cases.setup(MS)["qs"]
    assert out.level == MS.L - 1 and out.data.shape == (2, out.level, 1 << MS.log_n)
    assert out.scale == Fraction(MS.delta) ** 2 / qs[MS.L - 1]
    assert err <= ref_err
    assert err < 1.5 * cases.FUSED_ERR[count]


def test_inner_product_errors():
    from fhecore import polyeval

    be = cases.backend(MS)
    xs, ys = cases.mulsum_operands(2)
    with pytest.raises(ValueError, match="one length"):
        polyeval.inner_product(be, xs, ys[:1])
    with pytest.raises(ValueError, match="one length"):
        polyeval.inner_product(be, [], [])
    off = [ys[0], polyeval.Ct(ys[1].data, ys[1].level, 2 * MS.delta)]
    with pytest.raises(ValueError, match="one scale"):
        polyeval.inner_product(be, xs, off)
    low = [polyeval.Ct(x.data[:, :1], 1, x.scale) for x in xs]
    with pytest.raises(ValueError, match="lowest level"):
        polyeval.inner_product(be, low, ys)
