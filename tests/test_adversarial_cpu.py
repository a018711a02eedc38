"""tests/adversarial.py does what it says, and the two oracles agree on it (no GPU, N = 2^10).

The GPU kernels are judged against coracle and pyoracle on these inputs
(tests/test_gpu_adversarial.py); here the inputs are checked to sit where they claim to sit --
both sides of the rescale wrap, exact zeros, the top of the conversion sums -- and the C oracle is
pinned to pyoracle, which stays the definition, on every family."""
import math

import numpy as np
import pytest

import adversarial as adv
import coracle
import pyoracle
import refs

LOG_N = 10
N = 1 << LOG_N


def _g(bits, count, skip=0):
    return pyoracle.gen_moduli(LOG_N, count, bits=bits, skip=skip)


RESCALE_CHAINS = {
    "b60": lambda: _g(60, 3),
    "q0-60-over-50": lambda: _g(60, 1) + _g(50, 3),
    "50-50-under-60": lambda: _g(50, 2) + _g(60, 1),
}


@pytest.mark.parametrize("name", sorted(RESCALE_CHAINS))
def test_rescale_boundary_sits_on_the_wrap_and_the_oracles_agree(name):
    mods = RESCALE_CHAINS[name]()
    l, ql = len(mods), mods[-1]
    h = (ql - 1) // 2
    assert h == ql // 2
    x = adv.rescale_boundary(mods, LOG_N, 3)
    assert x.dtype == np.uint64 and x.shape == (3, l, N)
    assert (x == adv.rescale_boundary(mods, LOG_N, 3)).all()  # deterministic
    edges = adv.rescale_edges(ql)
    assert edges == [0, 1, h - 1, h, h + 1, h + 2, ql - 1] and len(set(edges)) == 7
    for p in range(3):
        xo = x[p].astype(object)
        assert all(int(row.max()) < q for row, q in zip(xo, mods))  # canonical residues
        last = xo[-1]
        for e in edges:
            assert (last == e).sum() >= N // 8, (p, e)
        # both sides of the wrap: x = h lifts to h, x = h + 1 to h + 1 - q_last = -h
        lift = (last + h) % ql - h
        assert (lift[last == h] == h).all() and (lift[last == h + 1] == -h).all()
        assert (last == h).any() and (last == h + 1).any()
        want = pyoracle.rescale_exact(xo, mods)
        got = pyoracle.rescale_coeff(xo, mods)
        assert (got == want).all()
        for j in range(l - 1):
            assert (got[j] == 0).sum() >= N // 4, (p, j)
            assert (xo[j] == mods[j] - 1).sum() >= N // 4, (p, j)
    # the NTT-form variant is the same array through the forward NTT
    xn = adv.rescale_boundary_ntt(mods, LOG_N, 2)
    assert (coracle.ntt_inv(xn, mods) == x[:2]).all()


def _ks_chain(bits, L, K):
    m = _g(bits, L + K)
    return m[:L], m[L:]


def _fractions(qs, ps, dnum):
    """(best ModUp target fraction, best ModDown target fraction) of conv_worst on a chain."""
    allm = qs + ps
    up = []
    for lo, hi in pyoracle.digit_ranges(len(qs), dnum):
        others = [allm[i] for i in range(len(allm)) if not lo <= i < hi]
        up += adv.conv_fraction(qs[lo:hi], others)
    return max(up), max(adv.conv_fraction(ps, qs))


@pytest.mark.parametrize("src", [lambda: _g(60, 1), lambda: _g(60, 2), lambda: _g(61, 4),
                                 lambda: _g(62, 3), lambda: adv.far_chain()[0]])
def test_conv_worst_makes_every_y_the_largest(src):
    src = src()
    x = adv.conv_worst(src, LOG_N)
    assert x.dtype == np.uint64 and x.shape == (len(src), N)
    S = math.prod(src)
    for i, s in enumerate(src):
        y = x[i].astype(object) * pow((S // s) % s, -1, s) % s
        assert (y == s - 1).all(), i


@pytest.mark.parametrize("bits", [60, 61])
def test_conv_worst_reaches_the_top_of_the_sums(bits):
    """L = 4, K = 2, dnum = 2 on the default chains: (S / s_i) mod t lands just below t for the
    targets above the sources (descending primes), so the unreduced sum reaches the bound."""
    qs, ps = _ks_chain(bits, 4, 2)
    up, down = _fractions(qs, ps, 2)
    print(f"b{bits}: ModUp {up:.4f}, ModDown {down:.4f} of alpha max(s) t")
    assert up >= 0.99 and down >= 0.99
    # the reference's own sums, term by term from the input (y_i = x_i (S / s_i)^-1 mod s_i, then
    # sum_i y_i ((S / s_i) mod t) unreduced), on the worst target of ModDown and of each ModUp digit
    allm = qs + ps
    cases = [(ps, qs)]
    for lo, hi in pyoracle.digit_ranges(len(qs), 2):
        cases.append((qs[lo:hi], [allm[i] for i in range(len(allm)) if not lo <= i < hi]))
    best = []
    for src, dst in cases:
        x = adv.conv_worst(src, LOG_N).astype(object)
        S = math.prod(src)
        t = dst[int(np.argmax(adv.conv_fraction(src, dst)))]
        total = sum(x[i][0] * pow((S // s) % s, -1, s) % s * ((S // s) % t)
                    for i, s in enumerate(src))
        assert (pyoracle.baseconv(x, src, [t])[0] == total % t).all()
        best.append(total / (len(src) * max(src) * t))
    assert best[0] >= 0.99 and max(best[1:]) >= 0.99  # ModDown, ModUp


def test_far_chain_is_the_one_of_the_width_tests():
    """adv.far_chain restates tests/test_gpu_wide.py's `far` chain (that file builds it next to its
    device contexts); the two must stay the same primes."""
    import test_gpu_wide

    assert adv.far_chain() == test_gpu_wide._chain(None, "far")


def test_conv_fraction_of_the_other_chains_is_reported():
    """Not asserted: chains whose (S / s_i) mod t is not near t stay well below the bound."""
    qs, ps = adv.far_chain()
    up, down = _fractions(qs, ps, 2)
    print(f"far: ModUp {up:.4f}, ModDown {down:.4f}")
    qs, ps = _ks_chain(62, 4, 2)
    up, down = _fractions(qs, ps, 2)
    print(f"b62: ModUp {up:.4f}, ModDown {down:.4f}")


# (bits, L, K, dnum): the default chains, and a ragged last digit (7 = 3 + 3 + 1)
ORACLE_CHAINS = [(60, 4, 2, 2), (61, 4, 2, 2), (62, 4, 2, 2), (60, 7, 2, 3)]


@pytest.mark.parametrize("bits,L,K,dnum", ORACLE_CHAINS)
def test_oracles_agree_on_the_families(bits, L, K, dnum):
    qs, ps = _ks_chain(bits, L, K)
    allm = qs + ps
    keys = {k: adv.ks_keys(k, allm, dnum, LOG_N) for k in ("tm1", "select_0")}
    for kind in adv.D2_KINDS:
        d2 = adv.ks_d2(kind, qs, ps, dnum, LOG_N)
        assert d2.dtype == np.uint64 and d2.shape == (L, N)
        c = coracle.ntt_inv(d2, qs)
        assert (c.astype(object) == pyoracle.rns_ntt_inv(d2, qs)).all(), kind
        assert (coracle.ntt_fwd(c, qs) == d2).all(), kind
        assert (coracle.ntt_fwd(c, qs).astype(object) == pyoracle.rns_ntt_fwd(c, qs)).all(), kind
        for kname, (kb, ka) in keys.items():
            w0, w1 = pyoracle.keyswitch(d2, kb, ka, qs, ps, dnum)
            g0, g1 = coracle.keyswitch(d2, kb, ka, qs, ps, dnum)
            assert (g0.astype(object) == w0).all(), (kind, kname, 0)
            assert (g1.astype(object) == w1).all(), (kind, kname, 1)
            if kind == "zero" or kname == "select_0":
                assert not g1.any(), (kind, kname)  # exact zeros
            if kind == "zero":
                assert not g0.any(), (kind, kname)
    # the conversions themselves: every digit's ModUp and the ModDown, worst case and zero
    for lo, hi in pyoracle.digit_ranges(L, dnum):
        dst = [allm[i] for i in range(L + K) if not lo <= i < hi]
        for x in (adv.conv_worst(qs[lo:hi], LOG_N), np.zeros((hi - lo, N), dtype=np.uint64)):
            got = coracle.baseconv(x, qs[lo:hi], dst)
            assert (got.astype(object) == pyoracle.baseconv(x, qs[lo:hi], dst)).all(), (lo, hi)
            assert x.any() or not got.any()
    x = adv.conv_worst(ps, LOG_N)
    assert (coracle.baseconv(x, ps, qs).astype(object) == pyoracle.baseconv(x, ps, qs)).all()


def test_selector_key_returns_the_digit_through_moddown():
    """select_j: acc0 = NTT(ModUp(digit j)) and acc1 = 0, so ks1 = 0 and ks0 is ModDown of the
    extended digit; the key below the top level selects the same digit (the level reads its live
    rows)."""
    L, K, dnum = 5, 2, 3
    qs, ps = _ks_chain(60, L, K)
    allm = qs + ps
    d2 = adv.ks_d2("modup_worst", qs, ps, dnum, LOG_N)
    for j, kname in ((0, "select_0"), (dnum - 1, "select_last")):
        kb, ka = adv.ks_keys(kname, allm, dnum, LOG_N)
        assert (kb[j] == 1).all() and kb.sum() == (L + K) * N and not ka.any()
        ext = pyoracle.modup(pyoracle.rns_ntt_inv(d2, qs), qs, ps, dnum)[j]
        want = pyoracle.moddown_ntt(pyoracle.rns_ntt_fwd(ext, allm), qs, ps)
        g0, g1 = coracle.keyswitch(d2, kb, ka, qs, ps, dnum)
        assert (g0.astype(object) == want).all() and not g1.any(), kname
    # below the top: a partial last digit (level 3: digits [0, 2), [2, 3)) and level 1
    kb, ka = adv.ks_keys("select_0", allm, dnum, LOG_N)
    for level in (3, 1):
        assert pyoracle.digit_ranges(L, dnum, level) == {3: [(0, 2), (2, 3)], 1: [(0, 1)]}[level]
        for kind in ("zero", "modup_worst"):
            d = adv.ks_d2(kind, qs, ps, dnum, LOG_N, level=level)
            assert d.shape == (level, N)
            r0, r1 = pyoracle.keyswitch(d, kb, ka, qs, ps, dnum, level=level, ntt=refs.c_ntt())
            assert not r1.any() and (kind != "zero" or not r0.any()), (level, kind)
