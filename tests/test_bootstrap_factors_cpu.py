"""fhecore.bootstrap's CoeffToSlot / SlotToCoeff factors without a GPU: their product against
tests/encode_ref.py's special FFT (the stage network fhe_encode / fhe_decode fix) without its
bit-reversal, the diagonal counts and index sets, and the baby-step / giant-step placement against
a dense matrix product.

Tolerances are float64 round-off relative to the largest entry of the reference vector.  Measured
on the cases below: the factor products differ from encode_ref by at most 2.1e-15 (log_n = 11,
one group of 10 stages; 4e-16 with 3 groups) and SlotToCoeff o CoeffToSlot from n id by at most
4.9e-15; the placement reproduces the dense product to 1.1e-15.  Each bound is 4 times that."""
import numpy as np
import pytest

import encode_ref

TOL_PRODUCT = 4 * 2.1e-15
TOL_ROUND_TRIP = 4 * 4.9e-15
TOL_PLACEMENT = 4 * 1.1e-15

CASES = [(10, 1), (10, 3), (11, 1), (11, 2), (11, 3), (11, 5)]


def apply(factors, v):
    for f in factors:
        v = sum(d * np.roll(v, -k) for k, d in f.items())
    return v


def dense(f, n):
    a = np.zeros((n, n), dtype=np.complex128)
    j = np.arange(n)
    for k, d in f.items():
        a[j, (j + k) % n] += d
    return a


def slots(n):
    g = np.random.default_rng(1)
    return g.uniform(-1, 1, n) + 1j * g.uniform(-1, 1, n)


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("log_n,groups", CASES)
def test_factor_products_are_the_special_fft_without_its_bit_reversal(log_n, groups):
    from fhecore import bootstrap as bs

    n = 1 << (log_n - 1)
    rev = encode_ref._tables(log_n)[2]
    z = slots(n)
    cts = bs.dft_factors(log_n, groups, inverse=True)
    stc = bs.dft_factors(log_n, groups, inverse=False)
    assert len(cts) == len(stc) == groups
    # encode: the stages, then v[rev] (rev is an involution): undo it
    re, im = encode_ref.special_ifft(z.real, z.imag, log_n)
    want = np.empty(n, dtype=np.complex128)
    want[rev] = re + 1j * im
    e1 = rel(apply(cts, z), want)
    # decode: v[rev], then the stages: feed it z[rev]
    re, im = encode_ref.special_fft(z[rev].real, z[rev].imag, log_n)
    e2 = rel(apply(stc, z), re + 1j * im)
    e3 = rel(apply(stc, apply(cts, z)) / n, z)
    print(f"log_n {log_n}, {groups} groups: CoeffToSlot {e1:.2e}, SlotToCoeff {e2:.2e}, "
          f"round trip {e3:.2e}")
    assert e1 < TOL_PRODUCT and e2 < TOL_PRODUCT
    assert e3 < TOL_ROUND_TRIP


def test_diagonal_counts_and_indices_with_three_groups():
    """log_n = 10, 3 groups of 3 stages: 8, 15, 15 diagonals at stride a, a in -7 .. 7, strides 64,
    8, 1 (CoeffToSlot; at len = n the shifts +n/2 and -n/2 are one diagonal, so 8 not 15) and the
    mirror image for SlotToCoeff."""
    from fhecore import bootstrap as bs

    n = 512
    cts = bs.dft_factors(10, 3, inverse=True)
    stc = bs.dft_factors(10, 3, inverse=False)
    assert [len(f) for f in cts] == [8, 15, 15]
    assert [len(f) for f in stc] == [15, 15, 8]
    for f, stride in zip(cts + stc, (64, 8, 1, 1, 8, 64)):
        assert set(f) == {stride * a % n for a in range(-7, 8)}
    assert bs.factor_layouts(10, 3, True) == [(4, 2, 64, 0), (4, 4, 8, -7), (4, 4, 1, -7)]
    assert bs.factor_layouts(10, 3, False) == [(4, 4, 1, -7), (4, 4, 8, -7), (4, 2, 64, 0)]


def test_the_coinciding_diagonals_of_the_top_stage_are_added():
    """One stage per factor: the stage len = n has the diagonals 0 and n/2 only, and n/2 holds
    both the +lh entries (first half) and the -lh entries (second half)."""
    from fhecore import bootstrap as bs

    top = bs.dft_factors(10, 9, inverse=True)[0]
    assert set(top) == {0, 256}
    assert np.count_nonzero(top[256]) == 512
    assert (top[256][:256] == 1).all()


@pytest.mark.parametrize("log_n,groups", CASES)
def test_diagonal_counts(log_n, groups):
    """s merged stages: 2^(s+1) - 1 diagonals, 2^s for the factor that holds the stage len = n."""
    from fhecore import bootstrap as bs

    stages = log_n - 1
    sizes = bs.group_sizes(stages, groups)
    assert sum(sizes) == stages and max(sizes) - min(sizes) <= 1
    cts = bs.dft_factors(log_n, groups, inverse=True)
    stc = bs.dft_factors(log_n, groups, inverse=False)
    assert [len(f) for f in cts] == [1 << sizes[0]] + [(2 << s) - 1 for s in sizes[1:]]
    assert [len(f) for f in stc] == [(2 << s) - 1 for s in sizes[:-1]] + [1 << sizes[-1]]


@pytest.mark.parametrize("log_n,groups", CASES)
def test_strided_placement_against_a_dense_product(log_n, groups):
    """sum_g rot_{giant g}(sum_b z[g][b] rot_{baby b}(v)) = A v for the dense A of the diagonals."""
    from fhecore import bootstrap as bs

    n = 1 << (log_n - 1)
    v = slots(n)
    for inverse in (True, False):
        layouts = bs.factor_layouts(log_n, groups, inverse)
        for f, (n1, n2, stride, offset) in zip(bs.dft_factors(log_n, groups, inverse), layouts):
            z, baby, giant = bs.place_strided_diagonals(f, n, n1, n2, stride, offset)
            assert z.shape == (n2, n1, n)
            assert baby == [stride * (b + offset) for b in range(n1)]
            assert giant == [stride * g * n1 for g in range(n2)]
            # diagonal stride (g n1 + b + offset) sits at [g][b], rolled by stride g n1
            for g in range(n2):
                for b in range(n1):
                    k = stride * (g * n1 + b + offset) % n
                    want = np.roll(f[k], stride * g * n1) if k in f else np.zeros(n)
                    assert (z[g, b] == want).all()
            got = sum(np.roll(sum(z[g][b] * np.roll(v, -baby[b]) for b in range(n1)), -giant[g])
                      for g in range(n2))
            assert rel(got, dense(f, n) @ v) < TOL_PLACEMENT
            # no zero plaintexts beyond the padding of n1 n2
            used = sum(1 for g in range(n2) for b in range(n1) if z[g, b].any())
            assert used == len(f) and n1 * n2 - used <= 1


def test_placement_refusals():
    from fhecore import bootstrap as bs

    d = {k: np.ones(512) for k in (0, 8, 504)}
    with pytest.raises(ValueError, match="no place"):
        bs.place_strided_diagonals(d, 512, 2, 1, stride=8, offset=0)
    with pytest.raises(ValueError, match="two places"):
        bs.place_strided_diagonals({0: np.ones(512)}, 512, 4, 4, stride=64, offset=0)
    with pytest.raises(ValueError, match="groups"):
        bs.dft_factors(10, 10, True)
