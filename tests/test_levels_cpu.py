"""Level-aware key-switch without a GPU: pyoracle.keyswitch at a level is pinned against real
relinearisation keys and against its own top-level form wherever the truncated digit ranges coincide
with those of a shorter chain, and the C entry points (fhe_keyswitch_level, fhe_mul_relin_level,
fhe_rotate_level) refuse a null context."""
import numpy as np
import pytest

import pyoracle
import refs


@pytest.mark.parametrize("log_n,L,K,dnum,coincide_at_least", [(6, 5, 2, 3, {2, 3, 4, 5}),
                                                              (6, 7, 4, 2, {7})])
def test_keyswitch_level_switches_the_key_at_every_level(log_n, L, K, dnum, coincide_at_least):
    """ks0 + ks1 s = d2 s^2 + e with the top-level key at every level l = 1 .. L.  The bound 2^10
    on the centred error: the restatement measured at most 6 bits at (N, L, K, dnum) = (64, 5, 2, 3)
    (ternary s, errors in [-3, 3], the ModDown rounding), so 4 bits of margin for another seed.
    Where some dnum' makes pyoracle.digit_ranges(l, dnum') equal the truncated ranges, the result
    equals the top-level pyoracle.keyswitch of the l-limb chain on the sliced key word for word."""
    n, qs, ps, rng, s, evk_b, evk_a = refs.relin_setup(log_n, L, K, dnum, seed=20 + L)
    coincided = set()
    for level in range(1, L + 1):
        ql = qs[:level]
        d2 = np.stack([np.array([rng.randrange(q) for _ in range(n)], dtype=object) for q in ql])
        ks0, ks1 = pyoracle.keyswitch(d2, evk_b, evk_a, qs, ps, dnum, level=level,
                                      ntt=refs.c_ntt())
        col = pyoracle._mods_col(ql)
        s_n = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, ql), ql)
        diff = (ks0 + ks1 * s_n - d2 * s_n * s_n) % col
        err = pyoracle.crt_centered(pyoracle.rns_ntt_inv(diff, ql), ql)
        bits = max(abs(int(v)) for v in err).bit_length()
        print(f"L={L} dnum={dnum} level={level} error bits {bits}")
        assert bits <= 10, (level, bits)
        digits = pyoracle.digit_ranges(L, dnum, level)
        rows = pyoracle.key_rows(level, L, K)
        for dn in range(1, level + 1):
            if pyoracle.digit_ranges(level, dn) != digits:
                continue
            w0, w1 = pyoracle.keyswitch(d2, evk_b[:len(digits)][:, rows],
                                        evk_a[:len(digits)][:, rows], ql, ps, dn)
            assert (w0 == ks0).all() and (w1 == ks1).all(), level
            coincided.add(level)
            break
    assert coincided >= coincide_at_least, coincided


def test_level_digits_and_key_rows():
    assert pyoracle.digit_ranges(5, 3, 5) == pyoracle.digit_ranges(5, 3)
    assert pyoracle.digit_ranges(5, 3, 3) == [(0, 2), (2, 3)]
    assert pyoracle.digit_ranges(16, 4, 5) == [(0, 4), (4, 5)]  # no dnum' gives these ranges
    assert all(pyoracle.digit_ranges(5, dn) != [(0, 4), (4, 5)] for dn in range(1, 6))
    assert pyoracle.digit_ranges(16, 4, 13) == pyoracle.digit_ranges(13, 4)
    assert pyoracle.key_rows(2, 5, 2) == [0, 1, 5, 6]


def test_level_entry_points_refuse_a_null_context():
    """As test_capi.py's null-context checks: -1 before any HIP call; the workspace sizes, which
    cover every level, stay 0 for a null context."""
    from fhecore import _capi

    lib = _capi.load()
    assert lib.fhe_keyswitch_level(None, None, None, None, None, None, 1, 1, None, None) == -1
    assert lib.fhe_mul_relin_level(None, None, None, None, None, None, 1, 1, 0, None, None) == -1
    assert lib.fhe_rotate_level(None, None, None, 5, None, None, 1, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_keyswitch_workspace(None, 1, 1) == 0
    assert lib.fhe_mul_relin_workspace(None, 1) == 0
    assert lib.fhe_rotate_workspace(None, 1) == 0
