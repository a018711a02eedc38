"""fhecore.bootstrap.Bootstrapper without a GPU, on the CPU backend and the shared case of
tests/cases.py (BOOTSTRAP): the refreshed ciphertext decrypts to the input slots, its level and
scale, the refusals; and the self-checks of pyoracle.sparse_secret_coefficients, whose secret the
case uses."""
from fractions import Fraction

import numpy as np
import pytest

import bootstrap_ref as br
import cases
import pyoracle
import refs


def test_bootstrap_decrypts_to_the_input_slots():
    """Maximum slot error of this run: 2.833e-05 (deterministic under the fixed seeds; the margin
    covers float differences between numpy builds in encode / decode only)."""
    out, err = cases.run_cpu(cases.BOOTSTRAP)
    print(f"bootstrap: level {out.level}, scale / delta {float(out.scale) / br.DELTA:.12f}, "
          f"max slot error {err:.4e}")
    assert err < cases.MARGIN * cases.BOOTSTRAP_ERR


def test_bootstrap_level_and_scale():
    from fhecore import bootstrap as bs
    from fhecore import polyeval

    out, _ = cases.run_cpu(cases.BOOTSTRAP)
    assert polyeval.eval_mod_levels(31, 3) == 9
    assert out.level == br.L - 3 - 9 - 3 == br.OUT_LEVEL
    assert np.asarray(out.data).shape == (2, br.OUT_LEVEL, 1 << br.LOG_N)
    assert isinstance(out.scale, Fraction)
    # the result comes back at the input's scale up to the evaluator's drift (the primes sit
    # ~2^-30 off delta, three double angles)
    assert abs(out.scale / Fraction(br.DELTA) - 1) < Fraction(1, 1 << 26)
    boot = bs.Bootstrapper(cases.backend(cases.BOOTSTRAP), **br.PARAMS)
    assert boot.out_level == br.OUT_LEVEL
    # the declared scale in front of eval_mod is delta up to the rounding of the constants' roots
    assert abs(boot.scale_cts / Fraction(br.DELTA) - 1) < Fraction(1, 1 << 48)


def test_the_raised_ciphertext_stays_inside_eval_mods_range():
    """|I| <= (h + 2) / 2 = 15 = K - 1 for the case's secret of weight 28."""
    su = cases.setup(cases.BOOTSTRAP)
    qs = su["qs"]
    up = pyoracle.mod_raise(np.asarray(su["ct"])[:, :1], qs, 1, 2, ntt=refs.c_ntt())
    dec = pyoracle.decrypt(up, su["sk_ntt"], qs[:2])
    import encode_ref

    t = encode_ref.centred(np.asarray(dec).astype(np.uint64), qs, 2)
    big_i = np.array([round(Fraction(int(v), qs[0])) for v in t])
    print(f"max |I| = {np.abs(big_i).max()}")
    assert np.abs(big_i).max() <= (br.HAMMING + 2) // 2 == br.PARAMS["K"] - 1


def test_bootstrapper_refusals():
    from fhecore import bootstrap as bs

    be = cases.backend(cases.BOOTSTRAP)
    with pytest.raises(ValueError, match="Hamming weight"):
        bs.Bootstrapper(be, **dict(br.PARAMS, hamming_weight=29))
    with pytest.raises(ValueError, match="too short"):
        bs.Bootstrapper(be, **dict(br.PARAMS, double_angles=6))
    with pytest.raises(ValueError, match="not both"):
        bs.Bootstrapper(be, bs.BootstrapParams(), K=16)
    p = bs.BootstrapParams()
    assert (p.K, p.degree, p.double_angles, p.cts_groups, p.stc_groups) == (16, 31, 3, 3, 3)
    assert p.hamming_weight == 2 * p.K - 4 == 28


# ---- the sparse secret ----------------------------------------------------------------------------

@pytest.mark.parametrize("h", [1, 28, 64, 1023, 1024])
def test_sparse_ref_weight_is_exact(h):
    s = pyoracle.sparse_secret_coefficients(5, h, 10)
    assert s.shape == (1024,) and set(np.unique(s)) <= {-1, 0, 1}
    assert np.count_nonzero(s) == h


def test_sparse_ref_is_deterministic_and_seeded():
    a = pyoracle.sparse_secret_coefficients(5, 28, 10)
    b = pyoracle.sparse_secret_coefficients(5, 28, 10)
    assert (a == b).all()
    c = pyoracle.sparse_secret_coefficients(6, 28, 10)
    assert (a != c).any() and (np.flatnonzero(a) != np.flatnonzero(c)).any()
    # both signs occur, and a larger weight keeps the smaller one's support (one order of keys)
    assert {-1, 1} <= set(a)
    big = pyoracle.sparse_secret_coefficients(5, 64, 10)
    assert (big[a != 0] == a[a != 0]).all()


def test_sparse_ref_secret_is_the_same_integer_on_every_limb():
    import coracle

    m = [int(q) for q in pyoracle.gen_moduli(10, 3)]
    sk = pyoracle.keygen_secret_sparse(5, 28, m, 10)
    s = pyoracle.sparse_secret_coefficients(5, 28, 10)
    back = coracle.ntt_inv(np.asarray(sk).astype(np.uint64), m)
    for row, q in zip(back, m):
        assert (row == (s % q).astype(np.uint64)).all()


def test_new_entry_points_refuse_a_null_context():
    """No device needed: the checks come before any launch."""
    import ctypes

    from fhecore import _capi

    lib = _capi.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhe_keygen_secret_sparse(None, p, 28, 1, None) == -1
    assert lib.fhe_conj_split_level(None, p, p, p, p, 1, 1, None) == -1
    assert lib.fhe_conj_merge_level(None, p, p, p, 1, 1, None) == -1
