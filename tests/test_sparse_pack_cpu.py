"""Sparse packing without a GPU: the five facts the device path and the sparse bootstrap rest on
(tests/sparse_pack_ref.py against tests/encode_ref.py at N = 2^10), the host Encoder's sparse form,
the new entry points' device-free refusals, and fhecore.bootstrap.Bootstrapper(log_slots=6) on the
CPU backend."""
import ctypes

import numpy as np
import pytest

import bootstrap_ref as br
import cases
import encode_ref
import sparse_pack_ref as sp

LOG_N = 10
N = 1 << LOG_N
D50 = 2.0 ** 50
LOG_SLOTS = [0, 1, 3, 6, 9]


def bits64(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def slots(ls, seed, count=3):
    g = np.random.default_rng(seed + ls)
    return g.uniform(-1, 1, (count, 1 << ls)) + 1j * g.uniform(-1, 1, (count, 1 << ls))


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_fact1_encode_is_the_small_transform_on_the_grid(ls):
    gap, ns = sp.gap(LOG_N, ls), 1 << ls
    z = slots(ls, 1)
    small = encode_ref.encode_coeffs(z, D50, ls + 1)
    placed = np.zeros((z.shape[0], N), dtype=np.int64)
    placed[:, ::gap] = small
    assert (placed == sp.encode_coeffs(z, D50, LOG_N, ls)).all()
    assert placed[:, ::gap].any() and small.shape[-1] == 2 * ns


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_fact2_decode_of_grid_coefficients(ls):
    gap = sp.gap(LOG_N, ls)
    g = np.random.default_rng(20 + ls)
    c = np.zeros((2, N))
    c[:, ::gap] = g.integers(-2 ** 52, 2 ** 52, (2, N // gap)).astype(np.float64)
    small = encode_ref.decode_coeffs(c[:, ::gap], D50, ls + 1)
    full = encode_ref.decode_coeffs(c, D50, LOG_N)
    assert (bits64(np.tile(small, gap)) == bits64(full)).all()
    # the reference's decode reads the grid only: noise off it changes nothing
    qs = [int(q) for q in br.moduli()[0][:2]]
    noisy = c.copy()
    noisy[:, 1::2] += g.integers(-2 ** 30, 2 ** 30, (2, N // 2))
    pts = [encode_ref.coracle.ntt_fwd(encode_ref.residues(x.astype(np.int64), qs), qs)
           for x in (c, noisy)]
    a, b = (sp.decode(p, D50, LOG_N, ls, qs, 2) for p in pts)
    if gap > 1:
        assert (bits64(a) == bits64(b)).all()
    assert (bits64(a) == bits64(small)).all()


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_fact3_tables_are_slices(ls):
    gap, ns = sp.gap(LOG_N, ls), 1 << ls
    (c, s), (cs, ss) = encode_ref.roots(LOG_N), encode_ref.roots(ls + 1)
    assert (bits64(c[::gap]) == bits64(cs)).all() and (bits64(s[::gap]) == bits64(ss)).all()
    assert all(pow(5, j, 2 * N) % (4 * ns) == pow(5, j, 4 * ns) for j in range(ns))
    from fhecore import bootstrap as bs

    w, rot = bs._tables(LOG_N, ls)
    assert (bits64(w.real) == bits64(cs)).all() and (bits64(w.imag) == bits64(ss)).all()
    assert (rot == [pow(5, j, 4 * ns) for j in range(ns)]).all()


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_fact4_subsum_is_the_trace(ls):
    gap = sp.gap(LOG_N, ls)
    g = np.random.default_rng(40 + ls)
    t = g.integers(-2 ** 40, 2 ** 40, (2, N))
    want = np.zeros_like(t)
    want[:, ::gap] = gap * t[:, ::gap]
    assert (sp.subsum(t, ls) == want).all()
    # the automorphism is the slot rotation: sigma_{5^r} of an encoding decodes rolled by -r
    z = slots(LOG_N - 1, 4, 1)
    c = encode_ref.encode_coeffs(z, D50, LOG_N)
    import pyoracle

    r = encode_ref.decode_coeffs(sp.automorphism(c, pyoracle.galois_elt(3, N)).astype(np.float64),
                                 D50, LOG_N)
    assert np.abs(r - np.roll(z, -3)).max() < 1e-9


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_fact5_small_factors_act_on_periodic_vectors(ls):
    from fhecore import bootstrap as bs

    if ls == 0:  # one slot: no stage, no factor
        assert bs.stage_lengths(LOG_N, True, 0) == []
        with pytest.raises(ValueError, match="groups"):
            bs.dft_factors(LOG_N, 1, True, 0)
        return
    gap, ns = sp.gap(LOG_N, ls), 1 << ls
    rev = encode_ref._tables(ls + 1)[2]
    g = np.random.default_rng(50 + ls)
    t = g.integers(-2 ** 40, 2 ** 40, 2 * ns).astype(np.float64)
    c = np.zeros(N)
    c[::gap] = t
    v = encode_ref.decode_coeffs(c, 1.0, LOG_N)  # the full ring's slots: n_s-periodic
    assert (bits64(v) == bits64(np.tile(v[:ns], gap))).all()
    want = np.tile((t[:ns] + 1j * t[ns:])[rev], gap)
    for groups in sorted({1, min(ls, 3)}):
        inv = bs.dft_factors(LOG_N, groups, True, ls)
        fwd = bs.dft_factors(LOG_N, groups, False, ls)
        assert len(inv) == groups and all(len(d) == ns for f in inv for d in f.values())
        tile = lambda fs: [{k: np.tile(d, gap) for k, d in f.items()} for f in fs]  # noqa: E731
        got = br.apply_factors(tile(inv), v) / ns
        assert np.abs(got - want).max() <= 3e-12 * np.abs(want).max()
        back = br.apply_factors(tile(fwd), got * ns)
        assert np.abs(back - ns * v).max() <= 3e-12 * ns * np.abs(v).max()
        # the layouts place every diagonal, and the steps stay inside (-n_s, n_s)
        for fs, inverse in ((inv, True), (fwd, False)):
            for f, (n1, n2, stride, offset) in zip(fs, bs.factor_layouts(LOG_N, groups, inverse, ls)):
                z, baby, giant = bs.place_strided_diagonals(f, ns, n1, n2, stride, offset)
                assert z.shape == (n2, n1, ns) and max(map(abs, baby + giant)) < ns
    if ls == LOG_N - 1:  # full packing: the existing calls' results
        for inverse in (True, False):
            a, b = bs.dft_factors(LOG_N, 3, inverse), bs.dft_factors(LOG_N, 3, inverse, ls)
            assert all(x.keys() == y.keys() and all((bits64(x[k]) == bits64(y[k])).all() for k in x)
                       for x, y in zip(a, b))
            assert bs.factor_layouts(LOG_N, 3, inverse) == bs.factor_layouts(LOG_N, 3, inverse, ls)


@pytest.mark.parametrize("ls", LOG_SLOTS)
def test_host_encoder_is_within_a_unit_of_the_reference(ls):
    from fhecore import ckks

    enc = ckks.Encoder(N, slots=1 << ls)
    z = slots(ls, 6, 2)
    for row in z:
        c = enc.encode(row, D50)
        want = sp.encode_coeffs(row, D50, LOG_N, ls)
        assert np.abs(c - want).max() <= 1
        noisy = want.astype(np.float64)
        if ls < LOG_N - 1:
            noisy[1::2] += 12345.0  # off the grid: not read
        back = enc.decode(noisy, D50)
        assert back.shape == (1 << ls,) and np.abs(back - row).max() < 1e-9
    with pytest.raises(ValueError, match="slots"):
        ckks.Encoder(N, slots=3)
    with pytest.raises(ValueError, match="slots"):
        ckks.Encoder(N, slots=N)
    full = ckks.Encoder(N)
    zf = slots(LOG_N - 1, 7, 1)[0]
    assert (full.encode(zf, D50) == ckks.Encoder(N, slots=N // 2).encode(zf, D50)).all()


def test_new_entry_points_refuse_without_a_device():
    """delta is checked before the context, so both refusals need no device."""
    from fhecore import _capi

    lib = _capi.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert lib.fhe_encode_sparse(None, p, p, bad, 3, 1, 0, 1, None, None) == -1
        assert b"fhe_encode_sparse: delta" in lib.fhe_last_error()
        assert lib.fhe_decode_sparse(None, p, p, bad, 3, 1, 1, 1, None, None) == -1
        assert b"fhe_decode_sparse: delta" in lib.fhe_last_error()
    assert lib.fhe_encode_sparse(None, p, p, D50, 3, 1, 0, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_decode_sparse(None, p, p, D50, 3, 1, 1, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()


def test_sparse_bootstrap_decrypts_to_the_input_slots():
    """Maximum slot error of this run: 2.442e-05 (deterministic under the fixed seeds; the margin
    covers float differences between numpy builds only), at or below full packing's 2.833e-05 as
    expected at the same message ratio, and far from the 2 x 2.833e-05 that would mean a wrong
    constant in the composition.  Nearly all of it is EvalMod's cubic term of these 64 slots,
    which the exact sine on the bare coefficients gives as 2.47e-05."""
    out, err = cases.run_cpu(cases.SPARSE)
    print(f"sparse bootstrap: level {out.level}, scale / input scale "
          f"{float(out.scale) / sp.IN_SCALE:.12f}, max slot error {err:.4e}")
    assert cases.SPARSE_BOOTSTRAP_ERR <= cases.BOOTSTRAP_ERR
    assert err < cases.MARGIN * cases.SPARSE_BOOTSTRAP_ERR
    assert out.level == br.OUT_LEVEL and np.asarray(out.data).shape == (2, br.OUT_LEVEL, N)
    assert abs(float(out.scale) / sp.IN_SCALE - 1) < 2.0 ** -26
    su = cases.setup(cases.SPARSE)
    cubic = sp.cubic_term(su["z"], sp.IN_SCALE, su["qs"][0], sp.LOG_SLOTS)
    print(f"cubic term alone: {cubic:.4e}")
    assert abs(err - cubic) < 0.05 * cubic


def test_the_cubic_term_follows_the_message_ratio_not_the_packing():
    """Why the case is encoded at delta / sqrt(gap) (sparse_pack_ref.IN_SCALE): at one scale a
    plaintext of n_s slots has coefficients sqrt(gap) larger, and the exact sine on the bare
    coefficients -- no ciphertext, no bootstrap -- leaves about gap times the slot error.  At the
    same coefficient size the term is full packing's."""
    su, full = cases.setup(cases.SPARSE), cases.setup(cases.BOOTSTRAP)
    q0 = su["qs"][0]
    at_delta = sp.cubic_term(su["z"], br.DELTA, q0, sp.LOG_SLOTS)
    at_ratio = sp.cubic_term(su["z"], sp.IN_SCALE, q0, sp.LOG_SLOTS)
    full_packing = sp.cubic_term(full["z"], br.DELTA, q0, br.LOG_N - 1)
    print(f"cubic term: 64 slots at delta {at_delta:.3e}, at delta / sqrt(gap) {at_ratio:.3e}; "
          f"512 slots at delta {full_packing:.3e}")
    gap = sp.gap(br.LOG_N, sp.LOG_SLOTS)
    # (sqrt(gap))^3 per coefficient, 1 / sqrt(gap) for the scale; the sine's next term,
    # (2 pi m / q_0)^2 / 20 of the cubic one, is below 1e-3 for |m| / q_0 < 0.02
    assert abs(at_delta / at_ratio - gap) < 1e-3 * gap
    assert 0.5 * full_packing < at_ratio < 1.5 * full_packing
    rms = lambda z, s, ls: np.sqrt(np.mean(  # noqa: E731
        encode_ref.encode_coeffs(z, s, ls + 1).astype(np.float64) ** 2))
    same = rms(su["z"], sp.IN_SCALE, sp.LOG_SLOTS) / rms(full["z"], br.DELTA, br.LOG_N - 1)
    assert 0.85 < same < 1.15  # the message ratio of bootstrap_ref's case


def test_sparse_bootstrapper_constants_and_refusals():
    from fhecore import bootstrap as bs

    boot = bs.Bootstrapper(cases.backend(cases.SPARSE), **sp.PARAMS)
    full = bs.Bootstrapper(cases.backend(cases.BOOTSTRAP), **br.PARAMS)
    assert boot.subsum_steps == [64, 128, 256] and full.subsum_steps == []
    # 2 n_s gap = N: the constants and scales are full packing's, to the digit
    assert boot.scale_cts == full.scale_cts and boot.mult_stc == full.mult_stc
    assert boot.out_level == br.OUT_LEVEL
    be = cases.backend(cases.SPARSE)
    for bad in (2, -1, LOG_N):
        with pytest.raises(ValueError, match="log_slots"):
            bs.Bootstrapper(be, **dict(sp.PARAMS, log_slots=bad))
    with pytest.raises(ValueError, match="more groups"):
        bs.Bootstrapper(cases.backend(cases.BOOTSTRAP),
                        **dict(br.PARAMS, cts_groups=1, log_slots=LOG_N - 1))
    assert bs.BootstrapParams().log_slots is None


def test_full_packing_bootstrap_is_unchanged():
    """log_slots = log_n - 1 is the full-packing path: the bits of the BOOTSTRAP case's CPU run,
    which runs Bootstrapper with the default None."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    ref, err = cases.run_cpu(cases.BOOTSTRAP)
    assert err < cases.MARGIN * cases.BOOTSTRAP_ERR
    su = cases.setup(cases.BOOTSTRAP)
    boot = bs.Bootstrapper(cases.backend(cases.BOOTSTRAP), **dict(br.PARAMS, log_slots=LOG_N - 1))
    out = boot.bootstrap(Ct(np.asarray(su["ct"])[:, :1], 1, br.DELTA))
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (np.asarray(out.data) == np.asarray(ref.data)).all()
