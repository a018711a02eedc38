"""GPU parity for the device CKKS encoder / decoder (fhe_encode / fhe_decode; include/fhecore.h)
against tests/encode_ref.py, bit for bit: 60- and 62-bit chains (the last takes the unfused lift),
a 60-bit q_0 over 50-bit primes, a second N, the two-pass FFT's smallest N, both workgroup
placements, every level and row set, the rounding ties, coefficients just below 2^61, both
centrings of the decoder and the sticky bit of its 128-bit -> double conversion, the refusals,
graph capture, and the two consumers: encryption under device keys and encode_diagonals feeding
linear_transform."""
import ctypes

import numpy as np
import pytest

import coracle
import encode_ref

pytestmark = pytest.mark.gpu

D50 = 2.0 ** 50
D60 = 2.0 ** 60


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


_CTX = {}
_REF = {}


def ctx_for(fc, log_n, L, K, dnum, bits):
    """bits = "mixed": a 60-bit q_0 over 50-bit primes."""
    key = (log_n, L, K, dnum, bits)
    if key not in _CTX:
        if bits == "mixed":
            m = fc.gen_moduli(log_n, 1, bits=60) + fc.gen_moduli(log_n, L - 1 + K, bits=50)
        else:
            m = fc.gen_moduli(log_n, L + K, bits=bits)
        _CTX[key] = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    return _CTX[key]


def bits64(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def slots_to_host(t):
    return t.detach().cpu().numpy()


def from_coeffs(m, log_n):
    """Slots whose encoding at scale delta is (close to) delta m: the host decoder of m."""
    from fhecore import ckks

    return ckks.Encoder(1 << log_n).decode(m, 1.0)


def slot_inputs(log_n):
    """(z50 [8][n], z60 [3][n]): at delta = 2^50 three uniform vectors in the unit square, the
    rounding ties (constant (2k + 1) / 2^51, k even, and its negation with k odd), all zeros, a
    vector whose coefficients are all negative, one more uniform; at delta = 2^60 vectors whose
    coefficients sit just below 2^61 in magnitude (|m| in [1.9, 1.98])."""
    n = 1 << (log_n - 1)
    rng = np.random.default_rng(100 + log_n)
    uni = lambda: rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)  # noqa: E731
    z50 = np.stack([uni(), uni(), uni(),
                    np.full(n, (2 * 6 + 1) / 2.0 ** 51, dtype=np.complex128),
                    np.full(n, -(2 * 7 + 1) / 2.0 ** 51, dtype=np.complex128),
                    np.zeros(n, dtype=np.complex128),
                    from_coeffs(-(0.5 + rng.uniform(0, 1, 2 * n)) * 2.0 ** -10, log_n),
                    uni()])
    big = lambda: rng.choice([-1.0, 1.0], 2 * n) * rng.uniform(1.9, 1.98, 2 * n)  # noqa: E731
    z60 = np.stack([from_coeffs(big(), log_n) for _ in range(3)])
    return z50, z60


def reference(ctx, log_n, bits):
    """The inputs and their reference encodings over all L + K limbs, once per context."""
    key = (log_n, ctx.L, ctx.K, bits)
    if key not in _REF:
        z50, z60 = slot_inputs(log_n)
        allm = ctx.all_moduli
        c50 = encode_ref.encode_coeffs(z50, D50, log_n)
        c60 = encode_ref.encode_coeffs(z60, D60, log_n)
        assert c50[3, 0] == 6 and c50[4, 0] == -8 and not c50[3, 1:].any()  # ties to even
        assert not c50[5].any() and (c50[6] < 0).all()
        assert (np.abs(c60) > 1.8 * 2.0 ** 60).all() and (np.abs(c60) < 2.0 ** 61).all()
        enc = lambda c: coracle.ntt_fwd(encode_ref.residues(c, allm), allm).astype(np.uint64)  # noqa: E731
        _REF[key] = (z50, c50, enc(c50), z60, c60, enc(c60))
    return _REF[key]


CONTEXTS = [(10, 5, 2, 3, 60), (10, 5, 2, 3, 62), (10, 5, 2, 3, "mixed"), (11, 4, 2, 2, 60)]


@pytest.mark.parametrize("log_n,L,K,dnum,bits", CONTEXTS)
def test_encode_matches_the_reference(fc, log_n, L, K, dnum, bits):
    """Counts 1, 3 (rows fastest) and 8 (the XCD placement), levels 1, 2 and L, with and without
    the P rows, at delta = 2^50; coefficients just below 2^61 at delta = 2^60."""
    import torch

    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    n = 1 << log_n
    z50, _, w50, z60, _, w60 = reference(ctx, log_n, bits)
    for z, want, delta, counts in ((z50, w50, D50, (1, 3, 8)), (z60, w60, D60, (3,))):
        for count in counts:
            zd = torch.from_numpy(np.ascontiguousarray(z[:count])).to("cuda")
            for level in (1, 2, L):
                for special in (False, True):
                    rows = encode_ref.rows_limbs(level, special, L, K)
                    got = fc.to_host(ctx.encode(zd, delta, level=level, special=special))
                    assert got.shape == (count, len(rows), n)
                    assert (got == want[:count, rows]).all(), (count, level, special, delta)
            assert (bits64(slots_to_host(zd)) == bits64(z[:count])).all()  # read only
    # a host array is moved first; no batch axis; level defaults to L; a caller's out
    assert (fc.to_host(ctx.encode(z50[1], D50)) == w50[1, :L]).all()
    out = ctx.empty(2, L + K, n)
    assert ctx.encode(z50[:2], D50, special=True, out=out).data_ptr() == out.data_ptr()
    assert (fc.to_host(out) == w50[:2]).all()


def test_encode_two_pass_fft(fc):
    """N = 2^13 is the smallest ring whose N/2 points exceed one workgroup's tile: the strided
    pass over the workspace, then the contiguous one.  Count 1, level 2."""
    log_n = 13
    ctx = ctx_for(fc, log_n, 2, 1, 1, 60)
    z50, c50, w50, _, _, _ = reference(ctx, log_n, 60)
    got = fc.to_host(ctx.encode(z50[:1], D50, level=2))
    assert (got == w50[:1, :2]).all()
    back = slots_to_host(ctx.decode(fc.to_device(w50[:1, :2]), D50))
    want = encode_ref.decode_coeffs(c50[:1].astype(np.float64), D50, log_n)
    assert (bits64(back) == bits64(want)).all()


def test_unfused_switch_gives_the_same_bits(fc, monkeypatch):
    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    z50, _, w50, _, _, _ = reference(ctx, log_n, 60)
    monkeypatch.setenv("FHECORE_ENCODE_UNFUSED", "1")
    assert (fc.to_host(ctx.encode(z50[:3], D50, special=True)) == w50[:3]).all()
    assert (fc.to_host(ctx.encode(z50[:1], D50, level=2)) == w50[:1, :2]).all()


def test_equals_the_composition_of_public_calls(fc):
    """special=False at level L equals ctx.ntt(to_device(to_rns(reference coefficients)))."""
    from fhecore import ckks

    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    z50, c50, _, _, _, _ = reference(ctx, log_n, 60)
    for i in (0, 6):
        want = ctx.ntt(fc.to_device(ckks.to_rns(c50[i], ctx.moduli)))
        got = ctx.encode(z50[i], D50, special=False)
        assert got.shape == want.shape and (got == want).all()


def decode_inputs(qs, log_n, seed):
    """Coefficient-form limbs 0 and 1, [3][2][N].  Polynomial 0: x_0 and x_1 cycle through
    0, 1, h, h + 1, q - 1 of their own modulus with periods 5 and 25 (both sides of the level-1
    centring, and of the two-limb one through t).  Polynomial 1: values that need the sticky bit,
    2^53 + 1, 2^64 +- 1, 2^100 + 2^47 + 1 and their negatives, then uniform values below 2^110 in
    magnitude, built through the CRT.  Polynomial 2: uniform limbs."""
    n = 1 << log_n
    q0, q1 = int(qs[0]), int(qs[1])
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    v0 = np.array([0, 1, (q0 - 1) // 2, (q0 - 1) // 2 + 1, q0 - 1], dtype=np.uint64)
    v1 = np.array([0, 1, (q1 - 1) // 2, (q1 - 1) // 2 + 1, q1 - 1], dtype=np.uint64)
    p0 = np.stack([v0[i % 5], v1[(i // 5) % 5]])
    sticky = [2 ** 53 + 1, 2 ** 64 + 1, 2 ** 64 - 1, 2 ** 100 + 2 ** 47 + 1, 2 ** 100 + 2 ** 47,
              2 ** 100 + 2 ** 47 - 1, 3 * 2 ** 52 + 1, 2 ** 105 + 3 * 2 ** 52]
    vals = [v for s in sticky for v in (s, -s)]
    vals += [int(rng.integers(-2 ** 55, 2 ** 55)) * int(rng.integers(0, 2 ** 55))
             for _ in range(n - len(vals))]
    p1 = np.stack([np.array([v % q for v in vals], dtype=np.uint64) for q in (q0, q1)])
    p2 = np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in (q0, q1)])
    return np.stack([p0, p1, p2])


@pytest.mark.parametrize("log_n,L,K,dnum,bits", [(10, 5, 2, 3, 60), (10, 5, 2, 3, "mixed"),
                                                 (10, 5, 2, 3, 62)])
def test_decode_matches_the_reference(fc, log_n, L, K, dnum, bits):
    """Levels 1, 2 and L with pt_rows = level and = L + K; the limbs from 2 on are poisoned and
    must not be read."""
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    n = 1 << log_n
    x = decode_inputs(qs, log_n, seed=7)
    limbs = coracle.ntt_fwd(x, qs[:2]).astype(np.uint64)  # [3][2][N]
    delta = 1.2345e15
    for level in (1, 2, L):
        want = encode_ref.decode(limbs, delta, log_n, qs, level)
        for rows in (level, L + K):
            pt = np.full((3, rows, n), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            pt[:, :min(rows, 2)] = limbs[:, :min(rows, 2)]
            ptd = fc.to_device(pt)
            got = slots_to_host(ctx.decode(ptd, delta, level=level))
            assert got.shape == (3, n // 2)
            assert (bits64(got) == bits64(want)).all(), (level, rows)
            assert (fc.to_host(ptd) == pt).all()
    # count 1 and 8, no batch axis, a caller's out
    import torch
    pt8 = fc.to_device(np.concatenate([limbs, limbs, limbs[:2]]))
    want = encode_ref.decode(limbs, delta, log_n, qs, 2)
    got8 = slots_to_host(ctx.decode(pt8, delta))
    assert (bits64(got8) == bits64(np.concatenate([want, want, want[:2]]))).all()
    out = torch.empty(n // 2, dtype=torch.complex128, device=pt8.device)
    assert ctx.decode(pt8[1], delta, out=out).data_ptr() == out.data_ptr()
    assert (bits64(slots_to_host(out)) == bits64(want[1])).all()


def test_errors_write_nothing(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    n = 1 << log_n
    lib = fc.load()
    z50, _, w50, _, _, _ = reference(ctx, log_n, 60)
    z = torch.from_numpy(z50[:2].copy()).to("cuda")
    pt = fc.to_device(w50[:2])
    poison = 0x5A5A5A5A5A5A5A5
    out = torch.full((2, L + K, n), poison, dtype=torch.int64, device=z.device)
    zout = torch.full((2, n), poison, dtype=torch.int64, device=z.device)
    assert lib.fhe_encode_workspace(ctx.handle, 2) == 2 * 2 * n * 8
    assert lib.fhe_decode_workspace(ctx.handle, 2) == 3 * 2 * n * 8
    ws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, 2))

    def enc(o, i, delta=D50, level=L, special=1, count=2, c=ctx.handle, w=ws):
        return lib.fhe_encode(c, o, i, delta, level, special, count, _ptr(w), None)

    def dec(o, i, delta=D50, rows=L + K, level=L, count=2, c=ctx.handle, w=ws):
        return lib.fhe_decode(c, o, i, delta, rows, level, count, _ptr(w), None)

    for level in (0, L + 1):
        assert enc(_ptr(out), _ptr(z), level=level) == -1 and b"level" in lib.fhe_last_error()
        assert dec(_ptr(zout), _ptr(pt), level=level) == -1 and b"level" in lib.fhe_last_error()
        with pytest.raises(fc.FheError, match="level"):
            ctx.encode(z, D50, level=level, out=out.view(-1)[:2 * level * n].view(2, level, n))
    for bad in (0.0, -D50, float("inf"), float("nan")):
        assert enc(_ptr(out), _ptr(z), delta=bad) == -1 and b"delta" in lib.fhe_last_error()
        assert dec(_ptr(zout), _ptr(pt), delta=bad) == -1 and b"delta" in lib.fhe_last_error()
    assert enc(None, _ptr(z)) == -1 and b"null" in lib.fhe_last_error()
    assert enc(_ptr(out), None) == -1
    assert dec(None, _ptr(pt)) == -1 and b"null" in lib.fhe_last_error()
    assert dec(_ptr(zout), None) == -1
    assert enc(_ptr(out), _ptr(z), c=None) == -1 and dec(_ptr(zout), _ptr(pt), c=None) == -1
    # pt_rows below the limbs read
    assert dec(_ptr(zout), _ptr(pt), rows=1, level=2) == -1 and b"pt_rows" in lib.fhe_last_error()
    assert dec(_ptr(zout), _ptr(pt), rows=0, level=1) == -1
    # special on a context without P-limbs
    ctx0 = fc.Context(log_n, L=2, K=0)
    with pytest.raises(fc.FheError, match="special"):
        ctx0.encode(z, D50, special=True, out=out.view(-1)[:2 * 2 * n].view(2, 2, n))
    # overlaps: out over slots (encode), slots over pt (decode), either way round
    both = torch.full((2 * (L + K) * n + 2 * n,), poison, dtype=torch.int64, device=z.device)
    zin = both[2 * (L + K) * n - n:][:2 * n]  # starts inside out's span
    assert enc(_ptr(both), _ptr(zin)) == -1 and b"overlaps" in lib.fhe_last_error()
    assert dec(_ptr(zin), _ptr(both)) == -1 and b"overlaps" in lib.fhe_last_error()
    assert enc(_ptr(both[n:]), _ptr(both[:2 * n])) == -1
    assert dec(_ptr(both[:2 * n]), _ptr(both[n:])) == -1
    # count 0 is a no-op
    assert enc(_ptr(out), _ptr(z), count=0) == 0 and dec(_ptr(zout), _ptr(pt), count=0) == 0
    torch.cuda.synchronize()
    assert (out == poison).all() and (zout == poison).all() and (both == poison).all()
    assert (bits64(slots_to_host(z)) == bits64(z50[:2])).all()
    assert (fc.to_host(pt) == w50[:2]).all()


def test_graph_replay(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum = 11, 4, 2, 2
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    n = 1 << log_n
    lib = fc.load()
    z50, c50, w50, _, _, _ = reference(ctx, log_n, 60)
    back = encode_ref.decode_coeffs(c50.astype(np.float64), D50, log_n)
    z = torch.from_numpy(z50[:2].copy()).to("cuda")
    ews = ctx.workspace(lib.fhe_encode_workspace(ctx.handle, 2))
    dws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, 2))
    pt = torch.zeros(2, L + K, n, dtype=torch.int64, device=z.device)
    z2 = torch.zeros(2, n // 2, dtype=torch.complex128, device=z.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.encode(z, D50, special=True, workspace=ews, out=pt)
            ctx.decode(pt, D50, level=L, workspace=dws, out=z2)
        g.launch()
        stream.synchronize()
        assert (fc.to_host(pt) == w50[:2]).all()
        assert (bits64(slots_to_host(z2)) == bits64(back[:2])).all()
        z.copy_(torch.from_numpy(z50[6:8].copy()))  # the captured pointers, new input
        pt.zero_()
        z2.zero_()
        g.launch()
        stream.synchronize()
        assert (fc.to_host(pt) == w50[6:8]).all()
        assert (bits64(slots_to_host(z2)) == bits64(back[6:8])).all()
    # the internal workspace is refused while capturing, and the capture still ends cleanly
    rcs = []
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(sp) == 0
        rcs.append(lib.fhe_encode(ctx.handle, _ptr(pt), _ptr(z), D50, L, 1, 2, None, sp))
        err = lib.fhe_last_error().decode()
        rcs.append(lib.fhe_decode(ctx.handle, _ptr(z2), _ptr(pt), D50, L + K, L, 2, None, sp))
        err += lib.fhe_last_error().decode()
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(sp, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    assert rcs == [-1, -1] and err.count("capturing") == 2
    stream.synchronize()
    assert (fc.to_host(pt) == w50[6:8]).all()  # nothing was launched


def test_encrypt_round_trip_under_device_keys(fc):
    """decode(decrypt(encrypt_sk(encode(z)))) against the same chain through the host Encoder
    (the same secret and encryption seed): both are dominated by the encryption noise."""
    from fhecore import ckks

    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    qs, n = ctx.moduli, ctx.n
    z = reference(ctx, log_n, 60)[0][0]
    sk = ctx.keygen_secret(seed=5)
    dev = ctx.decode(ctx.decrypt(ctx.encrypt_sk(ctx.encode(z, D50), sk, seed=13), sk), D50)
    e_dev = np.abs(slots_to_host(dev) - z).max()
    enc = ckks.Encoder(n)
    pt = ctx.ntt(fc.to_device(ckks.to_rns(enc.encode(z, D50), qs)))
    dec = coracle.ntt_inv(fc.to_host(ctx.decrypt(ctx.encrypt_sk(pt, sk, seed=13), sk)), qs)
    e_host = np.abs(enc.decode(ckks.from_rns(dec, qs), D50) - z).max()
    print(f"encrypt round trip: device encoder {e_dev:.3e}, host encoder {e_host:.3e}")
    assert e_dev <= 2 * e_host


def test_encode_diagonals_feed_linear_transform(fc):
    """A random 16-diagonal matrix, n1 = n2 = 4, real rotation keys, at level L and at level 3
    with the same keys and diagonals: the transform decrypts and decodes to A z, with at most
    twice the error of the same transform fed with host-encoded diagonals.  A z here is
    sum_k d_k * np.roll(z, -k): galois_elt(step) moves slot j + step into slot j."""
    from fhecore import ckks

    log_n, L, K, dnum = 10, 5, 2, 3
    n1 = n2 = 4
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    n, ns, allm = ctx.n, ctx.n // 2, ctx.all_moduli
    rng = np.random.default_rng(77)
    z = rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns)
    diags = {k: rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns) for k in range(n1 * n2)}
    want = sum(d * np.roll(z, -k) for k, d in diags.items())
    sk = ctx.keygen_secret(seed=21)
    baby, giant, pts = ctx.encode_diagonals(diags, n1, n2, D50)
    assert baby == [ctx.galois_elt(b) for b in range(n1)]
    assert giant == [ctx.galois_elt(g * n1) for g in range(n2)]
    keys = lambda elts, s0: [None if e == 1 else ctx.keygen_rotation(sk, e, seed=s0 + i)  # noqa: E731
                             for i, e in enumerate(elts)]
    bk, gk = keys(baby, 30), keys(giant, 40)
    enc = ckks.Encoder(n)
    host_pts = [[fc.to_device(coracle.ntt_fwd(
        ckks.to_rns(enc.encode(np.roll(diags[g * n1 + b], g * n1), D50), allm), allm))
        for b in range(n1)] for g in range(n2)]
    top = ctx.encrypt_sk(ctx.encode(z, D50), sk, seed=50)
    # the rotation direction on its own: one rotation by 1 decrypts to np.roll(z, -1)
    r1 = ctx.decode(ctx.decrypt(ctx.rotate(top, baby[1], *bk[1]), sk), D50)
    assert np.abs(slots_to_host(r1) - np.roll(z, -1)).max() < 1e-6
    for level in (L, 3):
        ct = top if level == L else ctx.drop_level(top, level)
        errs = []
        for p in (pts, host_pts):
            out = ctx.linear_transform(ct, baby, bk, giant, gk, p)
            got = slots_to_host(ctx.decode(ctx.decrypt(out, sk), D50 * D50))
            errs.append(np.abs(got - want).max())
        print(f"level {level}: |A z - decode| device diagonals {errs[0]:.3e}, host diagonals "
              f"{errs[1]:.3e}")
        assert errs[1] < 1e-3  # the transform itself is right (noise over delta^2 is far below)
        assert errs[0] <= 2 * errs[1]
