"""GPU parity for sparse packing (fhe_encode_sparse / fhe_decode_sparse; include/fhecore.h) against
tests/sparse_pack_ref.py, bit for bit: every slot count that takes another path at N = 2^10 (one
slot, packed tiles with short last groups, full packing), both lift placements, the unfused lift,
a mixed chain's two centrings, the rounding ties, one full tile and the two-pass form, plaintexts
with noise off the grid, the refusals and graph capture; then the consumers: a rotation of an
encrypted sparse plaintext and the sparse bootstrap on the GPU backend."""
import ctypes

import numpy as np
import pytest

import bootstrap_ref as br
import cases
import coracle
import encode_ref
import sparse_pack_ref as sp

pytestmark = pytest.mark.gpu

D50 = 2.0 ** 50
COUNT = 9


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


def host(t):
    return t.detach().cpu().numpy()


def slot_inputs(log_n, ls, count=COUNT):
    """[count][n_s]: uniform vectors in the unit square; rows 3 and 4 are the rounding ties of
    test_gpu_encode.py (constant (2k + 1) / 2^51, k even, and its negation with k odd), row 5 zeros."""
    ns = 1 << ls
    rng = np.random.default_rng(1000 * log_n + ls)
    z = rng.uniform(-1, 1, (count, ns)) + 1j * rng.uniform(-1, 1, (count, ns))
    if count > 5:
        z[3] = (2 * 6 + 1) / 2.0 ** 51
        z[4] = -(2 * 7 + 1) / 2.0 ** 51
        z[5] = 0
    return z


def reference(ctx, log_n, ls, bits, count=COUNT):
    """(z, coefficients, encodings over all L + K limbs), once per context and slot count."""
    key = (log_n, ctx.L, ctx.K, bits, ls, count)
    if key not in _REF:
        z = slot_inputs(log_n, ls, count)
        c = sp.encode_coeffs(z, D50, log_n, ls)
        allm = ctx.all_moduli
        _REF[key] = (z, c, coracle.ntt_fwd(encode_ref.residues(c, allm), allm).astype(np.uint64))
    return _REF[key]


def check_encode(fc, ctx, log_n, ls, bits, counts, levels):
    import torch

    L, K, n = ctx.L, ctx.K, 1 << log_n
    z, _, want = reference(ctx, log_n, ls, bits)
    for count in counts:
        zd = torch.from_numpy(np.ascontiguousarray(z[:count])).to("cuda")
        for level in levels:
            for special in (False, True):
                rows = encode_ref.rows_limbs(level, special, L, K)
                got = fc.to_host(ctx.encode(zd, D50, level=level, special=special, log_slots=ls))
                assert got.shape == (count, len(rows), n)
                assert (got == want[:count, rows]).all(), (ls, count, level, special)
        assert (bits64(host(zd)) == bits64(z[:count])).all()  # read only


def check_decode(fc, ctx, log_n, ls, counts, levels, seed=7):
    """Uniform limbs: every coefficient off the grid is non-zero and must not be read; the limbs
    from 2 on are poisoned."""
    qs, n = ctx.moduli, 1 << log_n
    rng = np.random.default_rng(seed + ls)
    limbs = np.stack([rng.integers(0, q, (max(counts), n), dtype=np.uint64) for q in qs[:2]], axis=1)
    delta = 1.2345e15
    for level in levels:
        want = sp.decode(limbs, delta, log_n, ls, qs, level)
        for count in counts:
            rows = max(level, 2) + 1
            pt = np.full((count, rows, n), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            pt[:, :min(level, 2)] = limbs[:count, :min(level, 2)]
            got = host(ctx.decode(fc.to_device(pt), delta, level=level, log_slots=ls))
            assert got.shape == (count, 1 << ls)
            assert (bits64(got) == bits64(want[:count])).all(), (ls, level, count)


@pytest.mark.parametrize("ls", [0, 1, 2, 5, 8, 9])
def test_encode_and_decode_match_the_reference(fc, ls):
    """N = 2^10, a 60-bit chain, K = 2.  Counts 1, 3 (rows fastest), 8 (the XCD placement) and 9:
    tiles of up to 8 plaintexts whose last group holds 1, 3 or all of them.  log_slots = 9 is
    full packing and must also equal fhe_encode / fhe_decode."""
    log_n, L = 10, 4
    ctx = ctx_for(fc, log_n, L, 2, 2, 60)
    check_encode(fc, ctx, log_n, ls, 60, (1, 3, 8, 9), (1, L))
    check_decode(fc, ctx, log_n, ls, (1, 3, 9), (1, L))
    z, c, want = reference(ctx, log_n, ls, 60)
    gap = sp.gap(log_n, ls)
    assert gap == 1 or not c.reshape(COUNT, -1, gap)[:, :, 1:].any()
    assert c[3, 0] == 6 and c[4, 0] == -8 and not c[3, 1:].any() and not c[5].any()  # ties to even
    if ls == log_n - 1:
        assert (fc.to_host(ctx.encode(z, D50, special=True)) == want).all()
        pt = fc.to_device(want[:, :L])
        assert (bits64(host(ctx.decode(pt, D50))) == bits64(host(ctx.decode(pt, D50, log_slots=ls)))).all()
    # decode inverts encode: the slots come back (the reference's bits, and close to the input)
    back = host(ctx.decode(fc.to_device(want[:, :L]), D50, log_slots=ls))
    assert (bits64(back) == bits64(sp.decode(want[:, :L], D50, log_n, ls, ctx.moduli, L))).all()
    assert np.abs(back - z).max() < 1e-9


def test_wide_chain_takes_the_unfused_lift(fc):
    log_n, L, ls = 10, 4, 5
    ctx = ctx_for(fc, log_n, L, 2, 2, 62)
    check_encode(fc, ctx, log_n, ls, 62, (3,), (1, L))
    check_decode(fc, ctx, log_n, ls, (3,), (1, 2))


def test_unfused_switch_gives_the_same_bits(fc, monkeypatch):
    log_n, L, ls = 10, 4, 5
    ctx = ctx_for(fc, log_n, L, 2, 2, 60)
    monkeypatch.setenv("FHECORE_ENCODE_UNFUSED", "1")
    check_encode(fc, ctx, log_n, ls, 60, (3,), (L,))


def test_mixed_chain_decodes_at_levels_1_and_2(fc):
    """A 60-bit q_0 over 50-bit primes: both centrings, the ties in the encodings."""
    log_n, L, ls = 10, 4, 5
    ctx = ctx_for(fc, log_n, L, 2, 2, "mixed")
    check_encode(fc, ctx, log_n, ls, "mixed", (9,), (L,))
    check_decode(fc, ctx, log_n, ls, (3,), (1, 2))


def test_one_full_tile_and_full_packing_at_n13(fc):
    """N = 2^13: log_slots = 11 fills one workgroup's tile; log_slots = 12 is fhe_encode."""
    log_n = 13
    ctx = ctx_for(fc, log_n, 2, 1, 1, 60)
    for ls in (11, 12):
        z, _, want = reference(ctx, log_n, ls, 60, 2)
        for count in (1, 2):
            got = fc.to_host(ctx.encode(z[:count], D50, special=True, log_slots=ls))
            assert (got == want[:count]).all(), (ls, count)
        back = host(ctx.decode(fc.to_device(want[:, :2]), D50, log_slots=ls))
        assert (bits64(back) == bits64(sp.decode(want[:, :2], D50, log_n, ls, ctx.moduli, 2))).all()
    assert (fc.to_host(ctx.encode(z, D50, special=True)) == want).all()  # ls = 12: the full call
    check_decode(fc, ctx, log_n, 11, (2,), (2,))


@pytest.mark.parametrize("count", [1, 2])
def test_sparse_two_pass_form(fc, count):
    """N = 2^14, log_slots = 12: the smallest sparse shape whose points exceed a tile -- the strided
    pass with ln != log_n - 1, then the contiguous one."""
    log_n, ls = 14, 12
    ctx = ctx_for(fc, log_n, 2, 1, 1, 60)
    z, _, want = reference(ctx, log_n, ls, 60, 2)
    got = fc.to_host(ctx.encode(z[:count], D50, level=2, log_slots=ls))
    assert (got == want[:count, :2]).all()
    check_decode(fc, ctx, log_n, ls, (count,), (2,))


def test_sliced_rounding_store(fc):
    """N = 2^14, log_slots = 5: one plaintext's 2^14 coefficients exceed what one workgroup
    stores, so two workgroups each redo the 32-point transform and write half the runs."""
    log_n, ls = 14, 5
    ctx = ctx_for(fc, log_n, 2, 1, 1, 60)
    z, _, want = reference(ctx, log_n, ls, 60, 3)
    got = fc.to_host(ctx.encode(z, D50, special=True, log_slots=ls))
    assert (got == want).all()
    check_decode(fc, ctx, log_n, ls, (3,), (2,))


def test_refusals_write_nothing(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, ls = 10, 4, 2, 5
    ctx = ctx_for(fc, log_n, L, K, 2, 60)
    n, ns = 1 << log_n, 1 << ls
    lib = fc.load()
    z0, _, want = reference(ctx, log_n, ls, 60)
    z = torch.from_numpy(z0[:2].copy()).to("cuda")
    pt = fc.to_device(want[:2])
    poison = 0x5A5A5A5A5A5A5A5
    out = torch.full((2, L + K, n), poison, dtype=torch.int64, device=z.device)
    zout = torch.full((2, 2 * ns), poison, dtype=torch.int64, device=z.device)
    ws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, 2))

    def enc(o, i, delta=D50, s=ls, level=L, special=1, count=2, c=ctx.handle):
        return lib.fhe_encode_sparse(c, o, i, delta, s, level, special, count, _ptr(ws), None)

    def dec(o, i, delta=D50, s=ls, rows=L + K, level=L, count=2, c=ctx.handle):
        return lib.fhe_decode_sparse(c, o, i, delta, s, rows, level, count, _ptr(ws), None)

    for bad in (log_n, log_n + 7, 0xFFFFFFFF):
        assert enc(_ptr(out), _ptr(z), s=bad) == -1 and b"log_slots" in lib.fhe_last_error()
        assert dec(_ptr(zout), _ptr(pt), s=bad) == -1 and b"log_slots" in lib.fhe_last_error()
    with pytest.raises(ValueError, match="log_slots"):
        ctx.encode(z, D50, log_slots=log_n)
    with pytest.raises(ValueError, match="log_slots"):
        ctx.decode(pt, D50, log_slots=-1)
    with pytest.raises(ValueError, match="slots"):
        ctx.encode(z, D50, log_slots=ls + 1)  # the last dimension is not 2^log_slots
    for level in (0, L + 1):
        assert enc(_ptr(out), _ptr(z), level=level) == -1 and b"level" in lib.fhe_last_error()
        assert dec(_ptr(zout), _ptr(pt), level=level) == -1 and b"level" in lib.fhe_last_error()
    for bad in (0.0, float("inf"), float("nan")):
        assert enc(_ptr(out), _ptr(z), delta=bad) == -1 and b"delta" in lib.fhe_last_error()
        assert dec(_ptr(zout), _ptr(pt), delta=bad) == -1 and b"delta" in lib.fhe_last_error()
    assert enc(None, _ptr(z)) == -1 and enc(_ptr(out), None) == -1
    assert dec(None, _ptr(pt)) == -1 and dec(_ptr(zout), None) == -1
    assert enc(_ptr(out), _ptr(z), c=None) == -1 and dec(_ptr(zout), _ptr(pt), c=None) == -1
    assert dec(_ptr(zout), _ptr(pt), rows=1, level=2) == -1 and b"pt_rows" in lib.fhe_last_error()
    ctx0 = fc.Context(log_n, L=2, K=0)
    with pytest.raises(fc.FheError, match="special"):
        ctx0.encode(z, D50, special=True, log_slots=ls,
                    out=out.view(-1)[:2 * 2 * n].view(2, 2, n))
    # overlaps, by the sparse extent of the slots: 2 * 2 n_s words
    both = torch.full((2 * (L + K) * n + 4 * ns,), poison, dtype=torch.int64, device=z.device)
    inside = both[2 * (L + K) * n - ns:][:4 * ns]  # starts inside out's span
    assert enc(_ptr(both), _ptr(inside)) == -1 and b"overlaps" in lib.fhe_last_error()
    assert dec(_ptr(inside), _ptr(both)) == -1 and b"overlaps" in lib.fhe_last_error()
    assert enc(_ptr(both[ns:]), _ptr(both[:4 * ns])) == -1
    assert dec(_ptr(both[:4 * ns]), _ptr(both[ns:])) == -1
    assert enc(_ptr(out), _ptr(z), count=0) == 0 and dec(_ptr(zout), _ptr(pt), count=0) == 0
    torch.cuda.synchronize()
    assert (out == poison).all() and (zout == poison).all() and (both == poison).all()
    # slots that end where out begins are no overlap, although N words per plaintext would be
    both[:4 * ns].copy_(torch.view_as_real(z).contiguous().view(torch.int64).reshape(-1))
    assert enc(_ptr(both[4 * ns:]), _ptr(both[:4 * ns])) == 0
    torch.cuda.synchronize()
    assert (fc.to_host(both[4 * ns:].view(2, L + K, n)) == want[:2]).all()
    assert (fc.to_host(pt) == want[:2]).all()


def test_graph_replay(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, ls = 10, 4, 2, 5
    ctx = ctx_for(fc, log_n, L, K, 2, 60)
    n, ns = 1 << log_n, 1 << ls
    lib = fc.load()
    z0, c, want = reference(ctx, log_n, ls, 60)
    back = encode_ref.decode_coeffs(c[:, ::sp.gap(log_n, ls)].astype(np.float64), D50, ls + 1)
    z = torch.from_numpy(z0[:3].copy()).to("cuda")
    ews = ctx.workspace(lib.fhe_encode_workspace(ctx.handle, 3))
    dws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, 3))
    pt = torch.zeros(3, L + K, n, dtype=torch.int64, device=z.device)
    z2 = torch.zeros(3, ns, dtype=torch.complex128, device=z.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.encode(z, D50, special=True, workspace=ews, out=pt, log_slots=ls)
            ctx.decode(pt, D50, level=L, workspace=dws, out=z2, log_slots=ls)
        for lo in (0, 6):  # the captured pointers, new input
            z.copy_(torch.from_numpy(z0[lo:lo + 3].copy()))
            pt.zero_()
            z2.zero_()
            g.launch()
            stream.synchronize()
            assert (fc.to_host(pt) == want[lo:lo + 3]).all()
            assert (bits64(host(z2)) == bits64(back[lo:lo + 3])).all()
    # the internal workspace is refused while capturing, and the capture still ends cleanly
    rcs = []
    with torch.cuda.stream(stream):
        s = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(s) == 0
        rcs.append(lib.fhe_encode_sparse(ctx.handle, _ptr(pt), _ptr(z), D50, ls, L, 1, 3, None, s))
        err = lib.fhe_last_error().decode()
        rcs.append(lib.fhe_decode_sparse(ctx.handle, _ptr(z2), _ptr(pt), D50, ls, L + K, L, 3,
                                         None, s))
        err += lib.fhe_last_error().decode()
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(s, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    assert rcs == [-1, -1] and err.count("capturing") == 2
    stream.synchronize()
    assert (fc.to_host(pt) == want[6:9]).all()  # nothing was launched


# ---- consumers ------------------------------------------------------------------------------------

def test_rotation_of_an_encrypted_sparse_plaintext(fc):
    """encrypt(encode(z, log_slots)) rotated by one step decodes sparsely to np.roll(z, -1): the
    rotation is n_s-cyclic.  The tolerance is that of test_gpu_encode.py's round trip: at most
    twice the error of the same chain (secret, seeds, key) through the host Encoder."""
    from fhecore import ckks

    log_n, L, ls = 10, 4, 5
    ctx = ctx_for(fc, log_n, L, 2, 2, 60)
    qs, n = ctx.moduli, ctx.n
    z = reference(ctx, log_n, ls, 60)[0][0]
    sk = ctx.keygen_secret(seed=5)
    elt = ctx.galois_elt(1)
    key = ctx.keygen_rotation(sk, elt, seed=6)
    ct = ctx.encrypt_sk(ctx.encode(z, D50, log_slots=ls), sk, seed=13)
    dev = ctx.decode(ctx.decrypt(ctx.rotate(ct, elt, *key), sk), D50, log_slots=ls)
    e_dev = np.abs(host(dev) - np.roll(z, -1)).max()
    enc = ckks.Encoder(n, slots=1 << ls)
    pt = ctx.ntt(fc.to_device(ckks.to_rns(enc.encode(z, D50), qs)))
    rot = ctx.rotate(ctx.encrypt_sk(pt, sk, seed=13), elt, *key)
    dec = coracle.ntt_inv(fc.to_host(ctx.decrypt(rot, sk)), qs)
    e_host = np.abs(enc.decode(ckks.from_rns(dec, qs), D50) - np.roll(z, -1)).max()
    print(f"sparse rotation: device encoder {e_dev:.3e}, host encoder {e_host:.3e}")
    assert e_host < 1e-6
    assert e_dev <= 2 * e_host


def test_encode_diagonals_passes_log_slots_through(fc):
    """pts[g][b] is the sparse encoding of d_k rolled by g n1 within its n_s entries; the Galois
    elements are the full ring's."""
    log_n, L, ls, n1, n2 = 10, 4, 5, 4, 2
    ctx = ctx_for(fc, log_n, L, 2, 2, 60)
    ns = 1 << ls
    rng = np.random.default_rng(91)
    diags = {k: rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns) for k in (0, 1, 5, 7)}
    baby, giant, pts = ctx.encode_diagonals(diags, n1, n2, D50, log_slots=ls)
    assert baby == [ctx.galois_elt(b) for b in range(n1)]
    assert giant == [ctx.galois_elt(g * n1) for g in range(n2)]
    for k in range(n1 * n2):
        g, b = divmod(k, n1)
        d = np.roll(diags[k], g * n1) if k in diags else np.zeros(ns, dtype=np.complex128)
        assert (fc.to_host(pts[g][b]) == sp.encode(d, D50, log_n, ls, ctx.all_moduli)).all(), k
    with pytest.raises(ValueError, match="slots"):
        ctx.encode_diagonals(diags, n1, n2, D50)  # 32-entry diagonals are not full-packing ones


@pytest.fixture(scope="module")
def bctx(fc):
    su = cases.setup(cases.SPARSE)
    c = fc.Context(br.LOG_N, moduli=su["qs"], special=su["ps"], dnum=br.DNUM)
    assert c.moduli == su["qs"] and c.special == su["ps"]
    return c


def u64(x):
    return np.asarray(x).astype(np.uint64)


def test_sparse_bootstrap_matches_the_cpu_backend_bit_for_bit(fc, bctx):
    """Both backends receive the same integers and the same float64 diagonals (fhe_encode_sparse
    of [n2, n1, 64] equals the reference's encoding of the tiled vectors), so data, level and
    scale are the same."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    su = cases.setup(cases.SPARSE)
    d = lambda key: (fc.to_device(u64(key[0])), fc.to_device(u64(key[1])))  # noqa: E731
    be = bs.GpuBackend(bctx, relin_key=d(su["relin"]),
                       rot_keys={k: d(v) for k, v in su["rot"].items()})
    boot = bs.Bootstrapper(be, **sp.PARAMS)
    ct = fc.to_device(u64(np.asarray(su["ct"])[:, :1]))
    out = boot.bootstrap(Ct(ct, 1, sp.IN_SCALE))
    ref, err = cases.run_cpu(cases.SPARSE)
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (fc.to_host(out.data) == u64(ref.data)).all()
    assert err < cases.MARGIN * cases.SPARSE_BOOTSTRAP_ERR


def test_sparse_bootstrap_under_device_keys(fc, bctx):
    """A weight-28 secret, every key and the encryption made on the device; the ciphertext dropped
    to level 1 comes back at level 3 and decodes (sparsely) to the 64 input slots within
    2 x SPARSE_BOOTSTRAP_ERR, a second bootstrap within 4 x: the factors of the full-packing
    test, for its reasons."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    su = cases.setup(cases.SPARSE)
    sk = bctx.keygen_secret(seed=61, hamming_weight=br.HAMMING)
    be = bs.GpuBackend(bctx, sk=sk, seed=2000)
    boot = bs.Bootstrapper(be, **sp.PARAMS)
    ct = bctx.encrypt_sk(fc.to_device(su["pt"]), sk, seed=62)
    out = boot.bootstrap(Ct(bctx.drop_level(ct, 1), 1, sp.IN_SCALE))
    assert sorted(be.rot_keys) == sp.rotation_elements()  # SubSum's, every step's, the conjugation's
    assert out.level == boot.out_level == br.OUT_LEVEL
    assert tuple(out.data.shape) == (2, br.OUT_LEVEL, 1 << br.LOG_N)

    def slots(c):
        return cases.decode(cases.SPARSE, fc.to_host(bctx.decrypt(c.data, sk)), c.level, c.scale)

    err = float(np.abs(slots(out) - su["z"]).max())
    print(f"sparse bootstrap under device keys: max slot error {err:.4e} "
          f"(CPU run {cases.SPARSE_BOOTSTRAP_ERR:.4e})")
    assert err < 2 * cases.SPARSE_BOOTSTRAP_ERR
    # the device decoder reads the same slots
    dev = host(bctx.decode(bctx.decrypt(out.data, sk), float(out.scale), level=out.level,
                           log_slots=sp.LOG_SLOTS))
    assert (bits64(dev) == bits64(slots(out))).all()
    again = boot.bootstrap(out)
    assert again.level == br.OUT_LEVEL
    err2 = float(np.abs(slots(again) - su["z"]).max())
    print(f"second sparse bootstrap: max slot error {err2:.4e}")
    assert err2 < 4 * cases.SPARSE_BOOTSTRAP_ERR
