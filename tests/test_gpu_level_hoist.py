"""GPU parity for the hoisted rotations, the rotation sums and the BSGS linear transform below the
top level (fhe_rotate_hoisted_level, fhe_rotate_sum_hoisted_level, fhe_rotate_sum_multi_level,
fhe_linear_transform_level; include/fhecore.h) against pyoracle at the level, bit for bit: the
levels of contexts on each path (FAST k_rot_sum with the fused ModDown, alpha = 4, dnum > 4, K > 4,
split30, wide), batch 1 and 3 (3 is a partial group of the kernel's 2-ciphertext blocks), one key
tensor and one plaintext tensor per context serving every level in place."""
import ctypes
import random

import numpy as np
import pytest

import coracle
import pyoracle
import refs

pytestmark = pytest.mark.gpu
NTT = refs.c_ntt()


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


def rand(mods, log_n, lead=(), seed=0):
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    return np.stack([rng.integers(0, q, size=lead + (n,), dtype=np.uint64) for q in mods],
                    axis=len(lead))


# (log_n, L, K, dnum, bits): alpha = 2, FAST k_rot_sum, fused ModDown, partial and full last
# digits; alpha = 4, dl = 1 and 2; dnum > 4 (non-FAST, alpha = 1); K > 4 (k_moddown_finish with
# both addends); a 61-bit chain (split30) and a 62-bit one (WIDE)
CONTEXTS = [(10, 5, 2, 3, 60), (11, 7, 4, 2, 60), (10, 6, 2, 6, 60), (10, 4, 5, 2, 60),
            (10, 5, 2, 3, 61), (10, 5, 2, 3, 62)]


def levels_of(i):
    """Every level of the first two contexts; 1, L - 1, L and one partial-digit level (where one
    exists) of the others."""
    _, L, _, dnum, _ = CONTEXTS[i]
    if i < 2:
        return list(range(1, L + 1))
    alpha = -(-L // dnum)
    partial = [lv for lv in range(2, L) if lv % alpha]
    return sorted({1, L - 1, L} | set(partial[-1:]))


CASES = [(i, lv) for i in range(len(CONTEXTS)) for lv in levels_of(i)]
_WORLD = {}


def world(fc, i):
    """Context i, its Galois elements, and ONE key tensor and ONE plaintext tensor on the device,
    uploaded once and used at every level (the in-place read)."""
    if i in _WORLD:
        return _WORLD[i]
    log_n, L, K, dnum, bits = CONTEXTS[i]
    if bits == 60:
        ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    else:  # as tests/test_gpu_wide.py builds its chains
        m = fc.gen_moduli(log_n, L + K, bits=bits)
        ctx = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    n = 1 << log_n
    elts = [pow(5, 1, 2 * n), pow(pow(5, 2, 2 * n), -1, 2 * n), 2 * n - 1]
    allm = ctx.all_moduli
    hk = rand(allm, log_n, (len(elts), 2, dnum), seed=900 + i)  # [elt][b / a][dnum][L + K][N]
    hp = rand(allm, log_n, (4,), seed=950 + i)                  # [4][L + K][N]
    dk, dp = fc.to_device(hk), fc.to_device(hp)
    w = dict(ctx=ctx, log_n=log_n, L=L, K=K, dnum=dnum, n=n, qs=ctx.moduli, ps=allm[L:],
             elts=elts, hk=hk, hp=hp, dk=dk, dp=dp,
             hkeys={k: (hk[r, 0], hk[r, 1]) for r, k in enumerate(elts)},
             dkeys={k: (dk[r, 0], dk[r, 1]) for r, k in enumerate(elts)})
    _WORLD[i] = w
    return w


def keys_for(w, ks, dev):
    src = w["dkeys"] if dev else w["hkeys"]
    return [src.get(k) for k in ks]


def same(got, want):
    return got.shape == want.shape and (got.astype(object) == want).all()


@pytest.mark.parametrize("i,level", CASES)
def test_rotate_sum_and_rotate_hoisted_match_the_reference(fc, i, level):
    w = world(fc, i)
    ctx, qs, ps, dnum, log_n = w["ctx"], w["qs"], w["ps"], w["dnum"], w["log_n"]
    e1, e2, conj = w["elts"]
    ct = rand(qs[:level], log_n, (3, 2), seed=100 * i + level)
    dct = fc.to_device(ct)
    ks = [1, e1, e2, conj]
    pts = [w["dp"][r] for r in range(4)]
    want = [pyoracle.rotate_sum_hoisted(ct[b], ks, keys_for(w, ks, False), w["hp"], qs, ps, dnum,
                                        log_n, level=level, ntt=NTT) for b in range(3)]
    hks = [e1, conj]
    hwant = [pyoracle.rotate_hoisted(ct[b], hks, keys_for(w, hks, False), qs, ps, dnum, log_n,
                                     level=level, ntt=NTT) for b in range(3)]
    for batch in (1, 3):
        got = fc.to_host(ctx.rotate_sum_hoisted(dct[:batch], ks, keys_for(w, ks, True), pts))
        assert got.shape == (batch, 2, level, w["n"])
        for b in range(batch):
            assert same(got[b], want[b]), ("rotate_sum_hoisted", level, batch, b)
        got = fc.to_host(ctx.rotate_hoisted(dct[:batch], hks, keys_for(w, hks, True)))
        assert got.shape == (2, batch, 2, level, w["n"])
        for b in range(batch):
            assert same(got[:, b], hwant[b]), ("rotate_hoisted", level, batch, b)


@pytest.mark.parametrize("i,level", CASES)
def test_rotate_sum_multi_and_linear_transform_match_the_reference(fc, i, level):
    w = world(fc, i)
    ctx, qs, ps, dnum, log_n = w["ctx"], w["qs"], w["ps"], w["dnum"], w["log_n"]
    e1, e2, conj = w["elts"]
    cts = [rand(qs[:level], log_n, (3, 2), seed=100 * i + level + 1000 * (r + 1))
           for r in range(3)]
    dcts = [fc.to_device(c) for c in cts]
    mks = [e1, 1, conj]  # three ciphertexts, one of them unrotated
    mwant = [pyoracle.rotate_sum_multi([c[b] for c in cts], mks, keys_for(w, mks, False), qs, ps,
                                       dnum, log_n, level=level, ntt=NTT) for b in range(3)]
    baby, giant = [1, e1], [e2, 1]  # n1 = n2 = 2, an element 1 in each list
    hpts = [[w["hp"][0], w["hp"][1]], [w["hp"][2], w["hp"][3]]]
    dpts = [[w["dp"][0], w["dp"][1]], [w["dp"][2], w["dp"][3]]]
    lwant = [pyoracle.linear_transform(cts[0][b], baby, keys_for(w, baby, False), giant,
                                       keys_for(w, giant, False), hpts, qs, ps, dnum, log_n,
                                       level=level, ntt=NTT) for b in range(3)]
    for batch in (1, 3):
        got = fc.to_host(ctx.rotate_sum_multi([c[:batch] for c in dcts], mks,
                                              keys_for(w, mks, True)))
        assert got.shape == (batch, 2, level, w["n"])
        for b in range(batch):
            assert same(got[b], mwant[b]), ("rotate_sum_multi", level, batch, b)
        got = fc.to_host(ctx.linear_transform(dcts[0][:batch], baby, keys_for(w, baby, True), giant,
                                              keys_for(w, giant, True), dpts))
        assert got.shape == (batch, 2, level, w["n"])
        for b in range(batch):
            assert same(got[b], lwant[b]), ("linear_transform", level, batch, b)


# ---- the C entry points themselves -------------------------------------------------------------
def _arr(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _kp(w, ks, h):
    return _arr([w["dkeys"][k][h].data_ptr() if k != 1 else None for k in ks])


def c_rotate_hoisted(fc, w, out, ct, ks, level, batch, ws=None):
    """fhe_rotate_hoisted_level (level not None) or fhe_rotate_hoisted, through ctypes."""
    lib = fc.load()
    g = (ctypes.c_uint32 * len(ks))(*ks)
    head = (w["ctx"].handle, out.data_ptr(), ct.data_ptr(), g, _kp(w, ks, 0), _kp(w, ks, 1))
    tail = (len(ks), batch, ws.data_ptr() if ws is not None else None, None)
    if level is None:
        return lib.fhe_rotate_hoisted(*head, *tail)
    return lib.fhe_rotate_hoisted_level(*head, level, *tail)


def c_rotate_sum_hoisted(fc, w, out, ct, ks, level, batch, ws=None):
    lib = fc.load()
    g = (ctypes.c_uint32 * len(ks))(*ks)
    p = _arr([w["dp"][r].data_ptr() for r in range(len(ks))])
    head = (w["ctx"].handle, out.data_ptr(), ct.data_ptr(), g, _kp(w, ks, 0), _kp(w, ks, 1), p)
    tail = (len(ks), batch, ws.data_ptr() if ws is not None else None, None)
    if level is None:
        return lib.fhe_rotate_sum_hoisted(*head, *tail)
    return lib.fhe_rotate_sum_hoisted_level(*head, level, *tail)


def c_rotate_sum_multi(fc, w, out, cts, ks, level, batch, ws=None):
    lib = fc.load()
    g = (ctypes.c_uint32 * len(ks))(*ks)
    head = (w["ctx"].handle, out.data_ptr(), _arr([c.data_ptr() for c in cts]), g, _kp(w, ks, 0),
            _kp(w, ks, 1))
    tail = (len(ks), batch, ws.data_ptr() if ws is not None else None, None)
    if level is None:
        return lib.fhe_rotate_sum_multi(*head, *tail)
    return lib.fhe_rotate_sum_multi_level(*head, level, *tail)


def c_linear_transform(fc, w, out, ct, baby, giant, level, batch, ws=None):
    lib = fc.load()
    bg = (ctypes.c_uint32 * len(baby))(*baby)
    gg = (ctypes.c_uint32 * len(giant))(*giant)
    p = _arr([w["dp"][r].data_ptr() for r in range(len(baby) * len(giant))])
    head = (w["ctx"].handle, out.data_ptr(), ct.data_ptr(), len(baby), len(giant), bg,
            _kp(w, baby, 0), _kp(w, baby, 1), gg, _kp(w, giant, 0), _kp(w, giant, 1), p)
    tail = (batch, ws.data_ptr() if ws is not None else None, None)
    if level is None:
        return lib.fhe_linear_transform(*head, *tail)
    return lib.fhe_linear_transform_level(*head, level, *tail)


def four_calls(fc, w, level, batch, seed):
    """The four operations' inputs at `level` and one runner each: run(level_arg, ws) -> the
    output tensor (level_arg None: the top-level entry point)."""
    import torch

    qs, log_n, n = w["qs"], w["log_n"], w["n"]
    e1, e2, conj = w["elts"]
    cts = [fc.to_device(rand(qs[:level], log_n, (batch, 2), seed=seed + r)) for r in range(3)]
    lib = fc.load()

    def runner(shape, call):
        def run(level_arg, ws=None):
            out = torch.full(shape, -1, dtype=torch.int64, device="cuda")
            rc = call(out, level_arg, ws)
            torch.cuda.synchronize()
            assert rc == 0, lib.fhe_last_error()
            return out
        return run

    ct_shape = (batch, 2, level, n)
    return {
        "rotate_hoisted": runner((2,) + ct_shape, lambda o, lv, ws: c_rotate_hoisted(
            fc, w, o, cts[0], [e1, conj], lv, batch, ws)),
        "rotate_sum_hoisted": runner(ct_shape, lambda o, lv, ws: c_rotate_sum_hoisted(
            fc, w, o, cts[0], [1, e1, e2, conj], lv, batch, ws)),
        "rotate_sum_multi": runner(ct_shape, lambda o, lv, ws: c_rotate_sum_multi(
            fc, w, o, cts, [e1, 1, conj], lv, batch, ws)),
        "linear_transform": runner(ct_shape, lambda o, lv, ws: c_linear_transform(
            fc, w, o, cts[0], [1, e1], [e2, 1], lv, batch, ws)),
    }


@pytest.mark.parametrize("i", range(len(CONTEXTS)))
def test_level_entry_points_at_L_equal_the_top_level_ones(fc, i):
    w = world(fc, i)
    for name, run in four_calls(fc, w, w["L"], 3, seed=7000 + 10 * i).items():
        assert (fc.to_host(run(w["L"])) == fc.to_host(run(None))).all(), name


def workspace_bytes(fc, w, name, batch):
    lib, h = fc.load(), w["ctx"].handle
    return {"rotate_hoisted": lambda: lib.fhe_rotate_hoisted_workspace(h, batch),
            "rotate_sum_hoisted": lambda: lib.fhe_rotate_sum_hoisted_workspace(h, batch),
            "rotate_sum_multi": lambda: lib.fhe_rotate_sum_multi_workspace(h, 3, batch),
            "linear_transform": lambda: lib.fhe_linear_transform_workspace(h, 2, batch)}[name]()


@pytest.mark.parametrize("level", [1, 4])
def test_the_top_level_workspace_size_suffices_and_nothing_is_written_past_it(fc, level):
    """An explicit workspace of exactly *_workspace(...) bytes (sized for L) followed by a 4 KiB
    guard: the result equals the internal-workspace call and the guard is untouched."""
    import torch

    w = world(fc, 0)
    assert level in (1, w["L"] - 1)
    batch = 3
    for name, run in four_calls(fc, w, level, batch, seed=7100 + level).items():
        nbytes = workspace_bytes(fc, w, name, batch)
        assert nbytes % 8 == 0
        buf = torch.full((nbytes // 8 + 512,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        want = fc.to_host(run(level))
        got = fc.to_host(run(level, buf))
        assert (got == want).all(), name
        assert (buf[nbytes // 8:] == 0x5A5A5A5A5A5A5A5A).all().item(), name
    # ... and `want` itself is the reference (ciphertext 0)
    e1, e2, conj = w["elts"]
    ct = rand(w["qs"][:level], w["log_n"], (batch, 2), seed=7100 + level)
    ks = [1, e1, e2, conj]
    got = fc.to_host(four_calls(fc, w, level, batch, seed=7100 + level)["rotate_sum_hoisted"](level))
    assert same(got[0], pyoracle.rotate_sum_hoisted(ct[0], ks, keys_for(w, ks, False), w["hp"],
                                                    w["qs"], w["ps"], w["dnum"], w["log_n"],
                                                    level=level, ntt=NTT))


def test_graph_replay_of_a_linear_transform_at_level_3(fc):
    import torch

    w = world(fc, 0)
    ctx, level, batch = w["ctx"], 3, 2
    e1, e2, _ = w["elts"]
    baby, giant = [1, e1], [e2, 1]
    dpts = [[w["dp"][0], w["dp"][1]], [w["dp"][2], w["dp"][3]]]
    ct = fc.to_device(rand(w["qs"][:level], w["log_n"], (batch, 2), seed=7200))
    args = (ct, baby, keys_for(w, baby, True), giant, keys_for(w, giant, True), dpts)
    eager = fc.to_host(ctx.linear_transform(*args))
    ws = ctx.workspace(fc.load().fhe_linear_transform_workspace(ctx.handle, 2, batch))
    out = torch.empty(batch, 2, level, w["n"], dtype=torch.int64, device=ct.device)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.linear_transform(*args, workspace=ws, out=out)
        for _ in range(2):
            out.zero_()
            g.launch()
            stream.synchronize()
            assert (fc.to_host(out) == eager).all()


def test_level_arguments_and_overlap_are_refused_before_any_launch(fc):
    import torch

    w = world(fc, 0)
    L, n, lib = w["L"], w["n"], fc.load()
    e1, e2, conj = w["elts"]
    ct = fc.to_device(rand(w["qs"], w["log_n"], (1, 2), seed=7300))
    for level in (0, L + 1):
        out = torch.full((2, 1, 2, L + 1, n), -1, dtype=torch.int64, device="cuda")
        for rc in (c_rotate_hoisted(fc, w, out, ct, [e1, conj], level, 1),
                   c_rotate_sum_hoisted(fc, w, out, ct, [1, e1], level, 1),
                   c_rotate_sum_multi(fc, w, out, [ct, ct], [e1, 1], level, 1),
                   c_linear_transform(fc, w, out, ct, [1, e1], [e2, 1], level, 1)):
            assert rc == -1 and b"level" in lib.fhe_last_error()
        torch.cuda.synchronize()
        assert (out == -1).all().item()
    # out overlapping in at a level below the top: FHE_EINVAL, nothing written
    level = 3
    buf = torch.full((2 * level * n + n,), -1, dtype=torch.int64, device="cuda")
    src = buf[:2 * level * n].view(1, 2, level, n)
    h = rand(w["qs"][:level], w["log_n"], (1, 2), seed=7301)
    src.copy_(fc.to_device(h))
    shifted = buf[n:]
    for rc in (c_rotate_hoisted(fc, w, shifted, src, [e1], level, 1),
               c_rotate_sum_hoisted(fc, w, shifted, src, [1, e1], level, 1),
               c_rotate_sum_multi(fc, w, shifted, [src, src], [e1, 1], level, 1),
               c_linear_transform(fc, w, shifted, src, [1, e1], [e2, 1], level, 1)):
        assert rc == -1 and b"overlap" in lib.fhe_last_error()
    torch.cuda.synchronize()
    assert (fc.to_host(src) == h).all() and (buf[2 * level * n:] == -1).all().item()


# ---- end to end with device-generated keys -----------------------------------------------------
def _sigma_int(m, k, n):
    idx = (np.arange(n, dtype=np.int64) * k) % (2 * n)
    out = np.zeros(n, dtype=np.int64)
    out[idx % n] = np.where(idx < n, m, -m)
    return out


def _negacyclic_i64(a, b, n):
    full = np.convolve(a, b)
    out = full[:n].copy()
    out[:n - 1] -= full[n:]
    return out


def test_end_to_end_linear_transform_at_level_2_under_device_keys(fc):
    """encrypt, two mul_relin(rescale=True) (level 4 -> 2), linear_transform at level 2, decrypt,
    with keygen_secret / keygen_relin / keygen_rotation keys: the result is the reference applied
    to the same ciphertext, and the error the transform adds -- decryption minus the transform of
    the input's own decryption, mod Q_l -- is within 4x the same figure of the top-level call
    (tests/test_level_hoist_cpu.py's method: the trusted l = L path is the yardstick)."""
    log_n, L, K, dnum = 12, 4, 2, 2
    n = 1 << log_n
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    qs, ps, allm = ctx.moduli, ctx.all_moduli[L:], ctx.all_moduli
    d = fc.to_device
    sk = ctx.keygen_secret(seed=21)
    pk = ctx.keygen_public(sk, seed=22)
    rb, ra = ctx.keygen_relin(sk, seed=23)
    s_n = fc.to_host(sk).astype(object)
    e1, e2 = ctx.galois_elt(1), ctx.galois_elt(-2)
    baby, giant = [1, e1], [e2, 1]
    rk = {k: ctx.keygen_rotation(sk, k, seed=30 + j) for j, k in enumerate((e1, e2))}
    rng = random.Random(24)
    pt_int = [np.array([rng.randrange(-3, 4) for _ in range(n)], dtype=np.int64) for _ in range(4)]
    hpts = [coracle.ntt_fwd(np.asarray(pyoracle._to_rns(p.tolist(), allm), dtype=np.uint64), allm)
            for p in pt_int]
    dp = [d(p) for p in hpts]
    dpts, hpts2 = [dp[:2], dp[2:]], [hpts[:2], hpts[2:]]
    bk, gk = [rk.get(k) for k in baby], [rk.get(k) for k in giant]
    hk = lambda kk: None if kk is None else (fc.to_host(kk[0]), fc.to_host(kk[1]))  # noqa: E731

    delta = 1 << 50
    msgs = [(rng.choice([-3, -2, -1, 1, 2, 3]), rng.randrange(n)) for _ in range(3)]

    def enc(c, k, seed):
        m = [0] * n
        m[k] = c * delta
        pt = coracle.ntt_fwd(np.asarray(pyoracle._to_rns(m, qs), dtype=np.uint64), qs)
        return ctx.encrypt(d(pt), pk, seed=seed)

    cts = [enc(c, k, 200 + j) for j, (c, k) in enumerate(msgs)]

    def decrypt(ct, level):
        ql = qs[:level]
        dec = (ct[0].astype(object) + ct[1].astype(object) * s_n[:level]) % pyoracle._mods_col(ql)
        return pyoracle.crt_centered(coracle.ntt_inv(np.asarray(dec, dtype=np.uint64), ql)
                                     .astype(object), ql)

    def added_error(ct_in, ct_out, level):
        m_in = decrypt(ct_in, level)
        assert max(abs(int(v)) for v in m_in) < 1 << 45  # the int64 convolutions below are exact
        m_in = np.array([int(v) for v in m_in], dtype=np.int64)
        expect = np.zeros(n, dtype=np.int64)
        for g, kg in enumerate(giant):
            inner = np.zeros(n, dtype=np.int64)
            for b, kb in enumerate(baby):
                inner += _negacyclic_i64(pt_int[2 * g + b], _sigma_int(m_in, kb, n), n)
            expect += _sigma_int(inner, kg, n)
        Q = 1
        for q in qs[:level]:
            Q *= q
        diff = [(int(x) - int(e)) % Q for x, e in zip(decrypt(ct_out, level), expect)]
        return max(min(v, Q - v) for v in diff)

    # the yardstick: the top-level call on a fresh encryption of a small message
    m0 = [rng.randrange(-1000, 1000) for _ in range(n)]
    top_in = ctx.encrypt(d(coracle.ntt_fwd(np.asarray(pyoracle._to_rns(m0, qs), dtype=np.uint64),
                                           qs)), pk, seed=210)
    top_out = ctx.linear_transform(top_in, baby, bk, giant, gk, dpts)
    top = added_error(fc.to_host(top_in), fc.to_host(top_out), L)

    x = cts[0]
    for j, level in enumerate((4, 3)):
        x = ctx.mul_relin(x, cts[j + 1][:, :level].contiguous(), rb, ra, rescale=True)
    assert x.shape == (2, 2, n)
    got = fc.to_host(ctx.linear_transform(x, baby, bk, giant, gk, dpts))
    hx = fc.to_host(x)
    want = pyoracle.linear_transform(hx, baby, [hk(k) for k in bk], giant, [hk(k) for k in gk],
                                     hpts2, qs, ps, dnum, log_n, level=2, ntt=NTT)
    assert same(got, want)
    err = added_error(hx, got, 2)
    print(f"linear_transform added error: top level {top}, level 2 {err}")
    assert err <= 4 * top


def test_full_size_level_13_partial_digit(fc):
    """N = 2^16, L = 16, K = 4, dnum = 4 at level 13 (four digits, the last one partial; the
    512 x 128 split): rotate_sum_hoisted with 3 terms, batch 3.  Ciphertext 0 against the
    reference, the other two each against their own single-ciphertext call.  At this size the
    reference is evaluated by its C restatement: level 13's digits are digit_ranges(13, 4), so
    rotate_sum_hoisted at that level is the top-level rotate_sum_hoisted on the key and plaintext
    rows the level reads (tests/test_level_hoist_cpu.py checks that identity word for word)."""
    log_n, L, K, dnum, level, B = 16, 16, 4, 4, 13, 3
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    qs, ps, allm = ctx.moduli, ctx.all_moduli[L:], ctx.all_moduli
    assert pyoracle.digit_ranges(L, dnum, level) == pyoracle.digit_ranges(level, dnum)
    ct = rand(qs[:level], log_n, (B, 2), seed=61)
    ks = [ctx.galois_elt(1), 1, ctx.galois_elt(-4)]
    kb = rand(allm, log_n, (len(ks), dnum), seed=62)
    ka = rand(allm, log_n, (len(ks), dnum), seed=63)
    pts = rand(allm, log_n, (len(ks),), seed=64)
    d = lambda v: fc.to_device(np.ascontiguousarray(v))  # noqa: E731
    dkeys = [None if k == 1 else (d(kb[r]), d(ka[r])) for r, k in enumerate(ks)]
    dpts = [d(pts[r]) for r in range(len(ks))]
    dct = d(ct)
    got = fc.to_host(ctx.rotate_sum_hoisted(dct, ks, dkeys, dpts))
    assert got.shape == (B, 2, level, 1 << log_n)
    for b in (1, 2):
        one = fc.to_host(ctx.rotate_sum_hoisted(dct[b:b + 1], ks, dkeys, dpts))
        assert (one[0] == got[b]).all(), b
    rows = pyoracle.key_rows(level, L, K)
    cut = lambda v: np.ascontiguousarray(v[..., rows, :])  # noqa: E731
    want = coracle.rotate_sum_hoisted(ct[0], ks, cut(kb), cut(ka), cut(pts), qs[:level], ps, dnum)
    assert (got[0] == want).all()
