"""GPU parity for the level-aware key-switch, multiply-relinearise and rotation (fhe_keyswitch_level,
fhe_mul_relin_level, fhe_rotate_level; include/fhecore.h) against pyoracle at the level, bit for bit,
every level l = 1 .. L of contexts on each key-switch path (fused lz16, split30, unfused dnum > 4,
wide, K > 4, both sides of the fused-ModDown predicate), the top-level key read in place."""
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


_CTX = {}


def ctx_for(fc, log_n, L, K, dnum, bits=60):
    key = (log_n, L, K, dnum, bits)
    if key not in _CTX:
        if bits == 60:
            _CTX[key] = fc.Context(log_n, L=L, K=K, dnum=dnum)
        else:  # as tests/test_gpu_wide.py builds its chains
            m = fc.gen_moduli(log_n, L + K, bits=bits)
            _CTX[key] = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    return _CTX[key]


GUARD = 0x5A5A5A5A5A5A5A5A


class Guarded:
    """An explicit workspace of exactly `nbytes` (a public fhe_*_workspace value, sized for L)
    followed by a 4 KiB guard of a fixed pattern: runs at every level must leave the guard alone."""

    def __init__(self, nbytes):
        import torch

        assert nbytes % 8 == 0
        self.words = nbytes // 8
        self.buf = torch.full((self.words + 512,), GUARD, dtype=torch.int64, device="cuda")

    def intact(self):
        return (self.buf[self.words:] == GUARD).all().item()


def pass_batch(fc, ctx, batch):
    return fc.load().fhe_keyswitch_pass_batch(ctx.handle, batch)


def _top_level_c(fc, ctx, name, outs, *args):
    """The C symbol `name` without a level argument, called directly on the default stream with
    the library's own workspace (the Context methods call the *_level entry points at every level,
    L included)."""
    import torch
    from fhecore.context import _ptr

    lib = fc.load()
    rc = getattr(lib, name)(ctx.handle, *[_ptr(o) for o in outs],
                            *[_ptr(a) if isinstance(a, torch.Tensor) else a for a in args],
                            None, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.fhe_last_error()
    return outs


# (log_n, L, K, dnum, bits): alpha = 2 on the fused lz16 path, partial and full last digits;
# alpha = 4 with l = 1 .. 3 on the other side of dl (l + K) >= 2 K; dnum > 4 (unfused kernels);
# K > 4; a 61-bit chain (fused, split30 sources) and a 62-bit one (wide: exact butterflies)
KS_CONTEXTS = [(10, 5, 2, 3, 60), (11, 7, 4, 2, 60), (10, 6, 2, 6, 60), (10, 4, 5, 2, 60),
               (10, 5, 2, 3, 61), (10, 5, 2, 3, 62)]


@pytest.mark.parametrize("log_n,L,K,dnum,bits", KS_CONTEXTS)
def test_keyswitch_every_level(fc, log_n, L, K, dnum, bits):
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    kb = rand(ctx.all_moduli, log_n, (dnum,), seed=31)
    ka = rand(ctx.all_moduli, log_n, (dnum,), seed=32)
    d = fc.to_device
    dkb, dka = d(kb), d(ka)
    lib = fc.load()
    guarded = {b: Guarded(lib.fhe_keyswitch_workspace(ctx.handle, L, pass_batch(fc, ctx, b)))
               for b in (1, 3)}
    for level in range(1, L + 1):
        d2 = rand(qs[:level], log_n, (3,), seed=40 + level)
        want = [pyoracle.keyswitch(d2[i], kb, ka, qs, ps, dnum, level=level, ntt=NTT)
                for i in range(3)]
        for batch in (1, 3):
            # the wrapper's own workspace, then exactly fhe_keyswitch_workspace bytes and a guard
            for ws in (None, guarded[batch]):
                ks0, ks1 = ctx.keyswitch(d(d2[:batch]), dkb, dka,
                                         workspace=None if ws is None else ws.buf)
                g0, g1 = fc.to_host(ks0), fc.to_host(ks1)
                assert g0.shape == (batch, level, 1 << log_n)
                for i in range(batch):
                    assert (g0[i].astype(object) == want[i][0]).all(), (level, batch, i, 0)
                    assert (g1[i].astype(object) == want[i][1]).all(), (level, batch, i, 1)
                assert ws is None or ws.intact(), (level, batch)
    # level == L through the level entry point: fhe_keyswitch word for word
    d2 = d(rand(qs, log_n, (3,), seed=50))
    l0, l1 = ctx.keyswitch(d2, dkb, dka)
    t0, t1 = _top_level_c(fc, ctx, "fhe_keyswitch", [ctx.empty(*d2.shape), ctx.empty(*d2.shape)],
                          d2, dkb, dka, 3)
    assert (fc.to_host(l0) == fc.to_host(t0)).all() and (fc.to_host(l1) == fc.to_host(t1)).all()


@pytest.mark.parametrize("log_n,L,K,dnum", [(10, 5, 2, 3), (12, 4, 2, 2)])
def test_mul_relin_every_level(fc, log_n, L, K, dnum):
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    kb = rand(ctx.all_moduli, log_n, (dnum,), seed=3)
    ka = rand(ctx.all_moduli, log_n, (dnum,), seed=4)
    d = fc.to_device
    dkb, dka = d(kb), d(ka)
    batch = 2
    ws = Guarded(fc.load().fhe_mul_relin_workspace(ctx.handle, pass_batch(fc, ctx, batch)))
    for level in range(1, L + 1):
        a = rand(qs[:level], log_n, (batch, 2), seed=60 + level)
        b = rand(qs[:level], log_n, (batch, 2), seed=70 + level)
        for rescale in (False, True):
            if rescale and level < 2:
                with pytest.raises(fc.FheError):  # FHE_EINVAL: nothing to rescale into
                    ctx.mul_relin(d(a), d(b), dkb, dka, rescale=True)
                continue
            got = fc.to_host(ctx.mul_relin(d(a), d(b), dkb, dka, rescale=rescale))
            # again in exactly fhe_mul_relin_workspace bytes followed by a guard
            again = fc.to_host(ctx.mul_relin(d(a), d(b), dkb, dka, rescale=rescale,
                                             workspace=ws.buf))
            assert got.shape == (batch, 2, level - (1 if rescale else 0), 1 << log_n)
            for i in range(batch):
                want = pyoracle.mul_relin(a[i], b[i], kb, ka, qs, ps, dnum, rescale, level=level,
                                          ntt=NTT)
                assert (got[i].astype(object) == want).all(), (level, rescale, i)
                assert (again[i].astype(object) == want).all(), (level, rescale, i, "explicit ws")
            assert ws.intact(), (level, rescale)


@pytest.mark.parametrize("log_n,L,K,dnum", [(10, 5, 2, 3), (10, 6, 2, 6)])
def test_rotate_every_level(fc, log_n, L, K, dnum):
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    two_n = 2 << log_n
    sk = ctx.keygen_secret(seed=5)
    d = fc.to_device
    ws = Guarded(fc.load().fhe_rotate_workspace(ctx.handle, pass_batch(fc, ctx, 1)))
    for g in (5, two_n - 1, pow(5, -1, two_n)):
        rb, ra = ctx.keygen_rotation(sk, g, seed=6 + g)
        hb, ha = fc.to_host(rb), fc.to_host(ra)
        for level in range(1, L + 1):
            ct = rand(qs[:level], log_n, (2,), seed=80 + level)
            got = fc.to_host(ctx.rotate(d(ct), g, rb, ra))
            want = pyoracle.rotate(ct, g, hb, ha, qs, ps, dnum, log_n, level=level, ntt=NTT)
            assert (got.astype(object) == want).all(), (g, level)
            # again in exactly fhe_rotate_workspace bytes followed by a guard
            again = fc.to_host(ctx.rotate(d(ct), g, rb, ra, workspace=ws.buf))
            assert (again.astype(object) == want).all(), (g, level, "explicit ws")
            assert ws.intact(), (g, level)


@pytest.mark.parametrize("bits", [60, 62])
def test_top_level_symbols_equal_their_level_twins_at_L(fc, bits):
    """fhe_keyswitch, fhe_rotate and fhe_mul_relin, which the Context methods no longer call, are
    fhe_*_level at level = L word for word (the hoisted four: tests/test_gpu_level_hoist.py).  The
    smallest context the library builds, batch 1; the 62-bit chain takes the wide path."""
    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    d = fc.to_device
    kb, ka = d(rand(ctx.all_moduli, log_n, (dnum,), seed=31)), d(rand(ctx.all_moduli, log_n,
                                                                      (dnum,), seed=32))
    a, b = d(rand(ctx.moduli, log_n, (1, 2), seed=33)), d(rand(ctx.moduli, log_n, (1, 2), seed=34))
    d2 = a[:, 1].contiguous()
    l0, l1 = ctx.keyswitch(d2, kb, ka)
    t0, t1 = _top_level_c(fc, ctx, "fhe_keyswitch", [ctx.empty(*d2.shape), ctx.empty(*d2.shape)],
                          d2, kb, ka, 1)
    assert (fc.to_host(l0) == fc.to_host(t0)).all() and (fc.to_host(l1) == fc.to_host(t1)).all()
    for g in (5, (2 << log_n) - 1):
        top, = _top_level_c(fc, ctx, "fhe_rotate", [ctx.empty(*a.shape)], a, g, kb, ka, 1)
        assert (fc.to_host(ctx.rotate(a, g, kb, ka)) == fc.to_host(top)).all(), g
    for rescale in (0, 1):
        top, = _top_level_c(fc, ctx, "fhe_mul_relin", [ctx.empty(1, 2, L - rescale, 1 << log_n)],
                            a, b, kb, ka, 1, rescale)
        assert (fc.to_host(ctx.mul_relin(a, b, kb, ka, rescale=bool(rescale))) ==
                fc.to_host(top)).all(), rescale


def test_depth_chain_under_real_keys(fc):
    """x <- mul_relin(x, enc(m_i) cut to x's level, rescale) three times, level 4 -> 1, with keys
    from ctx.keygen_*: every intermediate equals the pyoracle chain bit for bit and the result
    decrypts to the product of the monomials at the tracked scale.  Delta = 2^50 with 60-bit primes
    leaves scale ~2^20 at level 1 (|m| <= 81, far below q_0 / 2); the bound is the 1e-3 of the
    tracked scale that tests/test_gpu_pipeline.py uses for one level."""
    log_n, L, K, dnum = 10, 4, 2, 2
    n = 1 << log_n
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    d = fc.to_device
    sk = ctx.keygen_secret(seed=11)
    pk = ctx.keygen_public(sk, seed=12)
    rb, ra = ctx.keygen_relin(sk, seed=13)
    hb, ha, s_n = fc.to_host(rb), fc.to_host(ra), fc.to_host(sk).astype(object)
    delta = 1 << 50
    rng = random.Random(14)
    msgs = [(rng.choice([-3, -2, -1, 1, 2, 3]), rng.randrange(n)) for _ in range(4)]

    def enc(c, k, seed):
        m = [0] * n
        m[k] = c * delta
        pt = coracle.ntt_fwd(np.asarray(pyoracle._to_rns(m, qs), dtype=np.uint64), qs)
        return ctx.encrypt(d(pt), pk, seed=seed)

    cts = [enc(c, k, 100 + i) for i, (c, k) in enumerate(msgs)]
    hcts = [fc.to_host(t) for t in cts]

    def decrypt(ct, level):
        ql = qs[:level]
        dec_n = (ct[0].astype(object) + ct[1].astype(object) * s_n[:level]) % pyoracle._mods_col(ql)
        return pyoracle.crt_centered(coracle.ntt_inv(np.asarray(dec_n, dtype=np.uint64), ql)
                                     .astype(object), ql)

    # the oracle chain alone, on the CPU
    ref, chain, scale = hcts[0], [], float(delta)
    for i, level in enumerate((4, 3, 2)):
        ref = pyoracle.mul_relin(ref, hcts[i + 1][:, :level], hb, ha, qs, ps, dnum, True,
                                 level=level, ntt=NTT)
        chain.append(ref)
        scale = scale * delta / qs[level - 1]
    coef, expo = 1, 0
    for c, k in msgs:
        coef, expo = coef * c, expo + k
    want = [0] * n
    want[expo % n] = coef * (-1) ** (expo // n)

    def error(ct):
        return max(abs(int(x) - w * scale) for x, w in zip(decrypt(ct, 1), want))

    print(f"scale 2^{np.log2(scale):.3f}, oracle chain error {error(chain[-1]):.1f}, "
          f"bound {scale * 1e-3:.1f}")
    assert error(chain[-1]) < scale * 1e-3
    x = cts[0]
    for i, level in enumerate((4, 3, 2)):
        x = ctx.mul_relin(x, cts[i + 1][:, :level].contiguous(), rb, ra, rescale=True)
        assert (fc.to_host(x).astype(object) == chain[i]).all(), level
    assert error(fc.to_host(x)) < scale * 1e-3


def test_full_size_partial_last_digit(fc):
    """N = 2^16, L = 16, K = 4, dnum = 4 at level 13: four digits, the last one partial.  The
    truncated ranges equal digit_ranges(13, 4) (ceil(13 / 4) = 4 = alpha), so the C oracle's
    key-switch on the sliced key is the reference.  The LOGN = 16 instantiations and their XCD
    placement branch."""
    log_n, L, K, dnum, level, batch = 16, 16, 4, 4, 13, 2
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    assert pyoracle.digit_ranges(L, dnum, level) == pyoracle.digit_ranges(level, dnum)
    kb = rand(ctx.all_moduli, log_n, (dnum,), seed=91)
    ka = rand(ctx.all_moduli, log_n, (dnum,), seed=92)
    d2 = rand(qs[:level], log_n, (batch,), seed=93)
    d = fc.to_device
    ks0, ks1 = ctx.keyswitch(d(d2), d(kb), d(ka))
    g0, g1 = fc.to_host(ks0), fc.to_host(ks1)
    rows = pyoracle.key_rows(level, L, K)
    skb, ska = np.ascontiguousarray(kb[:, rows]), np.ascontiguousarray(ka[:, rows])
    for i in range(batch):
        w0, w1 = coracle.keyswitch(d2[i], skb, ska, qs[:level], ps, dnum)
        assert (g0[i] == w0).all() and (g1[i] == w1).all(), i


def test_keyswitch_shard_with_an_empty_last_digit(fc):
    """L = 5, dnum = 4 gives alpha = 2: digits [0, 2), [2, 4), [4, 5) are live and the fourth is
    empty (its key rows are never read).  fhe_keyswitch_shard as a single rank (limb0 = 0,
    nlimbs = L) on an unprepared c_all = INTT(d2), against pyoracle.keyswitch_shard, whose
    digit_ranges drops the empty digit."""
    log_n, L, K, dnum, batch = 10, 5, 2, 4, 2
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs, ps = ctx.moduli, ctx.all_moduli[L:]
    assert pyoracle.digit_ranges(L, dnum) == [(0, 2), (2, 4), (4, 5)]
    kb = rand(ctx.all_moduli, log_n, (dnum,), seed=97)
    ka = rand(ctx.all_moduli, log_n, (dnum,), seed=98)
    d2 = rand(qs, log_n, (batch,), seed=99)
    d = fc.to_device
    c_all = ctx.intt(d(d2))
    k0, k1 = ctx.keyswitch_shard(c_all, d(d2), d(kb), d(ka), 0)
    g0, g1 = fc.to_host(k0), fc.to_host(k1)
    for i in range(batch):
        w0, w1 = pyoracle.keyswitch_shard(coracle.ntt_inv(d2[i], qs), d2[i], kb, ka, qs, ps, dnum,
                                          0, L)
        assert (g0[i].astype(object) == w0).all() and (g1[i].astype(object) == w1).all(), i


def test_in_place_and_shifted_overlap(fc):
    log_n, L, K, dnum, level = 10, 5, 2, 3, 3
    n = 1 << log_n
    ctx = ctx_for(fc, log_n, L, K, dnum)
    d = fc.to_device
    kb, ka = d(rand(ctx.all_moduli, log_n, (dnum,), seed=31)), d(rand(ctx.all_moduli, log_n,
                                                                      (dnum,), seed=32))
    h = rand(ctx.moduli[:level], log_n, (2,), seed=95)
    o0, o1 = ctx.keyswitch(d(h), kb, ka)
    d2 = d(h)
    ks1 = ctx.empty(2, level, n)
    r0, r1 = ctx.keyswitch(d2, kb, ka, out=(d2, ks1))
    assert r0.data_ptr() == d2.data_ptr()
    assert (fc.to_host(r0) == fc.to_host(o0)).all() and (fc.to_host(r1) == fc.to_host(o1)).all()
    # an output shifted by one row onto d2: refused before anything is launched
    words = 2 * level * n
    buf = ctx.empty(words + n)
    src = buf[:words].view(2, level, n)
    src.copy_(d(h))
    shifted = buf[n:n + words].view(2, level, n)
    with pytest.raises(fc.FheError):
        ctx.keyswitch(src, kb, ka, out=(shifted, ks1))
    assert (fc.to_host(src).astype(np.uint64) == h).all()


def test_graph_replay_at_a_lower_level(fc):
    import torch

    log_n, L, K, dnum, level = 12, 4, 2, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum)
    d = fc.to_device
    ql = ctx.moduli[:level]
    a, b = d(rand(ql, log_n, (2, 2), seed=5)), d(rand(ql, log_n, (2, 2), seed=6))
    kb, ka = d(rand(ctx.all_moduli, log_n, (dnum,), seed=7)), d(rand(ctx.all_moduli, log_n,
                                                                     (dnum,), seed=8))
    eager = fc.to_host(ctx.mul_relin(a, b, kb, ka, rescale=True))
    ws = ctx.workspace(fc.load().fhe_mul_relin_workspace(ctx.handle, 2))
    out = torch.empty(2, 2, level - 1, 1 << log_n, dtype=torch.int64, device=a.device)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.mul_relin(a, b, kb, ka, rescale=True, workspace=ws, out=out)
        out.zero_()
        g.launch()
        g.launch()
    stream.synchronize()
    assert (fc.to_host(out) == eager).all()


def test_level_arguments_are_validated(fc):
    """level == 0 and level > L: FHE_EINVAL from the C entry points, nothing launched."""
    from fhecore.context import _ptr

    ctx = ctx_for(fc, 10, 5, 2, 3)
    lib = fc.load()
    t = ctx.empty(2, 5, 1 << 10)
    for level in (0, 6):
        assert lib.fhe_keyswitch_level(ctx.handle, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t),
                                       level, 1, None, None) == -1
        assert lib.fhe_mul_relin_level(ctx.handle, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t),
                                       level, 1, 0, None, None) == -1
        assert lib.fhe_rotate_level(ctx.handle, _ptr(t), _ptr(t), 5, _ptr(t), _ptr(t), level, 1,
                                    None, None) == -1
        assert b"level" in lib.fhe_last_error()
