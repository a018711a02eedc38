"""GPU parity for the level-aware plaintext arithmetic (fhe_lincomb_level, fhe_mul_plain_level;
include/fhecore.h) against pyoracle's lincomb / mul_plain, bit for bit: every output level, mixed
input levels, 1 .. 16 terms, the constant, the fused rescale, the worst-case accumulation on 60-,
61- and 62-bit chains, aliasing, graph capture, a decryption under real keys, and fhecore.polyeval's Chebyshev
evaluation on the GPU backend against the CPU backend's bits."""
import ctypes
import random

import numpy as np
import pytest

import cases
import coracle
import pyoracle
from refs import c_ntt

pytestmark = pytest.mark.gpu
CHEB = cases.CHEB


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
        m = fc.gen_moduli(log_n, L + K, bits=bits)
        _CTX[key] = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    return _CTX[key]


def u64(x):
    return np.asarray(x).astype(np.uint64)


# (log_n, L, K, dnum, bits): the 128-bit accumulation below 2^60 and below 2^61, the exact
# per-term path of a wide (62-bit) chain, and a second N
CONTEXTS = [(10, 5, 2, 3, 60), (10, 5, 2, 3, 61), (10, 5, 2, 3, 62), (11, 4, 2, 2, 60)]
COUNTS = (1, 2, 5, 16)


def in_level(t, count, level, L):
    """Term 0 at the output level (at level + 2 when it is the only term), the others cycling
    through level, level + 1, level + 2: strides that differ from the output's."""
    return min(L, level + (2 if count == 1 else t % 3))


@pytest.mark.parametrize("log_n,L,K,dnum,bits", CONTEXTS)
def test_lincomb_every_level(fc, log_n, L, K, dnum, bits):
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    n = 1 << log_n
    d = fc.to_device
    rng = random.Random(7)
    ks = [rng.randrange(-(1 << 200), 1 << 200) for _ in range(16)]
    k0 = rng.randrange(-(1 << 200), 1 << 200)
    pool = [rand(qs, log_n, (3, 2), seed=100 + t) for t in range(16)]  # [3][2][L][N] each
    tabs = {c: ctx.encode_scalars(ks[:c] + [k0], exact=True) for c in COUNTS}
    assert all(tuple(t.shape) == (c + 1, L) for c, t in tabs.items())  # scalar_stride == L
    for level in range(1, L + 1):
        ql = qs[:level]
        # the exact sums after 1 .. 16 terms, per ciphertext of the batch (shared by every case)
        run = [np.zeros((2, level, n), dtype=object) for _ in range(3)]
        sums = {}
        for t in range(16):
            for b in range(3):
                run[b] = pyoracle.lincomb([run[b], pool[t][b]], [1, ks[t]], qs, level=level)
            if t + 1 in COUNTS:
                sums[t + 1] = [r.copy() for r in run]
        refs = {}

        def want(count, const, rescale, b):  # once per case, shared by both batch sizes
            key = (count, const, rescale, b)
            if key not in refs:
                if rescale:
                    refs[key] = u64(pyoracle.rescale_ct(want(count, const, False, b), ql, c_ntt()))
                else:
                    refs[key] = u64(pyoracle.lincomb([sums[count][b]], [1], qs, level=level,
                                                     const=k0 if const else None))
            return refs[key]

        for count in COUNTS:
            lvs = [in_level(t, count, level, L) for t in range(count)]
            assert level == L or (max(lvs) > level and (count == 1 or min(lvs) == level))
            for batch in (1, 3):
                cts = [d(np.ascontiguousarray(pool[t][:batch, :, :lvs[t]])) for t in range(count)]
                for const in (False, True):
                    for rescale in (False, True):
                        if rescale and level < 2:
                            with pytest.raises(fc.FheError):
                                ctx.lincomb(cts, tabs[count], const=const, rescale=True, level=level)
                            continue
                        got = fc.to_host(ctx.lincomb(cts, tabs[count], const=const,
                                                     rescale=rescale, level=level))
                        assert got.shape == (batch, 2, level - (1 if rescale else 0), n)
                        for b in range(batch):
                            assert (got[b] == want(count, const, rescale, b)).all(), \
                                (level, count, batch, const, rescale, b)


@pytest.mark.parametrize("bits", [60, 61, 62])
def test_worst_case_accumulation(fc, bits):
    """16 terms, every input element, every scalar and the constant q_j - 1: the largest 128-bit
    sum the narrow path can meet (16 (q - 1)^2 + q - 1) and 16 conditional subtractions on the wide
    one.  (q - 1)^2 = 1 mod q: 16 - 1 = 15 on c0 and 16 on c1.  Then scalars 0 and 1 alternating."""
    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    n = 1 << log_n
    top = np.stack([np.full((2, 2, n), q - 1, dtype=np.uint64) for q in qs], axis=2)  # [2][2][L][N]
    cts = [fc.to_device(top) for _ in range(16)]
    got = fc.to_host(ctx.lincomb(cts, ctx.encode_scalars([-1] * 17, exact=True), const=True))
    assert (got[:, 0] == 15).all() and (got[:, 1] == 16).all()
    want = pyoracle.lincomb([top[0]] * 16, [-1] * 16, qs, level=L, const=-1)
    assert (got[0] == u64(want)).all() and (got[1] == u64(want)).all()
    want_r = pyoracle.rescale_ct(want, qs, c_ntt())
    got_r = fc.to_host(ctx.lincomb(cts, ctx.encode_scalars([-1] * 17, exact=True), const=True,
                                   rescale=True))
    assert (got_r[0] == u64(want_r)).all() and (got_r[1] == u64(want_r)).all()
    bits01 = [t % 2 for t in range(16)]
    got = fc.to_host(ctx.lincomb(cts, ctx.encode_scalars(bits01 + [0], exact=True), const=True))
    want = pyoracle.lincomb([top[0]] * 16, bits01, qs, level=L, const=0)
    assert (got[0] == u64(want)).all() and (got[1] == u64(want)).all()
    for j, q in enumerate(qs):  # eight times q - 1
        assert (got[:, :, j] == (8 * (q - 1)) % q).all()


@pytest.mark.parametrize("log_n,L,K,dnum,bits", [CONTEXTS[0], CONTEXTS[2]])
def test_drop_level_is_the_slice(fc, log_n, L, K, dnum, bits):
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    h = rand(ctx.moduli, log_n, (3, 2), seed=5)
    x = fc.to_device(h)
    for level in range(1, L + 1):
        got = fc.to_host(ctx.drop_level(x, level))
        assert got.shape == (3, 2, level, 1 << log_n)
        assert (got == h[:, :, :level]).all(), level
    assert (fc.to_host(ctx.drop_level(fc.to_device(h[0]), 2)) == h[0, :, :2]).all()  # no batch axis


@pytest.mark.parametrize("log_n,L,K,dnum,bits", CONTEXTS)
def test_mul_plain_every_level(fc, log_n, L, K, dnum, bits):
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    n = 1 << log_n
    d = fc.to_device
    batch = 3
    pt_top = rand(ctx.all_moduli, log_n, (batch,), seed=21)  # [batch][L + K][N]
    for level in range(1, L + 1):
        ct = rand(qs[:level], log_n, (batch, 2), seed=30 + level)
        dct = d(ct)
        for rows in sorted({level, L, L + K}):
            for pt_batch in (1, batch):
                pt = np.ascontiguousarray(pt_top[:pt_batch, :rows])
                dpt = d(pt[0] if pt_batch == 1 else pt)
                # the composition: vec mul on both components, then the rescale
                exp = np.ascontiguousarray(np.broadcast_to(pt[:, None, :level],
                                                           (pt_batch, 2, level, n)))
                exp = np.ascontiguousarray(np.broadcast_to(exp, (batch, 2, level, n)))
                prod = ctx.vec("mul", dct, d(exp))
                for rescale in (False, True):
                    if rescale and level < 2:
                        with pytest.raises(fc.FheError):
                            ctx.mul_plain(dct, dpt, rescale=True)
                        continue
                    got = fc.to_host(ctx.mul_plain(dct, dpt, rescale=rescale))
                    want = fc.to_host(ctx.rescale(prod) if rescale else prod)
                    assert got.shape == want.shape
                    assert (got == want).all(), (level, rows, pt_batch, rescale)
                    if rows == L:  # and the reference itself
                        for b in range(batch):
                            ref = pyoracle.mul_plain(ct[b], pt[b % pt_batch], qs, level=level,
                                                     rescale=rescale, ntt=c_ntt())
                            assert (got[b] == u64(ref)).all(), (level, pt_batch, rescale, b)
    # in place without rescale
    ct = d(rand(qs[:2], log_n, (batch, 2), seed=40))
    want = fc.to_host(ctx.mul_plain(ct, d(pt_top[0])))
    assert ctx.mul_plain(ct, d(pt_top[0]), out=ct).data_ptr() == ct.data_ptr()
    assert (fc.to_host(ct) == want).all()


def test_aliasing(fc):
    import torch

    log_n, L, K, dnum, level = 10, 5, 2, 3, 3
    n = 1 << log_n
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs = ctx.moduli
    d = fc.to_device
    ha, hb = rand(qs[:level], log_n, (2, 2), seed=51), rand(qs[:level + 1], log_n, (2, 2), seed=52)
    tab = ctx.encode_scalars([3, -5, 7], exact=True)
    want = fc.to_host(ctx.lincomb([d(ha), d(hb)], tab, const=True))
    a, b = d(ha), d(hb)
    got = ctx.lincomb([a, b], tab, const=True, out=a)  # in place on the term at the output level
    assert got.data_ptr() == a.data_ptr() and (fc.to_host(a) == want).all()
    # out on the start of the higher term (another stride): refused, nothing written
    view = b.view(-1)[:2 * 2 * level * n].view(2, 2, level, n)
    a = d(ha)
    with pytest.raises(fc.FheError):
        ctx.lincomb([a, b], tab, const=True, out=view)
    assert (fc.to_host(b) == hb).all()
    # with rescale every overlap is refused, the input itself included
    out = a.view(-1)[:2 * 2 * (level - 1) * n].view(2, 2, level - 1, n)
    with pytest.raises(fc.FheError):
        ctx.lincomb([a, b], tab, const=True, rescale=True, out=out)
    with pytest.raises(fc.FheError):
        ctx.mul_plain(a, d(rand(qs, log_n, seed=53)), rescale=True, out=out)
    torch.cuda.synchronize()
    assert (fc.to_host(a) == ha).all()


def test_arguments_are_validated(fc):
    from fhecore.context import _ptr

    ctx = ctx_for(fc, 10, 5, 2, 3)
    lib = fc.load()
    n = 1 << 10
    t = ctx.empty(2, 5, n)
    o = ctx.empty(2, 5, n)
    sc = ctx.encode_scalars([1, 1], exact=True)

    def lincomb(cts, lvs, stride, level, count, rescale=0):
        c_arr = (ctypes.c_void_p * max(len(cts), 1))(*cts)
        l_arr = (ctypes.c_uint32 * max(len(lvs), 1))(*lvs)
        return lib.fhe_lincomb_level(ctx.handle, _ptr(o), c_arr, l_arr, _ptr(sc), stride, 0, level,
                                     count, 1, rescale, None, None)

    p = t.data_ptr()
    assert lincomb([p], [5], 5, 0, 1) == -1 and b"level" in lib.fhe_last_error()
    assert lincomb([p], [5], 5, 6, 1) == -1
    assert lincomb([p], [2], 5, 3, 1) == -1 and b"in_levels" in lib.fhe_last_error()
    assert lincomb([p], [6], 5, 3, 1) == -1
    assert lincomb([], [], 5, 3, 0) == -1 and b"count" in lib.fhe_last_error()
    assert lincomb([p] * 17, [5] * 17, 5, 3, 17) == -1
    assert lincomb([p], [5], 2, 3, 1) == -1 and b"scalar_stride" in lib.fhe_last_error()
    assert lincomb([None], [5], 5, 3, 1) == -1 and b"null" in lib.fhe_last_error()
    assert lincomb([p], [5], 5, 1, 1, rescale=1) == -1 and b"rescale" in lib.fhe_last_error()
    assert lincomb([p], [5], 5, 3, 1) == 0

    def mul_plain(rows, pt_batch, level, rescale=0, pt=t):
        return lib.fhe_mul_plain_level(ctx.handle, _ptr(o), _ptr(t), _ptr(pt), rows, pt_batch, level,
                                       1, rescale, None, None)

    assert mul_plain(5, 1, 0) == -1 and mul_plain(5, 1, 6) == -1
    assert mul_plain(2, 1, 3) == -1 and b"pt_rows" in lib.fhe_last_error()
    assert mul_plain(5, 2, 3) == -1 and b"pt_batch" in lib.fhe_last_error()
    assert mul_plain(5, 1, 1, rescale=1) == -1
    assert mul_plain(5, 1, 3, pt=None) == -1 and b"null" in lib.fhe_last_error()


def test_graph_replay(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum, level = 11, 4, 2, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum)
    qs = ctx.moduli
    d = fc.to_device
    a, b = d(rand(qs[:level], log_n, (2, 2), seed=61)), d(rand(qs, log_n, (2, 2), seed=62))
    tab = ctx.encode_scalars([11, -13, 17], exact=True)
    eager = fc.to_host(ctx.lincomb([a, b], tab, const=True, rescale=True))
    lib = fc.load()
    ws = ctx.workspace(lib.fhe_lincomb_workspace(ctx.handle, 2))
    out = torch.empty(2, 2, level - 1, 1 << log_n, dtype=torch.int64, device=a.device)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.lincomb([a, b], tab, const=True, rescale=True, workspace=ws, out=out)
        out.zero_()
        g.launch()
        g.launch()
    stream.synchronize()
    assert (fc.to_host(out) == eager).all()
    # the internal workspace is refused while capturing (at the C ABI, as test_gpu_pipeline.py)
    c_arr = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    l_arr = (ctypes.c_uint32 * 2)(level, L)
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(sp) == 0
        rc = lib.fhe_lincomb_level(ctx.handle, _ptr(out), c_arr, l_arr, _ptr(tab), L, 1, level, 2, 2,
                                   1, None, sp)
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(sp, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    assert rc != 0 and "capturing" in lib.fhe_last_error().decode()
    # and through the Python layer, which hands workspace=None down as it is
    with torch.cuda.stream(stream):
        with pytest.raises(fc.FheError):
            with fc.Graph():
                ctx.lincomb([a, b], tab, const=True, rescale=True, out=out)
    stream.synchronize()


def cheb_ctx(fc):
    return ctx_for(fc, CHEB.log_n, CHEB.L, CHEB.nspecial, CHEB.dnum, CHEB.bits)


def test_decrypts_correctly_under_real_keys(fc):
    """rescale(k_1 ct_1 + k_2 ct_2 + k_0) under ctx.keygen_secret / encrypt_sk decrypts to
    k_1 z_1 + k_2 z_2 + k_0 within 16x the encoder's round-trip error at the inputs' scale.
    Inputs at delta = 2^40, scalars at 2^60 (the constant at 2^100) on the 50-bit chain, so the
    result sits at scale ~2^50 and the fused rescale's rounding (e_0 + e_1 s, sigma ~ sqrt(N / 18)
    coefficient units at the OUTPUT scale) is 2^-10 of the inputs' own precision.  What remains is
    the encryption error, sigma 3.24 per coefficient (centred binomial, eta = 21) against the
    encoder's rounding sigma 0.29: a ratio of 11.2 sqrt(k_1^2 + k_2^2) = 10.1 plus the input
    rounding itself -- CPU restatement of this run (pyoracle.encrypt_sk, pyoracle.lincomb): 9.8x.
    Public-key encryption (error e u + e_0 + e_1 s, ~400x) could not meet the bound."""
    from fhecore.ckks import Encoder, from_rns, to_rns

    ctx = cheb_ctx(fc)
    qs, n, L = ctx.moduli, ctx.n, ctx.L
    enc = Encoder(n)
    rng = np.random.default_rng(3)
    dc, ds = 2.0 ** 40, 2 ** 60
    z = [rng.uniform(-1, 1, n // 2) + 1j * rng.uniform(-1, 1, n // 2) for _ in range(2)]
    rt = max(np.abs(enc.decode(enc.encode(v, dc), dc) - v).max() for v in z)
    sk = ctx.keygen_secret(seed=11)
    cts = [ctx.encrypt_sk(fc.to_device(coracle.ntt_fwd(to_rns(enc.encode(v, dc), qs), qs)), sk,
                          seed=100 + i) for i, v in enumerate(z)]
    k1, k2, k0 = 0.75, -0.5, 0.3
    tab = fc.to_device(np.concatenate([fc.to_host(ctx.encode_scalars([k1, k2], delta=ds)),
                                       fc.to_host(ctx.encode_scalars([k0], delta=int(dc) * ds))]))
    for level in (L, 3):
        ins = [cts[0], ctx.drop_level(cts[1], max(level, L - 1))]  # mixed input levels
        out = ctx.lincomb(ins, tab, const=True, rescale=True, level=level)
        ql = qs[:level - 1]
        dec = coracle.ntt_inv(fc.to_host(ctx.decrypt(out, sk)), ql)
        got = enc.decode(from_rns(dec, ql), dc * ds / qs[level - 1])
        err = np.abs(got - (k1 * z[0] + k2 * z[1] + k0)).max()
        print(f"level {level}: round trip {rt:.3e}, error {err:.3e}, ratio {err / rt:.2f}")
        assert err < 16 * rt, (level, err, rt)


def _gpu_cheb(fc, degree):
    from fhecore import polyeval

    su = cases.setup(CHEB)
    ctx = cheb_ctx(fc)
    assert ctx.moduli == su["qs"] and ctx.special == su["ps"]
    key = (fc.to_device(u64(su["relin"][0])), fc.to_device(u64(su["relin"][1])))
    be = polyeval.GpuBackend(ctx, key)
    ct = polyeval.Ct(fc.to_device(u64(su["ct"])), CHEB.L, CHEB.delta)
    c = cases.cheb_coeffs(degree)
    return polyeval.chebyshev_eval(be, ct, c), c


def test_chebyshev_eval_matches_the_cpu_backend_bit_for_bit(fc):
    """The degree-7 run of tests/test_plain_cpu.py with the same seeds: both backends receive the
    same integer scalars, so the final ciphertext is the same bits."""
    out, _ = _gpu_cheb(fc, 7)
    ref, err = cases.run_cpu(CHEB, 7)
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (fc.to_host(out.data) == u64(ref.data)).all()
    assert err < 4 * cases.CHEB_ERR_DEG7


def test_chebyshev_eval_degree_15(fc):
    """Degree 15 (m = 4, giants T_4, T_8; five levels) against chebval alone.  The CPU backend
    measured 2.03e-12 for this run, below the degree-7 figure, so the bound stays 4x that one."""
    out, c = _gpu_cheb(fc, 15)
    assert out.level == CHEB.L - 5
    su = cases.setup(CHEB)
    got = cases.decrypt_decode(CHEB, fc.to_host(out.data), out.level, out.scale)
    err = np.abs(got - np.polynomial.chebyshev.chebval(su["x"], c)).max()
    print(f"degree 15: max slot error {err:.3e}")
    assert err < 4 * cases.CHEB_ERR_DEG7
