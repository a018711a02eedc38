"""GPU parity for the sum of ciphertext products with one relinearisation
(fhe_mul_sum_relin_level; include/fhecore.h) against pyoracle.mul_sum_relin, bit for bit: every count
that fills, overflows or underfills a term group, every level of contexts on each key-switch path
(fused lz16, alpha = 4, unfused dnum > 4, a 61-bit chain, a wide 62-bit chain), mixed input levels,
aliased operands, the accumulators at their bound, both workspaces, a captured graph, every
refusal, one full-size call across a pass boundary, and the shared decrypt case."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import cases
import pyoracle
import refs

MS = cases.MULSUM

pytestmark = pytest.mark.gpu


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


def ws_bytes(fc, ctx, batch):
    lib = fc.load()
    return lib.fhe_mul_relin_workspace(ctx.handle, lib.fhe_keyswitch_pass_batch(ctx.handle, batch))


# (log_n, L, K, dnum, bits): the fused lz16 path with a partial last digit; alpha = 4; dnum > 4
# (unfused kernels); a 61-bit chain (narrow accumulation at its widest); a 62-bit one (wide)
CONTEXTS = [(10, 5, 2, 3, 60), (11, 7, 4, 2, 60), (10, 6, 2, 6, 60), (10, 5, 2, 3, 61),
            (10, 5, 2, 3, 62)]
POOL, BATCH = 8, 3
_WORLD = {}


def world(fc, key):
    """Per context: a uniform key and a pool of POOL uniform top-level operands [BATCH, 2, L, N],
    on the host and on the device (once per process)."""
    if key not in _WORLD:
        log_n, L, K, dnum, bits = key
        ctx = ctx_for(fc, *key)
        kb = rand(ctx.all_moduli, log_n, (dnum,), seed=3)
        ka = rand(ctx.all_moduli, log_n, (dnum,), seed=4)
        pool = [rand(ctx.moduli, log_n, (BATCH, 2), seed=100 + i) for i in range(POOL)]
        d = fc.to_device
        _WORLD[key] = dict(ctx=ctx, qs=ctx.moduli, ps=ctx.all_moduli[L:], dnum=dnum, L=L, n=1 << log_n,
                           kb=kb, ka=ka, dkb=d(kb), dka=d(ka), pool=pool, dpool=[d(p) for p in pool])
    return _WORLD[key]


def reference(w, As, Bs, level, batch=None):
    """[(plain, rescaled or None)] per ciphertext of the batch: As[i], Bs[i] host [BATCH, 2, l, N]."""
    out = []
    for c in range(batch or As[0].shape[0]):
        r = pyoracle.mul_sum_relin([a[c] for a in As], [b[c] for b in Bs], w["kb"], w["ka"], w["qs"],
                                   w["ps"], w["dnum"], False, level=level, ntt=refs.c_ntt())
        out.append((r, pyoracle.rescale_ct(r, w["qs"][:level], refs.c_ntt()) if level >= 2 else None))
    return out


def same(got, want, what):
    assert got.shape[1:] == want[0].shape, what
    for c in range(got.shape[0]):
        assert (got[c].astype(object) == want[c]).all(), (what, c)


def terms(w, count, level):
    """count terms over the pool with mixed input levels: even terms a_i at L and b_i cut to
    `level`, odd terms the other way round.  -> (host As, host Bs, device As, device Bs)."""
    As, Bs, dAs, dBs = [], [], [], []
    for i in range(count):
        ia, ib = i % POOL, (3 * i + 1) % POOL
        for idx, full, hl, dl in ((ia, i % 2 == 0, As, dAs), (ib, i % 2 == 1, Bs, dBs)):
            hl.append(w["pool"][idx] if full else w["pool"][idx][:, :, :level])
            dl.append(w["dpool"][idx] if full else w["dpool"][idx][:, :, :level].contiguous())
    return As, Bs, dAs, dBs


@pytest.mark.parametrize("count", [1, 2, 5, 16])
@pytest.mark.parametrize("key", CONTEXTS, ids=lambda k: "n%d_L%d_K%d_d%d_b%d" % k)
def test_every_level_count_and_batch(fc, key, count):
    """count 5 leaves a ragged last term group, 16 fills the argument arrays; batches 1 and 3;
    rescale on and off; every level of the first context and levels {1, 2, L} of the others; the
    wrapper's own workspace, then exactly the documented bytes followed by a guard."""
    w = world(fc, key)
    ctx, L = w["ctx"], w["L"]
    guarded = {b: Guarded(ws_bytes(fc, ctx, b)) for b in (1, BATCH)}
    for level in (range(1, L + 1) if key == CONTEXTS[0] else (1, 2, L)):
        As, Bs, dAs, dBs = terms(w, count, level)
        want = reference(w, As, Bs, level)
        for batch in (1, BATCH):
            da = [t[:batch].contiguous() for t in dAs]
            db = [t[:batch].contiguous() for t in dBs]
            for rescale in (False, True):
                if rescale and level < 2:
                    with pytest.raises(fc.FheError):  # FHE_EINVAL: nothing to rescale into
                        ctx.mul_sum_relin(da, db, w["dkb"], w["dka"], rescale=True, level=level)
                    continue
                ref = [r[1 if rescale else 0] for r in want[:batch]]
                for ws in (None, guarded[batch]):
                    got = fc.to_host(ctx.mul_sum_relin(da, db, w["dkb"], w["dka"], rescale=rescale,
                                                       level=level,
                                                       workspace=None if ws is None else ws.buf))
                    assert got.shape == (batch, 2, level - (1 if rescale else 0), w["n"])
                    same(got, ref, (level, batch, rescale, ws is not None))
                    assert ws is None or ws.intact(), (level, batch, rescale)


@pytest.mark.parametrize("bits", [60, 62])
def test_squares_and_a_shared_operand(fc, bits):
    """Inputs may alias each other in any way: every term a square (a[i] is b[i], the same
    tensor), one operand shared by all terms on either side, and the default level (the lowest
    input's)."""
    w = world(fc, (10, 5, 2, 3, bits))
    ctx, level = w["ctx"], 3
    p, dp = w["pool"], w["dpool"]
    low, dlow = p[5][:, :, :level], dp[5][:, :, :level].contiguous()
    cases = {
        "squares": ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),
        "shared a": ([0] * 6, [1, 2, 3, 4, 0, 6]),
        "shared b": ([1, 2, 3], [7, 7, 7]),
    }
    for name, (ia, ib) in cases.items():
        As, Bs = [p[i] for i in ia] + [low], [p[i] for i in ib] + [low]
        dAs, dBs = [dp[i] for i in ia] + [dlow], [dp[i] for i in ib] + [dlow]
        want = reference(w, As, Bs, level)
        got = ctx.mul_sum_relin(dAs, dBs, w["dkb"], w["dka"])  # rescale, level = min = 3
        assert got.shape == (BATCH, 2, level - 1, w["n"])
        same(fc.to_host(got), [r[1] for r in want], name)


@pytest.mark.parametrize("key", CONTEXTS, ids=lambda k: "n%d_L%d_K%d_d%d_b%d" % k)
def test_one_term_is_mul_relin_bitwise(fc, key):
    w = world(fc, key)
    ctx, L = w["ctx"], w["L"]
    for level in (1, 2, L):
        a = w["dpool"][0][:, :, :level].contiguous()
        b = w["dpool"][1][:, :, :level].contiguous()
        for rescale in (False, True) if level >= 2 else (False,):
            got = ctx.mul_sum_relin([a], [b], w["dkb"], w["dka"], rescale=rescale)
            want = ctx.mul_relin(a, b, w["dkb"], w["dka"], rescale=rescale)
            assert (fc.to_host(got) == fc.to_host(want)).all(), (level, rescale)


@pytest.mark.parametrize("bits", [60, 61, 62])
def test_structured_inputs(fc, bits):
    """Every residue q_j - 1 in 16 terms: D_0 = D_2 = 16 (q - 1)^2 and D_1 = 32 (q - 1)^2 before
    reduction, each accumulator at the bound the kernel's narrow form relies on (32 q^2 < 2^127 for
    q < 2^61) and the wide form's per-term a0 b1 + a1 b0 < 2 q^2 at its own.  And inputs whose D_2
    is exactly 0 (every a_i's second polynomial zero): the key-switch of zero."""
    key = (10, 5, 2, 3, bits)
    w = world(fc, key)
    ctx, L, n = w["ctx"], w["L"], w["n"]
    d = fc.to_device
    top = np.stack([np.full((1, 2, n), q - 1, dtype=np.uint64) for q in w["qs"]], axis=2)
    assert top.shape == (1, 2, L, n)
    dtop = d(top)
    for level in (1, 2, L):
        want = reference(w, [top] * 16, [top] * 16, level)
        D = pyoracle.tensor_sum([top[0]] * 16, [top[0]] * 16, w["qs"], level=level)
        assert [int(D[k, 0, 0]) for k in range(3)] == [16, 32, 16]
        for rescale in (False, True) if level >= 2 else (False,):
            got = ctx.mul_sum_relin([dtop] * 16, [dtop] * 16, w["dkb"], w["dka"], rescale=rescale,
                                    level=level)
            same(fc.to_host(got), [r[1 if rescale else 0] for r in want], ("top", level, rescale))
    zero = [p.copy() for p in w["pool"][:5]]
    for z in zero:
        z[:, 1] = 0
    Bs = w["pool"][3:8]
    for level in (1, L):
        D = pyoracle.tensor_sum([z[0] for z in zero], [b[0] for b in Bs], w["qs"], level=level)
        assert not D[2].any() and D[0].any() and D[1].any()
        want = reference(w, zero, Bs, level)
        got = ctx.mul_sum_relin([d(z) for z in zero], w["dpool"][3:8], w["dkb"], w["dka"],
                                rescale=False, level=level)
        same(fc.to_host(got), [r[0] for r in want], ("D2 = 0", level))


def test_graph_replay_equals_eager(fc):
    import torch

    w = world(fc, CONTEXTS[0])
    ctx, level, batch = w["ctx"], 4, 2
    _, _, dAs, dBs = terms(w, 5, level)
    da = [t[:batch].contiguous() for t in dAs]
    db = [t[:batch].contiguous() for t in dBs]
    eager = fc.to_host(ctx.mul_sum_relin(da, db, w["dkb"], w["dka"], rescale=True, level=level))
    ws = ctx.workspace(ws_bytes(fc, ctx, batch))
    out = torch.empty(batch, 2, level - 1, w["n"], dtype=torch.int64, device=da[0].device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.mul_sum_relin(da, db, w["dkb"], w["dka"], rescale=True, level=level, workspace=ws,
                              out=out)
        for _ in range(2):
            out.zero_()
            g.launch()
            stream.synchronize()
            assert (fc.to_host(out) == eager).all()


def test_every_refusal_leaves_the_output_untouched(fc):
    """Each error of the list in include/fhecore.h returns FHE_EINVAL at the C ABI before any
    launch: the output keeps its fill pattern."""
    import torch
    from fhecore.context import _ptr

    w = world(fc, CONTEXTS[0])
    ctx, L, n = w["ctx"], w["L"], w["n"]
    lib = fc.load()
    level, batch = 3, 2
    a = [w["dpool"][i][:batch].contiguous() for i in range(2)]               # at L
    b = [w["dpool"][i][:batch, :, :level].contiguous() for i in range(2, 4)]  # at level
    # one buffer holding the output and, right behind it, an operand at `level`
    words = batch * 2 * level * n
    buf = torch.full((2 * words,), GUARD, dtype=torch.int64, device="cuda")
    out = buf[:words]
    behind = buf[words:].view(batch, 2, level, n)
    behind.copy_(b[1])
    ws = ctx.workspace(ws_bytes(fc, ctx, batch))
    kb, ka = w["dkb"], w["dka"]

    def arr(ts):
        return (ctypes.c_void_p * len(ts))(*[None if t is None else
                                             (t if isinstance(t, int) else t.data_ptr()) for t in ts])

    def lv(ls):
        return (ctypes.c_uint32 * len(ls))(*ls)

    def call(h=ctx.handle, o=out, A=a, la=(L, L), B=b, lb=(level, level), kb=kb, ka=ka,
             level=level, count=2, batch=batch, rescale=1, ws=ws, stream=None):
        return lib.fhe_mul_sum_relin_level(
            h, _ptr(o) if isinstance(o, torch.Tensor) else o, None if A is None else arr(A),
            None if la is None else lv(la), None if B is None else arr(B),
            None if lb is None else lv(lb), _ptr(kb), _ptr(ka), level, count, batch, rescale,
            _ptr(ws), stream)

    def untouched():
        torch.cuda.synchronize()
        return (out == GUARD).all().item()

    k0 = fc.Context(10, L=2)  # no special primes
    t0 = k0.empty(1, 2, 2, n)
    bad = {
        "K = 0": dict(h=k0.handle, A=[t0], la=(2,), B=[t0], lb=(2,), kb=t0, ka=t0, level=2, count=1,
                      batch=1, ws=None),
        "null out": dict(o=None),
        "null a": dict(A=None),
        "null a_levels": dict(la=None),
        "null b": dict(B=None),
        "null b_levels": dict(lb=None),
        "null evk_b": dict(kb=None),
        "null evk_a": dict(ka=None),
        "null inside a": dict(A=[a[0], None]),
        "null inside b": dict(B=[None, b[1]]),
        "count 0": dict(count=0),
        "count 17": dict(A=[a[0]] * 17, la=(L,) * 17, B=[a[1]] * 17, lb=(L,) * 17, count=17),
        "level 0": dict(level=0),
        "level above L": dict(level=L + 1),
        "an input below level": dict(lb=(level, level - 1)),
        "an input above L": dict(la=(L + 1, L)),
        "rescale at level 1": dict(level=1, rescale=1),
        "out is an input": dict(B=[b[0], behind], o=behind),
        "out overlaps an input": dict(B=[b[0], buf.data_ptr() + 8 * (words - n)], rescale=0),
        "the rescaled out overlaps an input": dict(B=[b[0], buf.data_ptr() + 8 * n]),
        "out overlaps an input at L": dict(A=[a[0], buf.data_ptr() + 8 * n], rescale=0),
    }
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        assert lib.fhe_last_error(), name
        assert untouched(), name
    assert (behind == b[1]).all().item()
    # batch == 0 is a no-op, whatever the other arguments point to
    assert call(batch=0) == 0 and untouched()
    # the internal workspace is refused while capturing, and the capture still ends cleanly
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(sp) == 0
        rc = call(ws=None, stream=sp)
        err = lib.fhe_last_error().decode()
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(sp, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    stream.synchronize()
    assert rc == -1 and "capturing" in err
    assert untouched()
    # the good call, for the record: the same arguments succeed
    assert call() == 0
    torch.cuda.synchronize()
    want = ctx.mul_sum_relin(a, b, kb, ka, rescale=True, level=level)
    assert (out[:batch * 2 * (level - 1) * n].view(batch, 2, level - 1, n) == want).all().item()


def test_full_size_call_across_a_pass(fc):
    """N = 2^16, L = 16, K = 4, dnum = 4, four terms over three operands, batch 33: a pass holds
    32 ciphertexts, so ciphertext 32 runs in the second pass, each term advanced by its own stride
    (one operand sits at level 16, the sum is taken at 15).  Ciphertexts 0 and 32 against the
    device's own composition: vec mul / add per tensor component, keyswitch, add, rescale."""
    import torch

    log_n, L, K, dnum, level, batch = 16, 16, 4, 4, 15, 33
    n = 1 << log_n
    ctx = ctx_for(fc, log_n, L, K, dnum)
    assert fc.load().fhe_keyswitch_pass_batch(ctx.handle, batch) == 32
    gen = torch.Generator(device="cuda").manual_seed(7)

    def uniform(mods, lead):
        return torch.stack([torch.randint(0, q, (*lead, n), generator=gen, device="cuda",
                                          dtype=torch.int64) for q in mods], dim=len(lead))

    kb, ka = uniform(ctx.all_moduli, (dnum,)), uniform(ctx.all_moduli, (dnum,))
    x = uniform(ctx.moduli, (batch, 2))            # level 16, read through its own stride
    y, z = (uniform(ctx.moduli[:level], (batch, 2)) for _ in range(2))
    As, Bs = [x, y, z, x], [y, z, x, x]
    got = ctx.mul_sum_relin(As, Bs, kb, ka, rescale=True, level=level)
    assert got.shape == (batch, 2, level - 1, n)
    pick = torch.tensor([0, 32], device="cuda")
    cut = lambda t: t[pick][:, :, :level].contiguous()  # noqa: E731
    D = None
    for a, b in zip(As, Bs):
        a, b = cut(a), cut(b)
        a0, a1, b0, b1 = (t.contiguous() for t in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
        d = [ctx.vec("mul", a0, b0),
             ctx.vec("add", ctx.vec("mul", a0, b1), ctx.vec("mul", a1, b0)),
             ctx.vec("mul", a1, b1)]
        D = d if D is None else [ctx.vec("add", s, t) for s, t in zip(D, d)]
    ks0, ks1 = ctx.keyswitch(D[2], kb, ka)
    ct = torch.stack([ctx.vec("add", D[0], ks0), ctx.vec("add", D[1], ks1)], dim=1).contiguous()
    want = ctx.rescale(ct)
    assert (got[pick] == want).all().item()


# ---- the shared decrypt case -----------------------------------------------------------------------

@pytest.mark.parametrize("count", cases.COUNTS)
def test_inner_product_decrypts(fc, count):
    """polyeval.inner_product on the GPU backend equals the CPU backend bit for bit, decrypts to
    numpy's sum_i z_i w_i with no more error than the composed form (mul_relin(rescale) per term,
    then the sum, evaluated here on the device), and within 1.5x of the recorded constant."""
    from fhecore import polyeval

    su = cases.setup(MS)
    ctx = ctx_for(fc, MS.log_n, MS.L, MS.nspecial, MS.dnum, MS.bits)
    assert ctx.moduli == su["qs"]
    d = fc.to_device
    be = polyeval.GpuBackend(ctx, tuple(d(np.asarray(k, dtype=np.uint64)) for k in su["relin"]))
    xs, ys = cases.mulsum_operands(count, wrap=d)
    out = polyeval.inner_product(be, xs, ys)
    cpu, cpu_err = cases.run_cpu(MS, count)
    assert out.level == cpu.level == MS.L - 1 and out.scale == cpu.scale
    host = fc.to_host(out.data)
    assert (host.astype(object) == cpu.data).all()
    err = cases.slot_error(MS, polyeval.Ct(host, out.level, out.scale), count)
    # the composed form on the device: one mul_relin(rescale) per term, then their sum
    acc = None
    for x, y in zip(xs, ys):
        p = be.mul_relin(x.data, y.data, True)
        acc = p if acc is None else ctx.vec("add", acc, p)
    composed = polyeval.Ct(fc.to_host(acc), MS.L - 1, Fraction(MS.delta) ** 2 / su["qs"][MS.L - 1])
    ref_err = cases.slot_error(MS, composed, count)
    print(f"count {count}: fused max slot error {err:.3e}, composed {ref_err:.3e} "
          f"(recorded {cases.FUSED_ERR[count]:.3e} / {cases.COMPOSED_ERR[count]:.3e})")
    assert err == cpu_err
    assert err <= ref_err
    assert err < 1.5 * cases.FUSED_ERR[count]
