"""GPU parity for ModRaise (fhe_mod_raise; include/fhecore.h) against pyoracle.mod_raise, bit for
bit: 60-, 61- and 62-bit chains (the last takes the unfused path of wide contexts), a second N, a
60-bit q_0 over 50-bit primes, both workgroup placements, strided inputs, every boundary of the
centring, the refusals, graph capture, the m + q_0 I identity under real keys on the device, and
the composition tools/modraise_times.py times it against."""
import ctypes
import os
import sys

import numpy as np
import pytest

import coracle
import pyoracle
import refs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


_CTX = {}


def ctx_for(fc, log_n, L, K, dnum, bits):
    """bits = "mixed": a 60-bit q_0 over 50-bit primes (q_l < q_0 / 2: the lift must reduce)."""
    key = (log_n, L, K, dnum, bits)
    if key not in _CTX:
        if bits == "mixed":
            m = fc.gen_moduli(log_n, 1, bits=60) + fc.gen_moduli(log_n, L - 1 + K, bits=50)
        else:
            m = fc.gen_moduli(log_n, L + K, bits=bits)
        _CTX[key] = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    return _CTX[key]


def u64(x):
    return np.asarray(x).astype(np.uint64)


CONTEXTS = [(10, 5, 2, 3, 60), (10, 5, 2, 3, 61), (10, 5, 2, 3, 62), (11, 4, 2, 2, 60),
            (10, 5, 2, 3, "mixed")]


def boundary_input(qs, log_n, batch, seed):
    """[batch][2][L][N], canonical residues.  Limb 0 is the forward NTT of a coefficient polynomial
    whose entries cycle through 0, 1, h, h + 1, q_0 - 1 (h = (q_0 - 1) / 2), starting at another
    point of the cycle in every polynomial -- both sides of the centring in every tile -- with
    uniform coefficients in the second half of the odd polynomials; the other limbs are uniform
    (mod_raise must not read them)."""
    n = 1 << log_n
    q0 = int(qs[0])
    h = (q0 - 1) // 2
    vals = np.array([0, 1, h, h + 1, q0 - 1], dtype=np.uint64)
    rng = np.random.default_rng(seed)
    x = np.stack([vals[(np.arange(n) + p) % 5] for p in range(2 * batch)])
    x[1::2, n // 2:] = rng.integers(0, q0, (batch, n // 2), dtype=np.uint64)
    limb0 = coracle.ntt_fwd(x[:, None, :], [q0])
    rest = np.stack([rng.integers(0, int(q), (2 * batch, n), dtype=np.uint64) for q in qs[1:]], axis=1)
    return np.concatenate([limb0, rest], axis=1).reshape(batch, 2, len(qs), n)


@pytest.mark.parametrize("log_n,L,K,dnum,bits", CONTEXTS)
def test_mod_raise_matches_the_reference(fc, log_n, L, K, dnum, bits):
    """Batches 1, 3 (limbs-fastest placement) and 4 (polys = 8: the XCD placement), in_level 1 and
    L (a strided read of limb 0), out_level 1, 2 and L.  One reference for the context: limb l of
    the result depends on limb 0 of the input alone, so out_level l is the first l limbs of it."""
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    if bits == "mixed":
        assert all(q < qs[0] // 2 for q in qs[1:])
    n = 1 << log_n
    full = boundary_input(qs, log_n, 4, seed=41)
    want = u64(pyoracle.mod_raise(full[:, :, :1], qs, 1, L, ntt=refs.c_ntt()))  # [4][2][L][N]
    assert (want[:, :, 0] == full[:, :, 0]).all()
    for batch in (1, 3, 4):
        for in_level in (1, L):
            src = np.ascontiguousarray(full[:batch, :, :in_level])
            x = fc.to_device(src)
            for out_level in (1, 2, L):
                got = fc.to_host(ctx.mod_raise(x, out_level))
                assert got.shape == (batch, 2, out_level, n)
                assert (got == want[:batch, :, :out_level]).all(), (batch, in_level, out_level)
            assert (fc.to_host(x) == src).all()  # the input is read only
    # level defaults to L; no batch axis; a caller's out
    x = fc.to_device(np.ascontiguousarray(full[1, :, :2]))
    assert (fc.to_host(ctx.mod_raise(x)) == want[1]).all()
    out = ctx.empty(2, 3, n)
    assert ctx.mod_raise(x, 3, out=out).data_ptr() == out.data_ptr()
    assert (fc.to_host(out) == want[1, :, :3]).all()


def test_errors_write_nothing(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    n = 1 << log_n
    lib = fc.load()
    src = boundary_input(ctx.moduli, log_n, 2, seed=43)
    x = fc.to_device(src)
    poison = 0x5A5A5A5A5A5A5A5
    out = torch.full((2, 2, L + 1, n), poison, dtype=torch.int64, device=x.device)
    ws = ctx.workspace(lib.fhe_mod_raise_workspace(ctx.handle, 2))
    assert lib.fhe_mod_raise_workspace(ctx.handle, 2) == 2 * 2 * n * 8
    # bad output levels through the Python layer
    for level in (0, L + 1):
        with pytest.raises(fc.FheError, match="level"):
            ctx.mod_raise(x, level, out=out.view(-1)[:2 * 2 * level * n].view(2, 2, level, n))

    def raw(o, i, in_level, out_level, batch=2, w=ws):
        return lib.fhe_mod_raise(ctx.handle, o, i, in_level, out_level, batch, _ptr(w), None)

    # bad input levels and null pointers at the C ABI
    assert raw(_ptr(out), _ptr(x), 0, L) == -1 and b"level" in lib.fhe_last_error()
    assert raw(_ptr(out), _ptr(x), L + 1, L) == -1
    assert raw(None, _ptr(x), L, L) == -1 and b"null" in lib.fhe_last_error()
    assert raw(_ptr(out), None, L, L) == -1
    # any overlap of out with in: the input itself, and out starting inside / before the input
    with pytest.raises(fc.FheError, match="overlaps"):
        ctx.mod_raise(x, L, out=x)
    tail = x.view(-1)[2 * 2 * L * n - 2 * 2 * n:].view(2, 2, 1, n)  # the last words of the input
    with pytest.raises(fc.FheError, match="overlaps"):
        ctx.mod_raise(x, 1, out=tail)
    both = torch.full((2 * 2 * 2 * L * n,), poison, dtype=torch.int64, device=x.device)
    late = both[2 * 2 * L * n - n:][:2 * 2 * L * n].view(2, 2, L, n)  # in: starts inside out's span
    with pytest.raises(fc.FheError, match="overlaps"):
        ctx.mod_raise(late, L, out=both[:2 * 2 * L * n].view(2, 2, L, n))
    # batch 0 is a no-op
    assert raw(_ptr(out), _ptr(x), L, L, batch=0) == 0
    torch.cuda.synchronize()
    assert (out == poison).all() and (both == poison).all()
    assert (fc.to_host(x) == src).all()


def test_graph_replay(fc):
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum = 11, 4, 2, 2
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    qs = ctx.moduli
    n = 1 << log_n
    lib = fc.load()
    ins = [boundary_input(qs, log_n, 2, seed=s)[:, :, :2].copy() for s in (47, 48)]
    wants = [u64(pyoracle.mod_raise(h, qs, 2, L, ntt=refs.c_ntt())) for h in ins]
    x = fc.to_device(ins[0])
    ws = ctx.workspace(lib.fhe_mod_raise_workspace(ctx.handle, 2))
    out = torch.zeros(2, 2, L, n, dtype=torch.int64, device=x.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.mod_raise(x, L, workspace=ws, out=out)
        g.launch()
        stream.synchronize()
        assert (fc.to_host(out) == wants[0]).all()
        x.copy_(fc.to_device(ins[1]))  # the captured pointers, new input
        out.zero_()
        g.launch()
        stream.synchronize()
        assert (fc.to_host(out) == wants[1]).all()
    # the internal workspace is refused while capturing (at the C ABI, as test_gpu_pipeline.py),
    # and the capture still ends cleanly
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(sp) == 0
        rc = lib.fhe_mod_raise(ctx.handle, _ptr(out), _ptr(x), 2, L, 2, None, sp)
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(sp, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    assert rc == -1 and "capturing" in lib.fhe_last_error().decode()
    # and through the Python layer, which hands workspace=None down as it is
    with torch.cuda.stream(stream):
        with pytest.raises(fc.FheError):
            with fc.Graph():
                ctx.mod_raise(x, L, out=out)
    stream.synchronize()
    assert (fc.to_host(out) == wants[1]).all()  # nothing was launched
    # the stream is out of capture: an eager call on it runs
    with torch.cuda.stream(stream):
        x.copy_(fc.to_device(ins[0]))
        ctx.mod_raise(x, L, out=out)
    stream.synchronize()
    assert (fc.to_host(out) == wants[0]).all()


@pytest.mark.parametrize("bits", [60, "mixed"])
def test_raised_ciphertext_decrypts_to_m_plus_q0_I(fc, bits):
    """keygen_secret, encrypt_sk, drop_level to 1, mod_raise to L, decrypt: the CRT-centred
    coefficients y satisfy y = m_1 (mod q_0) exactly (m_1 the centred level-1 decryption) and
    |(y - m_1) / q_0| <= (||s||_1 + 2) / 2, ||s||_1 counted from the secret itself (the bound is
    derived in tests/test_modraise_cpu.py)."""
    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, bits)
    qs, n = ctx.moduli, ctx.n
    q0 = qs[0]
    sk = ctx.keygen_secret(seed=5)
    s = coracle.ntt_inv(fc.to_host(sk)[:1], qs[:1])[0].astype(object)
    assert all(v in (0, 1, q0 - 1) for v in s)
    s1 = int(sum(1 for v in s if v))
    assert n // 2 < s1 < n
    rng = np.random.default_rng(9)
    m = rng.integers(-(1 << 40), 1 << 40, n).astype(object)
    pt = coracle.ntt_fwd(u64(pyoracle._to_rns(m, qs)), qs)
    ct = ctx.encrypt_sk(fc.to_device(pt), sk, seed=13)
    low = ctx.drop_level(ct, 1)
    d1 = coracle.ntt_inv(fc.to_host(ctx.decrypt(low, sk)), qs[:1])[0].astype(object)
    m1 = np.where(d1 > (q0 - 1) // 2, d1 - q0, d1)
    assert abs(m1 - m).max() <= 21  # the encryption error (centred binomial, eta = 21)
    up = ctx.mod_raise(low, L)
    assert (fc.to_host(up)[:, 0] == fc.to_host(ct)[:, 0]).all()
    y = pyoracle.crt_centered(coracle.ntt_inv(fc.to_host(ctx.decrypt(up, sk)), qs), qs)
    assert ((y - m1) % q0 == 0).all()
    big_i = (y - m1) // q0
    print(f"{bits}: max |I| = {abs(big_i).max()}, bound {(s1 + 2) / 2}")
    assert (abs(big_i) <= (s1 + 2) / 2).all()


def test_equals_the_composition_of_public_calls(fc):
    """ctx.intt of limb 0, a torch centred lift, ctx.ntt over the limbs: the form
    tools/modraise_times.py times mod_raise against."""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import modraise_times

    log_n, L, K, dnum = 10, 5, 2, 3
    ctx = ctx_for(fc, log_n, L, K, dnum, 60)
    x = fc.to_device(boundary_input(ctx.moduli, log_n, 3, seed=53))
    for level in (L, 2):
        got = ctx.mod_raise(x, level)
        want = modraise_times.composed_mod_raise(ctx, x, level)
        assert got.shape == want.shape and (got == want).all(), level
