"""GPU parity for batched encryption at any level (fhe_encrypt_level, fhe_encrypt_sk_level,
fhe_encrypt_slots; include/fhecore.h) against tests/encrypt_ref.py, bit for bit: 60- and 62-bit
chains (the last takes the unfused lift), a 60-bit q_0 over 50-bit primes, N = 2^13 (the two-pass
FFT and another column geometry); batches 1, 3 and 8 (both placements of the lift), levels 1, 2 and
L, index0 0 and 5, one plaintext for the batch, one per ciphertext and none; the three properties
against fhe_encrypt / fhe_encrypt_sk and drop_level; the slots form against encode then encrypt;
decryption under device-made keys; passes; the refusals; graph capture."""
import ctypes
import itertools

import numpy as np
import pytest

import encrypt_ref

pytestmark = pytest.mark.gpu

D50 = 2.0 ** 50
SEED = 0xC0FFEE_0123_4567
CONTEXTS = [(10, 4, 2, 2, 60), (10, 4, 2, 2, 62), (10, 4, 2, 2, "mixed"), (13, 3, 1, 1, 60)]


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


_CTX = {}


def setup_for(fc, log_n, L, K, dnum, bits):
    """(ctx, sk, pk, pts): device-made keys and 8 random plaintexts over all L + K limbs, once per
    context; each a (device tensor, host array) pair."""
    key = (log_n, L, K, dnum, bits)
    if key not in _CTX:
        if bits == "mixed":
            m = fc.gen_moduli(log_n, 1, bits=60) + fc.gen_moduli(log_n, L - 1 + K, bits=50)
        else:
            m = fc.gen_moduli(log_n, L + K, bits=bits)
        ctx = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
        sk = ctx.keygen_secret(seed=3)
        pk = ctx.keygen_public(sk, seed=4)
        rng = np.random.default_rng(log_n)
        pts = np.stack([np.stack([rng.integers(0, q, ctx.n, dtype=np.uint64)
                                  for q in ctx.all_moduli]) for _ in range(8)])
        _CTX[key] = (ctx, (sk, fc.to_host(sk)), (pk, fc.to_host(pk)), (fc.to_device(pts), pts))
    return _CTX[key]


@pytest.mark.parametrize("secret", [False, True])
@pytest.mark.parametrize("log_n,L,K,dnum,bits", CONTEXTS)
def test_matches_the_reference(fc, log_n, L, K, dnum, bits, secret):
    ctx, sk, pk, (ptd, pth) = setup_for(fc, log_n, L, K, dnum, bits)
    qs = ctx.moduli
    keyd, keyh = sk if secret else pk
    enc = ctx.encrypt_sk if secret else ctx.encrypt
    ref = encrypt_ref.encrypt_sk if secret else encrypt_ref.encrypt
    modes = itertools.cycle(["one", "each", "none"])
    for batch, level, index0 in itertools.product((1, 3, 8), (1, 2, L), (0, 5)):
        for mode in (next(modes), next(modes)):
            if mode == "one":    # a top-level [L, N] plaintext, read in place at every level
                d, h = ptd[1, :L], pth[1, :L]
            elif mode == "each":  # rows beyond the level (and beyond L) are skipped per plaintext
                d, h = ptd[:batch], pth[:batch]
            else:
                d = h = None
            got = fc.to_host(enc(d, keyd, SEED, level=level, batch=batch, index0=index0))
            want = ref(SEED, h, keyh, qs, log_n, level=level, batch=batch, index0=index0)
            assert got.shape == want.shape == (batch, 2, level, ctx.n)
            assert (got == want).all(), (batch, level, index0, mode)
    assert (fc.to_host(ptd) == pth).all() and (fc.to_host(keyd) == keyh).all()  # read only


@pytest.mark.parametrize("secret", [False, True])
@pytest.mark.parametrize("log_n,L,K,dnum,bits", [CONTEXTS[0], CONTEXTS[1]])
def test_the_three_properties_on_the_device(fc, log_n, L, K, dnum, bits, secret):
    ctx, sk, pk, (ptd, _) = setup_for(fc, log_n, L, K, dnum, bits)
    keyd = (sk if secret else pk)[0]
    enc = ctx.encrypt_sk if secret else ctx.encrypt
    pt = ptd[2, :L].contiguous()
    # (i) element 0, index0 = 0, level L is the single top-level call
    old = enc(pt, keyd, SEED)
    assert old.shape == (2, L, ctx.n)
    top = enc(pt, keyd, SEED, batch=4)
    assert (top[0] == old).all()
    assert (enc(pt, keyd, SEED, level=L) == old).all()  # no batch axis
    # (ii) level l is rows 0 .. l-1 of the level-L result, and drop_level's
    for level in (1, 2):
        low = enc(pt, keyd, SEED, level=level, batch=4)
        assert (low == top[:, :, :level]).all()
        assert (low == ctx.drop_level(top, level)).all()
    # (iii) element i at index0 = k is element 0 at index0 = k + i
    at5 = enc(pt, keyd, SEED, batch=3, index0=5)
    for i in range(3):
        assert (enc(pt, keyd, SEED, batch=1, index0=5 + i)[0] == at5[i]).all()
    assert (enc(pt, keyd, SEED, batch=4, index0=3)[2:] == at5[:2]).all()
    assert not (at5[0] == at5[1]).all()


@pytest.mark.parametrize("log_n,L,K,dnum,bits", [CONTEXTS[0], CONTEXTS[1], CONTEXTS[3]])
def test_slots_form_is_encode_then_encrypt(fc, log_n, L, K, dnum, bits):
    import torch

    ctx, sk, pk, _ = setup_for(fc, log_n, L, K, dnum, bits)
    rng = np.random.default_rng(9)
    for log_slots in (None, 3):
        ns = ctx.n // 2 if log_slots is None else 1 << log_slots
        z = torch.from_numpy(rng.uniform(-1, 1, (3, ns)) + 1j * rng.uniform(-1, 1, (3, ns))).to("cuda")
        for level, secret in itertools.product((2, L), (False, True)):
            keyd = (sk if secret else pk)[0]
            enc = ctx.encrypt_sk if secret else ctx.encrypt
            pt = ctx.encode(z, D50, level=level, log_slots=log_slots)
            want = enc(pt, keyd, SEED, index0=5)
            got = ctx.encrypt_slots(z, D50, keyd, secret=secret, level=level, log_slots=log_slots,
                                    seed=SEED, index0=5)
            assert got.shape == (3, 2, level, ctx.n)
            assert (got == want).all(), (log_slots, level, secret)
    # no batch axis, level defaults to L
    one = ctx.encrypt_slots(z[1], D50, pk[0], log_slots=3, seed=SEED, index0=6)
    assert one.shape == (2, L, ctx.n)
    assert (one == ctx.encrypt(ctx.encode(z, D50, log_slots=3), pk[0], SEED, index0=5)[1]).all()


@pytest.mark.parametrize("log_n,L,K,dnum,bits", [CONTEXTS[0], CONTEXTS[1]])
def test_decrypts_and_decodes_under_device_keys(fc, log_n, L, K, dnum, bits):
    """The centred limb-0 coefficients of decrypt(ct) - pt lie within 21 (2N + 1) (public key:
    e0 + e_pk u + e1 s) and 21 (secret key: e); a slot is a sum of the N coefficients times unit
    roots over delta, so the decoded slots lie within N (bound + 1/2) / delta of z (1/2: the
    encoder's rounding), plus 2^-40 for the decoder's double-precision FFT (log N rounding steps of
    2^-53 on values of magnitude about 1)."""
    import torch

    ctx, sk, pk, (ptd, pth) = setup_for(fc, log_n, L, K, dnum, bits)
    qs, n = ctx.moduli, ctx.n
    rng = np.random.default_rng(17)
    z = rng.uniform(-1, 1, (3, n // 2)) + 1j * rng.uniform(-1, 1, (3, n // 2))
    zd = torch.from_numpy(z).to("cuda")
    for secret in (False, True):
        keyd = (sk if secret else pk)[0]
        enc = ctx.encrypt_sk if secret else ctx.encrypt
        bound = encrypt_ref.noise_bound(log_n, secret)
        for level in (1, L):
            ct = enc(ptd[:3], keyd, SEED, level=level)
            noise = encrypt_ref.noise_limb0(fc.to_host(ct), pth[:3, :level], sk[1], qs)
            worst = int(np.abs(noise).max())
            assert (fc.to_host(ctx.decrypt(ct, sk[0])) ==
                    encrypt_ref.decrypt(fc.to_host(ct), sk[1], qs)).all()
            cs = ctx.encrypt_slots(zd, D50, keyd, secret=secret, level=level, seed=SEED)
            back = ctx.decode(ctx.decrypt(cs, sk[0]), D50).cpu().numpy()
            err = float(np.abs(back - z).max())
            slot_bound = n * (bound + 0.5) / D50 + 2.0 ** -40
            print(f"bits {bits} secret={secret} level {level}: |noise| <= {worst} (bound {bound}), "
                  f"|decode - z| <= {err:.3e} (bound {slot_bound:.3e})")
            assert 0 < worst <= bound
            assert err <= slot_bound


def test_passes_and_the_unfused_switch_give_the_same_bits(fc, monkeypatch):
    """FHECORE_ENCRYPT_PASS=2 runs a batch of 5 as passes of 2, 2 and 1 (the plaintexts, the slots
    and the index advance with the pass); FHECORE_ENCRYPT_UNFUSED=1 takes the wide contexts' route
    on a narrow one."""
    import torch

    log_n, L, K, dnum, bits = CONTEXTS[0]
    ctx, sk, pk, (ptd, _) = setup_for(fc, log_n, L, K, dnum, bits)
    rng = np.random.default_rng(23)
    z = torch.from_numpy(rng.uniform(-1, 1, (5, 8)) + 1j * rng.uniform(-1, 1, (5, 8))).to("cuda")

    def run():
        return [ctx.encrypt(ptd[:5], pk[0], SEED, level=3, index0=5),
                ctx.encrypt_sk(ptd[:5], sk[0], SEED, level=3, index0=5),
                ctx.encrypt(ptd[0], pk[0], SEED, level=2, batch=5),
                ctx.encrypt_slots(z, D50, pk[0], log_slots=3, seed=SEED),
                ctx.encrypt_slots(z, D50, sk[0], secret=True, level=2, log_slots=3, seed=SEED)]

    want = run()
    for name, value in (("FHECORE_ENCRYPT_PASS", "2"), ("FHECORE_ENCRYPT_UNFUSED", "1")):
        monkeypatch.setenv(name, value)
        for g, w in zip(run(), want):
            assert (g == w).all(), name
        monkeypatch.delenv(name)


def test_errors_write_nothing(fc):
    """Each refusal of the list in include/fhecore.h returns FHE_EINVAL before any launch."""
    import torch
    from fhecore.context import _ptr

    log_n, L, K, dnum, bits = CONTEXTS[0]
    ctx, sk, pk, (ptd, pth) = setup_for(fc, log_n, L, K, dnum, bits)
    n, lib, h = ctx.n, fc.load(), ctx.handle
    poison = 0x5A5A5A5A5A5A5A5
    ct = torch.full((2, 2, L, n), poison, dtype=torch.int64, device="cuda")
    z = torch.zeros(2, n // 2, dtype=torch.complex128, device="cuda")
    nbytes = lib.fhe_encrypt_workspace(h, L, 2)
    assert nbytes == (4 + L) * 2 * n * 8
    assert lib.fhe_encrypt_workspace(h, 0, 2) == 0 and lib.fhe_encrypt_workspace(h, L + 1, 2) == 0
    ws = ctx.workspace(nbytes)

    def pkc(o=_ptr(ct), p=_ptr(ptd), rows=L + K, pb=2, k=_ptr(pk[0]), level=L, batch=2, index0=0,
            w=_ptr(ws), c=h, fn=lib.fhe_encrypt_level):
        return fn(c, o, p, rows, pb, k, level, batch, SEED, index0, w, None)

    def slc(o=_ptr(ct), s=_ptr(z), delta=D50, ls=log_n - 1, k=_ptr(pk[0]), secret=0, level=L,
            batch=2, index0=0, w=_ptr(ws), c=h):
        return lib.fhe_encrypt_slots(c, o, s, delta, ls, k, secret, level, batch, SEED, index0, w,
                                     None)

    def refused(rc, word):
        return rc == -1 and word in lib.fhe_last_error()

    for fn, key in ((lib.fhe_encrypt_level, pk[0]), (lib.fhe_encrypt_sk_level, sk[0])):
        k = _ptr(key)
        assert refused(pkc(c=None, fn=fn, k=k), b"null context")
        assert refused(pkc(o=None, fn=fn, k=k), b"null")
        assert refused(pkc(k=None, fn=fn), b"null")
        for level in (0, L + 1):
            assert refused(pkc(level=level, fn=fn, k=k), b"level")
        assert refused(pkc(rows=L - 1, fn=fn, k=k), b"pt_rows")
        assert pkc(p=None, rows=0, pb=1, batch=0, fn=fn, k=k) == 0  # rows are not read without pt
        for pb in (0, 3):
            assert refused(pkc(pb=pb, fn=fn, k=k), b"pt_batch")
            assert refused(pkc(p=None, pb=pb, fn=fn, k=k), b"pt_batch")
        assert refused(pkc(index0=(1 << 32) - 1, fn=fn, k=k), b"index0")
        assert pkc(index0=(1 << 32) - 1, pb=1, batch=1, level=0, fn=fn, k=k) == -1  # the last index
        assert pkc(index0=(1 << 32) - 1, pb=1, batch=0, fn=fn, k=k) == 0  # batch == 0 is a no-op
    assert refused(slc(c=None), b"null context")
    assert refused(slc(o=None), b"null") and refused(slc(k=None), b"null")
    assert refused(slc(s=None), b"null slots")
    for level in (0, L + 1):
        assert refused(slc(level=level), b"level")
    for bad in (0.0, -D50, float("inf"), float("nan")):
        assert refused(slc(delta=bad), b"delta")
    assert refused(slc(ls=log_n), b"log_slots")
    assert refused(slc(index0=(1 << 32) - 1), b"index0")
    assert slc(batch=0) == 0
    # overlaps of ct with pt, slots, the key and the workspace, either way round
    # (every span named here lies inside `both`, so even a call that got through would stay in
    # bounds: ct takes 16 N words, pt 12 N, the keys 8 N and 6 N, the workspace 16 N, the slots 2 N)
    words = 2 * 2 * L * n
    both = torch.full((3 * words,), poison, dtype=torch.int64, device="cuda")
    inside = both[words - n:]  # starts inside the span of a ct at both
    late = both[n:]            # a ct here starts inside the span of anything at both
    assert refused(pkc(o=_ptr(both), p=_ptr(inside)), b"overlaps pt")
    assert refused(pkc(o=_ptr(late), p=_ptr(both)), b"overlaps pt")
    assert refused(pkc(o=_ptr(both), k=_ptr(inside)), b"overlaps the key")
    assert refused(pkc(o=_ptr(late), k=_ptr(both)), b"overlaps the key")
    assert refused(pkc(o=_ptr(both), k=_ptr(inside), fn=lib.fhe_encrypt_sk_level), b"overlaps the key")
    assert refused(pkc(o=_ptr(both), w=_ptr(inside)), b"overlaps the workspace")
    assert refused(pkc(o=_ptr(late), w=_ptr(both)), b"overlaps the workspace")
    assert refused(slc(o=_ptr(both), s=_ptr(inside)), b"overlaps slots")
    assert refused(slc(o=_ptr(late), s=_ptr(both)), b"overlaps slots")
    assert refused(slc(o=_ptr(both), k=_ptr(inside)), b"overlaps the key")
    assert refused(slc(o=_ptr(both), w=_ptr(inside)), b"overlaps the workspace")
    # workspace == NULL while the stream is capturing, and the capture still ends cleanly
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    rcs, err = [], ""
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        assert lib.fhe_graph_begin(sp) == 0
        for call in (
                lambda: lib.fhe_encrypt_level(h, _ptr(ct), _ptr(ptd), L + K, 2, _ptr(pk[0]), L, 2,
                                              SEED, 0, None, sp),
                lambda: lib.fhe_encrypt_sk_level(h, _ptr(ct), _ptr(ptd), L + K, 2, _ptr(sk[0]), L,
                                                 2, SEED, 0, None, sp),
                lambda: lib.fhe_encrypt_slots(h, _ptr(ct), _ptr(z), D50, log_n - 1, _ptr(pk[0]), 0,
                                              L, 2, SEED, 0, None, sp)):
            rcs.append(call())
            err += lib.fhe_last_error().decode()
        gr = ctypes.c_void_p()
        lib.fhe_graph_end(sp, ctypes.byref(gr))
        if gr.value:
            lib.fhe_graph_destroy(gr)
    assert rcs == [-1, -1, -1] and err.count("capturing") == 3
    torch.cuda.synchronize()
    assert (ct == poison).all() and (both == poison).all()
    assert (fc.to_host(ptd) == pth).all()
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="level"):
        ctx.encrypt(ptd[:2], pk[0], SEED, level=L + 1)
    with pytest.raises(ValueError, match="batch"):
        ctx.encrypt(ptd[:2], pk[0], SEED, batch=3)
    with pytest.raises(fc.FheError, match="pt_rows"):
        ctx.encrypt(ptd[:2, :2].contiguous(), pk[0], SEED, level=3)


def test_graph_replay(fc):
    """The three calls captured with explicit workspaces and replayed twice give the eager bits."""
    import torch

    log_n, L, K, dnum, bits = CONTEXTS[0]
    ctx, sk, pk, (ptd, _) = setup_for(fc, log_n, L, K, dnum, bits)
    n, lib = ctx.n, fc.load()
    rng = np.random.default_rng(31)
    z = torch.from_numpy(rng.uniform(-1, 1, (3, n // 2)) + 1j * rng.uniform(-1, 1, (3, n // 2))).to("cuda")
    pt = ptd[:3].clone()

    def eager():
        return (ctx.encrypt(pt, pk[0], SEED, level=3, index0=5),
                ctx.encrypt_sk(pt, sk[0], SEED, level=3, index0=5),
                ctx.encrypt_slots(z, D50, pk[0], level=2, seed=SEED))

    want = eager()
    outs = [torch.zeros_like(w) for w in want]
    wss = [ctx.workspace(lib.fhe_encrypt_workspace(ctx.handle, 3, 3)) for _ in outs]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.encrypt(pt, pk[0], SEED, level=3, index0=5, workspace=wss[0], out=outs[0])
            ctx.encrypt_sk(pt, sk[0], SEED, level=3, index0=5, workspace=wss[1], out=outs[1])
            ctx.encrypt_slots(z, D50, pk[0], level=2, seed=SEED, workspace=wss[2], out=outs[2])
        for _ in range(2):
            for o in outs:
                o.zero_()
            g.launch()
            stream.synchronize()
            for o, w in zip(outs, want):
                assert (o == w).all()
        # the captured pointers, new inputs
        pt.copy_(ptd[3:6])
        z.mul_(0.5)
        g.launch()
        stream.synchronize()
    for o, w in zip(outs, eager()):
        assert (o == w).all()
