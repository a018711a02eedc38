"""fhe_conj_split_level / fhe_conj_merge_level on the GPU (csrc/plain.hip) against pyoracle's
conj_split / conj_merge, which multiply by X^(N/2) in coefficient form: bit for bit at every level,
batch 1 and 3 (the batch / limb strides and the k = N/2 sign boundary), 50-, 60- and 62-bit chains;
in place, the refused overlaps, the slots under device keys, and inside a captured Graph."""
import ctypes

import numpy as np
import pytest

import pyoracle
import refs

pytestmark = pytest.mark.gpu
NTT = refs.c_ntt()

LOG_N, L, K, DNUM = 10, 3, 1, 3
N = 1 << LOG_N


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


_CTX = {}


def ctx_for(fc, bits):
    if bits not in _CTX:
        m = fc.gen_moduli(LOG_N, L + K, bits=bits)
        _CTX[bits] = fc.Context(LOG_N, moduli=m[:L], special=m[L:], dnum=DNUM)
    return _CTX[bits]


def rand(qs, lead, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, q, (*lead, N), dtype=np.uint64) for q in qs], axis=-2)


def u64(x):
    return np.asarray(x).astype(np.uint64)


@pytest.mark.parametrize("bits", [50, 60, 62])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("level", [1, 2, 3])
def test_split_and_merge_match_the_coefficient_form_reference(fc, bits, batch, level):
    ctx = ctx_for(fc, bits)
    qs = ctx.moduli
    a, b = rand(qs[:level], (batch, 2), 10 * level + batch), rand(qs[:level], (batch, 2), 77 + level)
    # the extremes on both sides of the sign boundary
    a[0, 0, :, N // 2 - 1:N // 2 + 1] = np.array(qs[:level], dtype=np.uint64)[:, None] - 1
    b[0, 1, :, N // 2 - 1:N // 2 + 1] = 0
    da, db = fc.to_device(a), fc.to_device(b)
    re, im = ctx.conj_split(da, db)
    want_re, want_im = pyoracle.conj_split(a, b, qs, level=level, ntt=NTT)
    assert tuple(re.shape) == tuple(im.shape) == (batch, 2, level, N)
    assert (fc.to_host(re) == u64(want_re)).all()
    assert (fc.to_host(im) == u64(want_im)).all()
    out = ctx.conj_merge(da, db)
    assert (fc.to_host(out) == u64(pyoracle.conj_merge(a, b, qs, level=level, ntt=NTT))).all()
    # the inputs are untouched
    assert (fc.to_host(da) == a).all() and (fc.to_host(db) == b).all()


def test_unbatched_operands(fc):
    ctx = ctx_for(fc, 60)
    a, b = rand(ctx.moduli[:2], (2,), 1), rand(ctx.moduli[:2], (2,), 2)
    re, im = ctx.conj_split(fc.to_device(a), fc.to_device(b))
    want = pyoracle.conj_split(a, b, ctx.moduli, level=2, ntt=NTT)
    assert tuple(re.shape) == (2, 2, N)
    assert (fc.to_host(re) == u64(want[0])).all() and (fc.to_host(im) == u64(want[1])).all()


@pytest.mark.parametrize("bits", [60, 62])
def test_in_place(fc, bits):
    ctx = ctx_for(fc, bits)
    qs = ctx.moduli
    a, b = rand(qs, (3, 2), 5), rand(qs, (3, 2), 6)
    want_re, want_im = pyoracle.conj_split(a, b, qs, level=L, ntt=NTT)
    da, db = fc.to_device(a), fc.to_device(b)
    re, im = ctx.conj_split(da, db, out=(da, db))  # re is ct, im is cc
    assert re is da and im is db
    assert (fc.to_host(da) == u64(want_re)).all() and (fc.to_host(db) == u64(want_im)).all()
    da, db = fc.to_device(a), fc.to_device(b)
    ctx.conj_split(da, db, out=(db, da))  # crossed: re is cc, im is ct
    assert (fc.to_host(db) == u64(want_re)).all() and (fc.to_host(da) == u64(want_im)).all()
    da, db = fc.to_device(a), fc.to_device(b)
    assert ctx.conj_merge(da, db, out=da) is da  # out is a
    assert (fc.to_host(da) == u64(pyoracle.conj_merge(a, b, qs, level=L, ntt=NTT))).all()
    da = fc.to_device(a)
    ctx.conj_merge(da, db, out=db)  # out is b
    assert (fc.to_host(db) == u64(pyoracle.conj_merge(a, b, qs, level=L, ntt=NTT))).all()


def test_overlaps_and_bad_arguments_are_refused(fc):
    import torch

    ctx = ctx_for(fc, 60)
    lib = fc.load()
    words = 2 * 2 * N  # one ciphertext at level 2
    buf = torch.zeros(4 * words + N, dtype=torch.int64, device="cuda")
    p = lambda off: ctypes.c_void_p(buf.data_ptr() + 8 * off)  # noqa: E731
    h = ctx.handle

    def split(re, im, ct, cc, level=2, batch=1):
        return lib.fhe_conj_split_level(h, re, im, ct, cc, level, batch, None)

    def merge(out, a, b, level=2, batch=1):
        return lib.fhe_conj_merge_level(h, out, a, b, level, batch, None)

    ct, cc, re, im = p(0), p(words), p(2 * words), p(3 * words)
    assert split(re, im, ct, cc) == 0
    assert split(ct, cc, ct, cc) == 0 and merge(ct, ct, cc) == 0
    # a partial overlap of an output with an input, and of re with im
    assert split(p(N), im, ct, cc) == -1 and b"overlaps" in lib.fhe_last_error()
    assert split(re, p(words + N), ct, cc) == -1
    assert split(re, p(2 * words + N), ct, cc) == -1 and b"re and im" in lib.fhe_last_error()
    assert split(re, re, ct, cc) == -1
    assert merge(p(N), ct, cc) == -1 and merge(p(words - N), ct, cc) == -1
    # levels and null pointers
    assert split(re, im, ct, cc, level=0) == -1 and split(re, im, ct, cc, level=L + 1) == -1
    assert merge(re, ct, cc, level=0) == -1 and merge(re, ct, cc, level=L + 1) == -1
    for args in ((None, im, ct, cc), (re, None, ct, cc), (re, im, None, cc), (re, im, ct, None)):
        assert split(*args) == -1 and b"null" in lib.fhe_last_error()
    for args in ((None, ct, cc), (re, None, cc), (re, ct, None)):
        assert merge(*args) == -1
    assert lib.fhe_conj_split_level(None, re, im, ct, cc, 2, 1, None) == -1
    torch.cuda.synchronize()
    # the Python layer checks shapes
    a = ctx.empty(2, 2, N)
    with pytest.raises(ValueError):
        ctx.conj_split(a, ctx.empty(2, 3, N))
    with pytest.raises(ValueError):
        ctx.conj_merge(a, ctx.empty(1, 2, 2, N))


def test_slots_under_device_keys(fc):
    """cc from rotate by 2N - 1: re / im decode to 2 Re z / 2 Im z and merge(split) to 2 z, within
    the 1e-7 the rotation test under keys allows (tests/test_gpu_keys.py); at level 3 and, dropped,
    at level 2."""
    import torch

    ctx = ctx_for(fc, 50)
    delta = 2.0 ** 45
    sk = ctx.keygen_secret(seed=41)
    elt = 2 * N - 1
    kb, ka = ctx.keygen_rotation(sk, elt, seed=42)
    rng = np.random.default_rng(8)
    z = rng.uniform(-1, 1, (2, N // 2)) + 1j * rng.uniform(-1, 1, (2, N // 2))
    pts = ctx.encode(z, delta)
    top = torch.stack([ctx.encrypt_sk(pts[i].contiguous(), sk, seed=43 + i) for i in range(2)])
    for level in (3, 2):
        ct = top if level == L else ctx.drop_level(top, level)
        cc = ctx.rotate(ct, elt, kb, ka)

        def slots(x):
            return ctx.decode(ctx.decrypt(x, sk), delta).cpu().numpy()

        assert np.abs(slots(cc) - z.conj()).max() < 1e-7
        re, im = ctx.conj_split(ct, cc)
        e_re = np.abs(slots(re) - 2 * z.real).max()
        e_im = np.abs(slots(im) - 2 * z.imag).max()
        e_m = np.abs(slots(ctx.conj_merge(re, im)) - 2 * z).max()
        print(f"level {level}: |re - 2 Re z| {e_re:.2e}, |im - 2 Im z| {e_im:.2e}, "
              f"|merge(split) - 2 z| {e_m:.2e}")
        assert e_re < 1e-7 and e_im < 1e-7 and e_m < 1e-7


def test_graph_replay_without_a_workspace(fc):
    import torch

    ctx = ctx_for(fc, 60)
    qs = ctx.moduli
    a, b = rand(qs[:2], (3, 2), 21), rand(qs[:2], (3, 2), 22)
    da, db = fc.to_device(a), fc.to_device(b)
    re, im, out = (torch.empty_like(da) for _ in range(3))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with fc.Graph() as g:
            ctx.conj_split(da, db, out=(re, im))
            ctx.conj_merge(re, im, out=out)
        re.zero_(), im.zero_(), out.zero_()
        g.launch()
        g.launch()
    stream.synchronize()
    want_re, want_im = pyoracle.conj_split(a, b, qs, level=2, ntt=NTT)
    assert (fc.to_host(re) == u64(want_re)).all() and (fc.to_host(im) == u64(want_im)).all()
    assert (fc.to_host(out) == u64(pyoracle.conj_merge(want_re, want_im, qs, level=2, ntt=NTT))).all()
