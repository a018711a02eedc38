"""GPU parity of the fused HomMult row kernel's pair form (csrc/ntt.hip hm_row_pairs): N = 2^16
with the default 60-bit (lz16) moduli is the only size that takes it.  Bit for bit against the C
oracle; HomMult is independent per ciphertext and per limb, so one reference per input kind
(batch 3, all 8 limbs) serves every batch size and limb window by slicing.  The second half checks
the paths that must not have changed: wide (62-bit) and 61-bit moduli at N = 2^16, and N = 2^15."""
import numpy as np
import pytest

import coracle

pytestmark = pytest.mark.gpu

LOG_N, L, B = 16, 8, 3
N = 1 << LOG_N
KINDS = ["random", "zeros", "qm1", "cross"]
# (limb0, nlimbs): 1 and 8 limbs divide / are divided by the 8 XCDs, 3 limbs take the third branch
# of xcd_limb_split; (5, 3) also offsets both twiddle tables and the fold table
WINDOWS = [(0, 1), (0, 3), (5, 3), (0, 8)]


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


@pytest.fixture(scope="module")
def ctx(fc):
    return fc.Context(LOG_N, L=L)


def _inputs(kind, qs):
    rng = np.random.default_rng(KINDS.index(kind) + 700)
    a = np.zeros((B, 2, L, N), dtype=np.uint64)
    b = np.zeros_like(a)
    for li, q in enumerate(qs):
        if kind == "random":
            a[:, :, li] = rng.integers(0, q, size=(B, 2, N), dtype=np.uint64)
            b[:, :, li] = rng.integers(0, q, size=(B, 2, N), dtype=np.uint64)
        elif kind == "qm1":  # the largest sums
            a[:, :, li] = q - 1
            b[:, :, li] = q - 1
        elif kind == "cross":  # only A1 and B0: the cross terms and the sign of b1'
            a[:, 1, li] = rng.integers(0, q, size=(B, N), dtype=np.uint64)
            b[:, 0, li] = rng.integers(0, q, size=(B, N), dtype=np.uint64)
    return a, b


_REF = {}


def _case(kind, qs):
    """(a, b, reference) for batch B over all L limbs, computed once per kind."""
    if kind not in _REF:
        a, b = _inputs(kind, qs)
        same = kind in ("zeros", "qm1")  # every ciphertext of the batch is the same
        ref = np.empty((B, 3, L, N), dtype=np.uint64)
        for i in range(B):
            ref[i] = ref[0] if same and i else coracle.hommult(a[i], b[i], qs)
        a.setflags(write=False)
        b.setflags(write=False)
        ref.setflags(write=False)
        _REF[kind] = (a, b, ref)
    return _REF[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("limb0,nl", WINDOWS)
@pytest.mark.parametrize("batch", [1, 3])
def test_pair_form_matches_oracle(fc, ctx, batch, limb0, nl, kind):
    a, b, ref = _case(kind, ctx.moduli)
    sl = slice(limb0, limb0 + nl)
    ad = fc.to_device(np.ascontiguousarray(a[:batch, :, sl]))
    bd = fc.to_device(np.ascontiguousarray(b[:batch, :, sl]))
    d = fc.to_host(ctx.hommult(ad, bd, limb0=limb0))
    assert d.shape == (batch, 3, nl, N)
    assert (d == ref[:batch, :, sl]).all()
    if kind == "zeros":
        assert not d.any()


@pytest.mark.parametrize("log_n,bits", [(16, 62), (16, 61), (15, 60)])
def test_other_paths_unchanged(fc, log_n, bits):
    """Wide moduli (exact butterflies, 8 + 8 stages), 61-bit moduli (the 9 + 7 split with the full
    7-stage rows: not lz16) and N = 2^15 keep the full stages and the N^-1 R fold."""
    mods = fc.gen_moduli(log_n, 3, bits=bits)
    c = fc.Context(log_n, moduli=mods)
    rng = np.random.default_rng(bits + log_n)
    n = 1 << log_n
    a = np.stack([rng.integers(0, q, size=(2, 2, n), dtype=np.uint64) for q in mods], axis=2)
    b = np.stack([rng.integers(0, q, size=(2, 2, n), dtype=np.uint64) for q in mods], axis=2)
    a[1, :, :, ::3] = np.array(mods, dtype=np.uint64).reshape(1, -1, 1) - 1
    d = fc.to_host(c.hommult(fc.to_device(a), fc.to_device(b)))
    for i in range(2):
        assert (d[i] == coracle.hommult(a[i], b[i], mods)).all()
