"""GPU parity on the structured inputs of tests/adversarial.py, bit for bit against the reference
the existing test of each operation uses: rescale (and the fused rescale of lincomb / mul_plain)
on both sides of the centred lift's wrap and on words that rescale to exactly 0; baseconv at the
top of its sums; the key-switch (top level, below it, in place) on 0 / q - 1 / worst-case operands
under all-(t - 1), selector and zero keys; rotate, rotate_hoisted, the rotation sums, the linear
transform, mul_relin and hommult on the same.  Wherever the reference is all zero the output is
asserted to hold no non-zero word (a final reduction one step short stores q for 0).

N = 2^10 (2^12 where a row group needs it), batches of 1 and 3.  References that go through Python
object arithmetic are computed once per context and shared by the cases."""
import numpy as np
import pytest

import adversarial as adv
import coracle
import pyoracle
import refs

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


def u64(x):
    return np.asarray(x).astype(np.uint64)


_CTX = {}


def ctx_for(fc, log_n, L, K, dnum, bits=60):
    """As tests/test_gpu_levels.py builds its contexts; bits = "far": tests/test_gpu_wide.py's."""
    key = (log_n, L, K, dnum, bits)
    if key not in _CTX:
        if bits == 60:
            _CTX[key] = fc.Context(log_n, L=L, K=K, dnum=dnum)
        elif bits == "far":
            qs, ps = adv.far_chain()
            assert (L, K) == (len(qs), len(ps))
            _CTX[key] = fc.Context(log_n, moduli=qs, special=ps, dnum=dnum)
        else:
            m = fc.gen_moduli(log_n, L + K, bits=bits)
            _CTX[key] = fc.Context(log_n, moduli=m[:L], special=m[L:], dnum=dnum)
    return _CTX[key]


LZ16 = (10, 5, 2, 3, 60)   # fused lz16 (qfin)
WIDE = (10, 5, 2, 3, 62)   # a modulus >= 2^61: the unfused exact kernels


# ---- rescale ------------------------------------------------------------------------------------

def _rescale_chain(fc, name):
    """(log_n, moduli, levels rescaled)."""
    if name == "b60-n10":
        return 10, fc.gen_moduli(10, 3), [3]
    if name == "b60-n12":
        return 12, fc.gen_moduli(12, 4), [4]
    if name == "b62":  # the unfused spread
        return 10, fc.gen_moduli(10, 3, bits=62), [3]
    if name == "q0-60-over-50":  # the dropped limb a 50-bit prime; at level 2 the survivor is wider
        return 10, fc.gen_moduli(10, 1) + fc.gen_moduli(10, 3, bits=50), [4, 3, 2]
    if name == "far":
        return 10, adv.far_chain()[0], [4]
    raise ValueError(name)


RESCALE_CHAINS = ["b60-n10", "b60-n12", "b62", "q0-60-over-50", "far"]
_RESCALE = {}


def _rescale_case(fc, name):
    """Context, and per level: the 9-poly boundary input in both forms with both references (the
    smaller batches are its leading polys)."""
    if name not in _RESCALE:
        log_n, mods, levels = _rescale_chain(fc, name)
        ctx = fc.Context(log_n, moduli=mods)
        per = {}
        for lv in levels:
            ml = mods[:lv]
            x = adv.rescale_boundary(ml, log_n, 9, seed=lv)
            want = u64(np.stack([pyoracle.rescale_coeff(x[p].astype(object), ml)
                                 for p in range(9)]))
            per[lv] = (x, want, coracle.ntt_fwd(x, ml), coracle.ntt_fwd(want, ml[:-1]))
        _RESCALE[name] = (ctx, per)
    return _RESCALE[name]


# polys 1; 8 and 9: the two workgroup placements of k_lift_col
@pytest.mark.parametrize("polys", [1, 8, 9])
@pytest.mark.parametrize("name", RESCALE_CHAINS)
def test_rescale_on_the_boundary(fc, name, polys):
    ctx, per = _rescale_case(fc, name)
    for lv, (x, want, xn, wantn) in per.items():
        got = fc.to_host(ctx.rescale(fc.to_device(x[:polys]), ntt_form=False))
        assert got.shape == (polys, lv - 1, ctx.n)
        bad = np.argwhere(got != want[:polys])
        # (poly, limb, coefficient, index of the dropped residue in adv.rescale_edges)
        where = [(int(p), int(j), int(c), int(c + p) % 7) for p, j, c in bad[:4]]
        assert bad.size == 0, (lv, "coeff", where)
        # exact zeros stay zeros (every third word), never q
        assert ((got == 0).sum(axis=-1) >= ctx.n // 4).all(), lv
        gotn = fc.to_host(ctx.rescale(fc.to_device(xn[:polys]), ntt_form=True))
        assert (gotn == wantn[:polys]).all(), (lv, "ntt")


@pytest.mark.parametrize("spec", [LZ16, WIDE], ids=["lz16", "b62-wide"])
def test_fused_rescales_on_the_boundary(fc, spec):
    """lincomb(one term, scalar 1, rescale), mul_plain(all ones, rescale) and
    mul_relin(ct, (1, 0), rescale) are rescale itself (b = (1, 0) in NTT form gives d0 = a0,
    d1 = a1, d2 = 0, so the key-switch adds nothing whatever the key): on the NTT-form boundary
    input, at the top level and one below, each equals ctx.rescale of the same input and the
    reference."""
    log_n, L, K, dnum, _ = spec
    ctx = ctx_for(fc, *spec)
    qs = ctx.moduli
    one = ctx.encode_scalars([1], exact=True)
    ones = fc.to_device(np.ones((L, ctx.n), dtype=np.uint64))
    kb = fc.to_device(rand(ctx.all_moduli, log_n, (dnum,), seed=1))
    ka = fc.to_device(rand(ctx.all_moduli, log_n, (dnum,), seed=2))
    for lv in (L, L - 1):
        ql = qs[:lv]
        x = adv.rescale_boundary(ql, log_n, 6, seed=10 + lv)
        want = u64(np.stack([pyoracle.rescale_coeff(x[p].astype(object), ql) for p in range(6)]))
        wantn = coracle.ntt_fwd(want, ql[:-1]).reshape(3, 2, lv - 1, ctx.n)
        ct = fc.to_device(coracle.ntt_fwd(x, ql).reshape(3, 2, lv, ctx.n))
        unit = np.zeros((3, 2, lv, ctx.n), dtype=np.uint64)
        unit[:, 0] = 1
        unit = fc.to_device(unit)
        for batch in (1, 3):
            base = fc.to_host(ctx.rescale(ct[:batch]))
            assert (base == wantn[:batch]).all(), (lv, batch, "rescale")
            got = fc.to_host(ctx.lincomb([ct[:batch]], one, rescale=True, level=lv))
            assert (got == base).all(), (lv, batch, "lincomb")
            got = fc.to_host(ctx.mul_plain(ct[:batch], ones, rescale=True))
            assert (got == base).all(), (lv, batch, "mul_plain")
            got = fc.to_host(ctx.mul_relin(ct[:batch], unit[:batch], kb, ka, rescale=True))
            assert (got == base).all(), (lv, batch, "mul_relin")


# ---- base conversion ----------------------------------------------------------------------------

# (source limb0, source limbs, target limb0, targets) over Q u P = 4 + 2 limbs: windows of 1, 2 and
# 4 limbs, and ModDown's own P -> Q
BC_WINDOWS = [(1, 1, 2, 4), (0, 2, 2, 4), (0, 4, 4, 2), (4, 2, 0, 4)]


@pytest.mark.parametrize("bits", [60, 61, 62, "far"])
def test_baseconv_at_the_top_of_its_sums(fc, bits):
    log_n = 10
    ctx = ctx_for(fc, log_n, 4, 2, 2, bits)
    allm = ctx.all_moduli
    for s0, S, t0, T in BC_WINDOWS:
        src, dst = allm[s0:s0 + S], allm[t0:t0 + T]
        x = adv.conv_worst(src, log_n)
        got = fc.to_host(ctx.baseconv(fc.to_device(x), s0, t0, T))
        assert (got == coracle.baseconv(x, src, dst)).all(), (s0, S, t0, T)
        zero = np.zeros_like(x)
        assert not fc.to_host(ctx.baseconv(fc.to_device(zero), s0, t0, T)).any(), (s0, S, t0, T)


# ---- key-switch, top level ----------------------------------------------------------------------

# one context per plan path (tests/test_gpu_levels.py KS_CONTEXTS and the rows of
# tests/test_gpu_parity.py test_keyswitch_paths_match_oracle)
KS_PATHS = {
    "lz16-qfin": LZ16,
    "b61-split30": (10, 5, 2, 3, 61),
    "b62-wide": WIDE,
    "dnum6-unfused": (10, 6, 2, 6, 60),
    "K5-no-fused-moddown": (10, 4, 5, 2, 60),
    "alpha5-no-fused-up": (12, 10, 2, 2, 60),
    "ragged-last-digit": (12, 7, 2, 3, 60),
}
KEY_KINDS = ["tm1", "select_0", "select_last", "zero"]
_D2 = {}


def _d2_all(ctx, spec):
    """[4][L][N]: every ks_d2 kind, in adv.D2_KINDS order (zero first)."""
    if spec not in _D2:
        _D2[spec] = np.stack([adv.ks_d2(k, ctx.moduli, ctx.special, spec[3], spec[0])
                              for k in adv.D2_KINDS])
    return _D2[spec]


@pytest.mark.parametrize("keys", KEY_KINDS)
@pytest.mark.parametrize("path", sorted(KS_PATHS))
def test_keyswitch_on_structured_operands(fc, path, keys):
    spec = KS_PATHS[path]
    log_n, L, K, dnum, _ = spec
    ctx = ctx_for(fc, *spec)
    qs, ps = ctx.moduli, ctx.special
    d2 = _d2_all(ctx, spec)
    kb, ka = adv.ks_keys(keys, ctx.all_moduli, dnum, log_n)
    want = [coracle.keyswitch(d2[i], kb, ka, qs, ps, dnum) for i in range(4)]
    dkb, dka = fc.to_device(kb), fc.to_device(ka)
    # zero d2 alone, the other three kinds as one batch
    for lo, hi in ((0, 1), (1, 4)):
        ks0, ks1 = ctx.keyswitch(fc.to_device(d2[lo:hi]), dkb, dka)
        g0, g1 = fc.to_host(ks0), fc.to_host(ks1)
        for i in range(lo, hi):
            kind = adv.D2_KINDS[i]
            assert (g0[i - lo] == want[i][0]).all(), (kind, 0)
            assert (g1[i - lo] == want[i][1]).all(), (kind, 1)
            if kind == "zero" or keys == "zero":
                assert not g0[i - lo].any() and not want[i][0].any(), kind
            if kind == "zero" or keys != "tm1":
                assert not g1[i - lo].any() and not want[i][1].any(), kind
    if path in ("lz16-qfin", "b62-wide"):
        # ks0 written in place on d2: the finish reads d2 while it stores
        t = fc.to_device(d2[1:4])
        ks1 = ctx.empty(3, L, ctx.n)
        r0, r1 = ctx.keyswitch(t, dkb, dka, out=(t, ks1))
        assert r0.data_ptr() == t.data_ptr()
        g0, g1 = fc.to_host(r0), fc.to_host(r1)
        for i in range(1, 4):
            assert (g0[i - 1] == want[i][0]).all() and (g1[i - 1] == want[i][1]).all(), i


# ---- key-switch below the top -------------------------------------------------------------------

LEVEL_D2 = ["modup_worst", "zero", "qm1"]


@pytest.mark.parametrize("keys", ["tm1", "select_0"])
@pytest.mark.parametrize("spec", [LZ16, WIDE], ids=["lz16", "b62-wide"])
def test_keyswitch_below_the_top_on_structured_operands(fc, spec, keys):
    """Level 3 of L = 5, alpha = 2 (digits [0, 2) and a partial [2, 3)) and level 1."""
    log_n, L, K, dnum, _ = spec
    ctx = ctx_for(fc, *spec)
    qs, ps = ctx.moduli, ctx.special
    kb, ka = adv.ks_keys(keys, ctx.all_moduli, dnum, log_n)
    dkb, dka = fc.to_device(kb), fc.to_device(ka)
    for level in (3, 1):
        d2 = np.stack([adv.ks_d2(k, qs, ps, dnum, log_n, level=level) for k in LEVEL_D2])
        want = [pyoracle.keyswitch(d2[i], kb, ka, qs, ps, dnum, level=level, ntt=refs.c_ntt())
                for i in range(3)]
        for batch in (1, 3):
            ks0, ks1 = ctx.keyswitch(fc.to_device(d2[:batch]), dkb, dka)
            g0, g1 = fc.to_host(ks0), fc.to_host(ks1)
            assert g0.shape == (batch, level, ctx.n)
            for i in range(batch):
                assert (g0[i].astype(object) == want[i][0]).all(), (level, batch, LEVEL_D2[i], 0)
                assert (g1[i].astype(object) == want[i][1]).all(), (level, batch, LEVEL_D2[i], 1)
                if LEVEL_D2[i] == "zero":
                    assert not g0[i].any(), (level, batch)
                if LEVEL_D2[i] == "zero" or keys == "select_0":
                    assert not g1[i].any(), (level, batch, LEVEL_D2[i])


# ---- the composites -----------------------------------------------------------------------------

CT_KINDS = ["zero", "qm1", "modup_worst"]
_WORLD = {}


def world(fc, spec):
    """Context, the Galois elements of tests/test_gpu_level_hoist.py, keys (all t - 1 and the two
    selectors) and plaintexts (all t - 1, all zero) on the device once."""
    if spec in _WORLD:
        return _WORLD[spec]
    log_n, L, K, dnum, _ = spec
    ctx = ctx_for(fc, *spec)
    n = ctx.n
    allm = ctx.all_moduli
    e1, e2, conj = pow(5, 1, 2 * n), pow(pow(5, 2, 2 * n), -1, 2 * n), 2 * n - 1
    hkeys = {e1: adv.ks_keys("tm1", allm, dnum, log_n),
             e2: adv.ks_keys("select_0", allm, dnum, log_n),
             conj: adv.ks_keys("select_last", allm, dnum, log_n)}
    dkeys = {k: (fc.to_device(b), fc.to_device(a)) for k, (b, a) in hkeys.items()}
    top = adv.ks_keys("tm1", allm, 1, log_n)[0][0]  # [L + K][N], every word t - 1
    hpts = {"tm1": top, "zero": np.zeros_like(top)}
    dpts = {k: fc.to_device(v) for k, v in hpts.items()}
    w = dict(ctx=ctx, spec=spec, elts=(e1, e2, conj), hkeys=hkeys, dkeys=dkeys, hpts=hpts,
             dpts=dpts, cts={})
    _WORLD[spec] = w
    return w


def _cts(w, level, seed=0):
    """[3][2][level][N]: c1 = the ks_d2 kinds of CT_KINDS, c0 random."""
    key = (level, seed)
    if key not in w["cts"]:
        ctx = w["ctx"]
        log_n, L, K, dnum, _ = w["spec"]
        c0 = rand(ctx.moduli[:level], log_n, (3,), seed=700 + 10 * level + seed)
        c1 = np.stack([adv.ks_d2(k, ctx.moduli, ctx.special, dnum, log_n, level=level)
                       for k in CT_KINDS])
        w["cts"][key] = np.ascontiguousarray(np.stack([c0, c1], axis=1))
    return w["cts"][key]


def _keys(w, ks, dev):
    src = w["dkeys"] if dev else w["hkeys"]
    return [src.get(k) for k in ks]


def same(got, want):
    return got.shape == np.shape(want) and (got.astype(object) == want).all()


@pytest.mark.parametrize("spec", [LZ16, WIDE], ids=["lz16", "b62-wide"])
def test_rotate_and_rotate_hoisted_on_structured_ciphertexts(fc, spec):
    w = world(fc, spec)
    ctx = w["ctx"]
    log_n, L, K, dnum, _ = spec
    qs, ps = ctx.moduli, ctx.special
    e1, e2, conj = w["elts"]
    ct = _cts(w, L)
    dct = fc.to_device(ct)
    # one step under the all-(t - 1) key, the conjugation under a selector
    for k in (e1, conj):
        hb, ha = w["hkeys"][k]
        want = [pyoracle.rotate(ct[b], k, hb, ha, qs, ps, dnum, log_n, level=L, ntt=refs.c_ntt())
                for b in range(3)]
        for batch in (1, 3):
            got = fc.to_host(ctx.rotate(dct[:batch], k, *w["dkeys"][k]))
            for b in range(batch):
                assert same(got[b], want[b]), ("rotate", k, batch, CT_KINDS[b])
                if k == conj:  # ks1 = 0 under a selector
                    assert not got[b, 1].any(), (k, batch, CT_KINDS[b])
    ks = [e1, e2, conj]
    want = [pyoracle.rotate_hoisted(ct[b], ks, _keys(w, ks, False), qs, ps, dnum, log_n)
            for b in range(3)]
    for batch in (1, 3):
        got = fc.to_host(ctx.rotate_hoisted(dct[:batch], ks, _keys(w, ks, True)))
        assert got.shape == (3, batch, 2, L, ctx.n)
        for b in range(batch):
            assert same(got[:, b], want[b]), ("rotate_hoisted", batch, CT_KINDS[b])
            assert not got[1:, b, 1].any(), (batch, CT_KINDS[b])  # the selectors' ks1


def _sum_refs(w, level):
    """rotate_sum_hoisted, rotate_sum_multi and linear_transform references for the three
    ciphertexts of _cts, plaintexts all t - 1: pyoracle at `level`."""
    ctx = w["ctx"]
    log_n, L, K, dnum, _ = w["spec"]
    qs, ps = ctx.moduli, ctx.special
    e1, e2, conj = w["elts"]
    ct = _cts(w, level)
    others = [_cts(w, level, seed=1), _cts(w, level, seed=2)]
    pt = w["hpts"]["tm1"]
    sks, mks, baby, giant = [1, e1, e2], [e1, 1, conj], [1, e1], [e2, 1]
    tail = (qs, ps, dnum, log_n)
    at = dict(level=level, ntt=refs.c_ntt())
    out = dict(sks=sks, mks=mks, baby=baby, giant=giant, ct=ct, others=others)
    out["sum"] = [pyoracle.rotate_sum_hoisted(ct[b], sks, _keys(w, sks, False), [pt] * 3, *tail,
                                              **at) for b in range(3)]
    out["multi"] = [pyoracle.rotate_sum_multi([ct[b], others[0][b], others[1][b]], mks,
                                              _keys(w, mks, False), *tail, **at) for b in range(3)]
    out["lt"] = [pyoracle.linear_transform(ct[b], baby, _keys(w, baby, False), giant,
                                           _keys(w, giant, False), [[pt, pt], [pt, pt]], *tail,
                                           **at) for b in range(3)]
    return out


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("spec", [LZ16, WIDE], ids=["lz16", "b62-wide"])
def test_rotation_sums_and_linear_transform_on_structured_ciphertexts(fc, spec, below):
    """Three-term rotation sums and a 2 x 2 linear transform, at the top level and one below it.
    Plaintexts all t - 1; then all zero, where every output word must be zero."""
    w = world(fc, spec)
    ctx = w["ctx"]
    L = spec[1]
    level = L - 1 if below else L
    r = _sum_refs(w, level)
    dct = fc.to_device(r["ct"])
    dothers = [fc.to_device(c) for c in r["others"]]
    pt, zero = w["dpts"]["tm1"], w["dpts"]["zero"]
    for batch in (1, 3):
        got = fc.to_host(ctx.rotate_sum_hoisted(dct[:batch], r["sks"], _keys(w, r["sks"], True),
                                                [pt] * 3))
        assert got.shape == (batch, 2, level, ctx.n)
        for b in range(batch):
            assert same(got[b], r["sum"][b]), ("rotate_sum_hoisted", batch, CT_KINDS[b])
        got = fc.to_host(ctx.rotate_sum_hoisted(dct[:batch], r["sks"], _keys(w, r["sks"], True),
                                                [zero] * 3))
        assert not got.any(), ("rotate_sum_hoisted", batch, "zero plaintexts")
        got = fc.to_host(ctx.rotate_sum_multi([dct[:batch]] + [c[:batch] for c in dothers],
                                              r["mks"], _keys(w, r["mks"], True)))
        for b in range(batch):
            assert same(got[b], r["multi"][b]), ("rotate_sum_multi", batch, CT_KINDS[b])
        args = (r["baby"], _keys(w, r["baby"], True), r["giant"], _keys(w, r["giant"], True))
        got = fc.to_host(ctx.linear_transform(dct[:batch], *args, [[pt, pt], [pt, pt]]))
        for b in range(batch):
            assert same(got[b], r["lt"][b]), ("linear_transform", batch, CT_KINDS[b])
        got = fc.to_host(ctx.linear_transform(dct[:batch], *args, [[zero, zero], [zero, zero]]))
        assert not got.any(), ("linear_transform", batch, "zero plaintexts")


@pytest.mark.parametrize("keys", ["random", "tm1"])
@pytest.mark.parametrize("spec", [LZ16, WIDE], ids=["lz16", "b62-wide"])
def test_mul_relin_on_structured_ciphertexts(fc, spec, keys):
    """zero x random (every output word zero, with and without the rescale), (q - 1) x (q - 1) in
    every word, and a random pair; under random relinearisation keys and under all t - 1."""
    log_n, L, K, dnum, _ = spec
    ctx = ctx_for(fc, *spec)
    qs, ps = ctx.moduli, ctx.special
    allm = ctx.all_moduli
    if keys == "random":
        kb, ka = rand(allm, log_n, (dnum,), seed=3), rand(allm, log_n, (dnum,), seed=4)
    else:
        kb, ka = adv.ks_keys("tm1", allm, dnum, log_n)
    top = np.broadcast_to(adv.ks_d2("qm1", qs, ps, dnum, log_n), (2, L, ctx.n))
    r1, r2 = rand(qs, log_n, (2,), seed=5), rand(qs, log_n, (2,), seed=6)
    a = np.stack([np.zeros_like(r1), top, r1])
    b = np.stack([r2, top, r2])
    da, db, dkb, dka = (fc.to_device(v) for v in (a, b, kb, ka))
    for rescale in (False, True):
        want = [pyoracle.mul_relin(a[i], b[i], kb, ka, qs, ps, dnum, rescale, level=L,
                                   ntt=refs.c_ntt()) for i in range(3)]
        assert not want[0].any()
        for batch in (1, 3):
            got = fc.to_host(ctx.mul_relin(da[:batch], db[:batch], dkb, dka, rescale=rescale))
            assert got.shape == (batch, 2, L - (1 if rescale else 0), ctx.n)
            assert not got[0].any(), (rescale, batch, "zero ciphertext")
            for i in range(batch):
                assert same(got[i], want[i]), (rescale, batch, i)


@pytest.mark.parametrize("bits", [60, 61, 62])
@pytest.mark.parametrize("log_n", [10, 12])
def test_hommult_on_zero_and_largest_operands(fc, log_n, bits):
    mods = fc.gen_moduli(log_n, 3, bits=bits)
    ctx = fc.Context(log_n, moduli=mods)
    n = 1 << log_n
    top = np.stack([np.full((2, n), q - 1, dtype=np.uint64) for q in mods], axis=1)  # [2][L][N]
    r = rand(mods, log_n, (2,), seed=bits)
    a = np.stack([np.zeros_like(r), top, r])
    b = np.stack([r, top, np.zeros_like(r)])
    want = coracle.hommult(a, b, mods)
    for batch in (1, 3):
        got = fc.to_host(ctx.hommult(fc.to_device(a[:batch]), fc.to_device(b[:batch])))
        assert (got == want[:batch]).all(), batch
        assert not got[0].any(), batch
    assert not got[2].any()
