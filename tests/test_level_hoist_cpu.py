"""tests/level_hoist_ref.py, the reference of the hoisted rotations, rotation sums and the BSGS
linear transform below the top level, checked on the CPU: at level = L it is the oracle word for
word, and under real keys each of the four results decrypts at every level l = 1 .. L to the
expected sum of plaintext times rotated message.

The decryption error bound is measured, not fixed: the error of the same inputs at l = L (the path
already trusted) is the yardstick and every lower level must stay within 4x of it -- dropping
digits removes noise terms, and two bits cover the different rounding of a partial last digit.
Measured on this file's inputs (max |decryption - expectation| over the coefficients, l = L and
the worst l < L): see DESIGN.md §3 "Hoisted forms below the top"."""
import random

import numpy as np
import pytest

import coracle
import level_hoist_ref as ref
import pyoracle

LOG_N, L, K, DNUM = 10, 5, 2, 3
N = 1 << LOG_N


def sigma_int(m, k):
    """sigma_k on an integer coefficient vector."""
    out = [0] * N
    for i, v in enumerate(m):
        e = i * k % (2 * N)
        if e < N:
            out[e] = v
        else:
            out[e - N] = -v
    return out


def negacyclic_int(a, b):
    full = np.convolve(np.asarray(a, dtype=object), np.asarray(b, dtype=object))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return [int(v) for v in out]


def add_int(a, b):
    return [x + y for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def world():
    """Moduli, a ternary secret, three real ciphertexts, rotation keys and plaintext diagonals
    (ranges as in tests/test_gpu_rotsum.py), built once."""
    mods = pyoracle.gen_moduli(LOG_N, L + K, 60)
    qs, ps = [int(q) for q in mods[:L]], [int(p) for p in mods[L:]]
    allm = qs + ps
    rng = random.Random(2024)
    s = [rng.randrange(-1, 2) for _ in range(N)]
    ntt = lambda v, m: coracle.ntt_fwd(np.asarray(pyoracle._to_rns(v, m), dtype=np.uint64),  # noqa: E731
                                       m).astype(object)
    s_n = ntt(s, qs)
    col = pyoracle._mods_col(qs)
    cts, msgs = [], []
    for _ in range(3):
        m = [rng.randrange(-1000, 1000) for _ in range(N)]
        a = np.stack([np.array([rng.randrange(q) for _ in range(N)], dtype=object) for q in qs])
        e = ntt([rng.randrange(-3, 4) for _ in range(N)], qs)
        cts.append(np.stack([(-a * s_n + e + ntt(m, qs)) % col, a]).astype(np.uint64))
        msgs.append(m)
    ks = [1, pyoracle.galois_elt(1, N), pyoracle.galois_elt(-2, N), 2 * N - 1]
    keys = {}
    for k in ks[1:]:
        kb, ka = pyoracle.gen_rot_key(s, k, qs, ps, DNUM, rng)
        keys[k] = (kb.astype(np.uint64), ka.astype(np.uint64))
    pt_int = [[rng.randrange(-3, 4) for _ in range(N)] for _ in range(4)]
    pts = [coracle.ntt_fwd(np.asarray(pyoracle._to_rns(p, allm), dtype=np.uint64), allm)
           for p in pt_int]
    return dict(qs=qs, ps=ps, s_n=s_n, cts=cts, msgs=msgs, ks=ks, keys=keys, pt_int=pt_int, pts=pts)


def decrypt(ct, w, level):
    ql = w["qs"][:level]
    ct = np.asarray(ct).astype(object)
    dec = (ct[0] + ct[1] * w["s_n"][:level]) % pyoracle._mods_col(ql)
    return pyoracle.crt_centered(coracle.ntt_inv(dec.astype(np.uint64), ql).astype(object), ql)


def error(ct, w, level, expect):
    return max(abs(int(x) - e) for x, e in zip(decrypt(ct, w, level), expect))


def cut(ct, level):
    return np.ascontiguousarray(np.asarray(ct)[..., :level, :])


# ---- the four operations at a level, each -> [(ciphertext, expected message), ...] -------------
def op_rotate_hoisted(w, level):
    ks = w["ks"][1:3] + w["ks"][3:]
    out = ref.rotate_hoisted(cut(w["cts"][0], level), ks, [w["keys"][k] for k in ks], w["qs"],
                             w["ps"], DNUM, level, LOG_N)
    return [(o, sigma_int(w["msgs"][0], k)) for o, k in zip(out, ks)]


def op_rotate_sum_hoisted(w, level):
    ks = w["ks"]
    out = ref.rotate_sum_hoisted(cut(w["cts"][0], level), ks, [w["keys"].get(k) for k in ks],
                                 w["pts"], w["qs"], w["ps"], DNUM, level, LOG_N)
    expect = [0] * N
    for k, p in zip(ks, w["pt_int"]):
        expect = add_int(expect, negacyclic_int(p, sigma_int(w["msgs"][0], k)))
    return [(out, expect)]


def op_rotate_sum_multi(w, level):
    ks = [w["ks"][1], 1, w["ks"][3]]
    out = ref.rotate_sum_multi([cut(c, level) for c in w["cts"]], ks,
                               [w["keys"].get(k) for k in ks], w["qs"], w["ps"], DNUM, level, LOG_N)
    expect = [0] * N
    for k, m in zip(ks, w["msgs"]):
        expect = add_int(expect, sigma_int(m, k))
    return [(out, expect)]


def op_linear_transform(w, level):
    baby, giant = [1, w["ks"][1]], [1, w["ks"][2]]
    pts = [w["pts"][:2], w["pts"][2:]]
    out = ref.linear_transform(cut(w["cts"][0], level), baby, [w["keys"].get(k) for k in baby],
                               giant, [w["keys"].get(k) for k in giant], pts, w["qs"], w["ps"],
                               DNUM, level, LOG_N)
    expect = [0] * N
    for g, kg in enumerate(giant):
        inner = [0] * N
        for b, kb in enumerate(baby):
            inner = add_int(inner, negacyclic_int(w["pt_int"][2 * g + b],
                                                  sigma_int(w["msgs"][0], kb)))
        expect = add_int(expect, sigma_int(inner, kg))
    return [(out, expect)]


OPS = {"rotate_hoisted": op_rotate_hoisted, "rotate_sum_hoisted": op_rotate_sum_hoisted,
       "rotate_sum_multi": op_rotate_sum_multi, "linear_transform": op_linear_transform}


def test_top_level_is_the_oracle_word_for_word(world):
    w = world
    qs, ps, ct = w["qs"], w["ps"], w["cts"][0]
    ks = w["ks"]
    rk = ks[1:]
    assert (ref.rotate_hoisted(ct, rk, [w["keys"][k] for k in rk], qs, ps, DNUM, L, LOG_N) ==
            pyoracle.rotate_hoisted(ct, rk, [w["keys"][k] for k in rk], qs, ps, DNUM, LOG_N)).all()
    keys = [w["keys"].get(k) for k in ks]
    assert (ref.rotate_sum_hoisted(ct, ks, keys, w["pts"], qs, ps, DNUM, L, LOG_N) ==
            pyoracle.rotate_sum_hoisted(ct, ks, keys, w["pts"], qs, ps, DNUM, LOG_N)).all()
    mk = [ks[1], 1, ks[3]]
    mkeys = [w["keys"].get(k) for k in mk]
    assert (ref.rotate_sum_multi(w["cts"], mk, mkeys, qs, ps, DNUM, L, LOG_N) ==
            pyoracle.rotate_sum_multi(w["cts"], mk, mkeys, qs, ps, DNUM, LOG_N)).all()
    baby, giant = [1, ks[1]], [1, ks[2]]
    bk, gk = [w["keys"].get(k) for k in baby], [w["keys"].get(k) for k in giant]
    pts = [w["pts"][:2], w["pts"][2:]]
    assert (ref.linear_transform(ct, baby, bk, giant, gk, pts, qs, ps, DNUM, L, LOG_N) ==
            pyoracle.linear_transform(ct, baby, bk, giant, gk, pts, qs, ps, DNUM, LOG_N)).all()


@pytest.mark.parametrize("name", list(OPS))
def test_every_level_decrypts_within_four_times_the_top_level_error(world, name):
    top = max(error(ct, world, L, expect) for ct, expect in OPS[name](world, L))
    worst = 0
    for level in range(1, L):
        err = max(error(ct, world, level, expect) for ct, expect in OPS[name](world, level))
        print(f"{name}: level {level} error {err} (top level {top})")
        worst = max(worst, err)
        assert err <= 4 * top, (name, level, err, top)
    print(f"{name}: top-level error {top}, worst lower-level error {worst}")


def test_a_level_whose_digits_are_a_shorter_chains_is_the_c_oracle_on_the_rows_it_reads(world):
    """Level 4 of (L, dnum) = (5, 3) has the digits of a 4-limb chain with dnum = 2, so the
    reference must equal the C restatement of rotate_sum_hoisted run on that chain with the key
    and plaintext rows the level reads (how tests/test_gpu_level_hoist.py evaluates the reference
    at N = 2^16)."""
    import level_ref

    w, level, dn = world, 4, 2
    assert level_ref.level_digits(level, L, DNUM) == pyoracle.digit_ranges(level, dn)
    rows = level_ref.key_rows(level, L, K)
    ks = w["ks"]
    first = w["keys"][ks[1]]
    kb = np.stack([(w["keys"].get(k) or first)[0] for k in ks])[:, :dn][:, :, rows]
    ka = np.stack([(w["keys"].get(k) or first)[1] for k in ks])[:, :dn][:, :, rows]
    pts = np.stack(w["pts"])[:, rows]
    ct = cut(w["cts"][0], level)
    want = coracle.rotate_sum_hoisted(ct, ks, np.ascontiguousarray(kb), np.ascontiguousarray(ka),
                                      np.ascontiguousarray(pts), w["qs"][:level], w["ps"], dn)
    got = ref.rotate_sum_hoisted(ct, ks, [w["keys"].get(k) for k in ks], w["pts"], w["qs"],
                                 w["ps"], DNUM, level, LOG_N)
    assert (got == want.astype(object)).all()
