"""pyoracle's level= argument, the reference of the key-switch family below the top level, checked
on the CPU: every result at every level is pinned to what the functions it replaced computed, and
under real keys each of the four hoisted results decrypts at every level l = 1 .. L to the expected
sum of plaintext times rotated message.

The decryption error bound is measured, not fixed: the error of the same inputs at l = L (the path
already trusted) is the yardstick and every lower level must stay within 4x of it -- dropping
digits removes noise terms, and two bits cover the different rounding of a partial last digit.
Measured on this file's inputs (max |decryption - expectation| over the coefficients, l = L and
the worst l < L): see DESIGN.md §3 "Hoisted forms below the top"."""
import json
import os

import numpy as np
import pytest

import coracle
import pyoracle
import refs
from refs import cut

LOG_N, L, K, DNUM = 10, 5, 2, 3
N = 1 << LOG_N
NTT = refs.c_ntt()


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
    return refs.hoist_world(LOG_N, L, K, DNUM)


def decrypt(ct, w, level):
    ql = w["qs"][:level]
    ct = np.asarray(ct).astype(object)
    dec = (ct[0] + ct[1] * w["s_n"][:level]) % pyoracle._mods_col(ql)
    return pyoracle.crt_centered(coracle.ntt_inv(dec.astype(np.uint64), ql).astype(object), ql)


def error(ct, w, level, expect):
    return max(abs(int(x) - e) for x, e in zip(decrypt(ct, w, level), expect))


# ---- the four operations at a level, each -> [(ciphertext, expected message), ...] -------------
def op_rotate_hoisted(w, level):
    ks = w["ks"][1:3] + w["ks"][3:]
    out = pyoracle.rotate_hoisted(cut(w["cts"][0], level), ks, [w["keys"][k] for k in ks], w["qs"],
                                  w["ps"], DNUM, LOG_N, level=level, ntt=NTT)
    return [(o, sigma_int(w["msgs"][0], k)) for o, k in zip(out, ks)]


def op_rotate_sum_hoisted(w, level):
    ks = w["ks"]
    out = pyoracle.rotate_sum_hoisted(cut(w["cts"][0], level), ks, [w["keys"].get(k) for k in ks],
                                      w["pts"], w["qs"], w["ps"], DNUM, LOG_N, level=level, ntt=NTT)
    expect = [0] * N
    for k, p in zip(ks, w["pt_int"]):
        expect = add_int(expect, negacyclic_int(p, sigma_int(w["msgs"][0], k)))
    return [(out, expect)]


def op_rotate_sum_multi(w, level):
    ks = [w["ks"][1], 1, w["ks"][3]]
    out = pyoracle.rotate_sum_multi([cut(c, level) for c in w["cts"]], ks,
                                    [w["keys"].get(k) for k in ks], w["qs"], w["ps"], DNUM, LOG_N,
                                    level=level, ntt=NTT)
    expect = [0] * N
    for k, m in zip(ks, w["msgs"]):
        expect = add_int(expect, sigma_int(m, k))
    return [(out, expect)]


def op_linear_transform(w, level):
    baby, giant = [1, w["ks"][1]], [1, w["ks"][2]]
    pts = [w["pts"][:2], w["pts"][2:]]
    out = pyoracle.linear_transform(cut(w["cts"][0], level), baby,
                                    [w["keys"].get(k) for k in baby], giant,
                                    [w["keys"].get(k) for k in giant], pts, w["qs"], w["ps"], DNUM,
                                    LOG_N, level=level, ntt=NTT)
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


def _pinned():
    with open(os.path.join(os.path.dirname(__file__), "golden", "level_refs.json")) as f:
        return json.load(f)


def test_every_operation_at_every_level_is_what_the_parent_of_the_unification_computed(world):
    """tests/golden/level_refs.json holds the SHA-256 of every result of the key-switch family at
    every level on this file's world and on the two shapes of tests/test_levels_cpu.py, computed
    before pyoracle took level= by the two sets of functions it replaced
    (tests/golden/make_golden.py level_refs).  The unified functions must reproduce each: with the C transforms everywhere, and
    at log_n = 6 with ntt=None as well, the pure-Python definition."""
    want = _pinned()
    got = refs.level_digests(world, pyoracle, NTT)
    for shape in refs.PIN_SMALL:
        small = refs.small_world(*shape)
        pure = refs.level_digests(small, pyoracle, None)
        assert refs.level_digests(small, pyoracle, NTT) == pure, shape
        got.update(pure)
    assert got.keys() == want.keys()
    assert [k for k in want if got[k] != want[k]] == []


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
    w, level, dn = world, 4, 2
    assert pyoracle.digit_ranges(L, DNUM, level) == pyoracle.digit_ranges(level, dn)
    rows = pyoracle.key_rows(level, L, K)
    ks = w["ks"]
    first = w["keys"][ks[1]]
    kb = np.stack([(w["keys"].get(k) or first)[0] for k in ks])[:, :dn][:, :, rows]
    ka = np.stack([(w["keys"].get(k) or first)[1] for k in ks])[:, :dn][:, :, rows]
    pts = np.stack(w["pts"])[:, rows]
    ct = cut(w["cts"][0], level)
    want = coracle.rotate_sum_hoisted(ct, ks, np.ascontiguousarray(kb), np.ascontiguousarray(ka),
                                      np.ascontiguousarray(pts), w["qs"][:level], w["ps"], dn)
    got = pyoracle.rotate_sum_hoisted(ct, ks, [w["keys"].get(k) for k in ks], w["pts"], w["qs"],
                                      w["ps"], DNUM, LOG_N, level=level, ntt=NTT)
    assert (got == want.astype(object)).all()
