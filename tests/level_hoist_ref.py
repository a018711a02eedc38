"""Reference for the hoisted rotations, the rotation sums and the BSGS linear transform below the
top level (fhe_rotate_hoisted_level, fhe_rotate_sum_hoisted_level, fhe_rotate_sum_multi_level,
fhe_linear_transform_level; include/fhecore.h): pyoracle.rotate_hoisted, rotate_sum_hoisted,
rotate_sum_multi and linear_transform restated for the first `level` Q-limbs of a chain of L under
the rule of tests/level_ref.py:
  * Q-limbs 0 .. l-1, digits level_ref.level_digits (the top-level width, the last one cut at l),
  * the keys (dnum, L + K, N) and the plaintext diagonals (L + K, N) are the top-level tensors, read
    at the rows level_ref.key_rows = {0 .. l-1} u {L .. L+K-1} (a diagonal is an integer polynomial:
    its residues do not depend on the level),
  * everything else word for word: the own digit's rows are c1 itself, the unrotated term adds
    pt (P mod q_i) c1 into A1's Q rows (the multiplied form) or c0, c1 directly (the multi form),
    one ModDown per accumulator.
NTTs through coracle, object arrays."""
import math

import numpy as np

import level_ref
import pyoracle
from level_ref import _fwd, _inv, _moddown


def _setup(qs, ps, level):
    qs, ps = [int(q) for q in qs], [int(p) for p in ps]
    ql = qs[:level]
    return qs, ps, ql, ql + ps, level_ref.key_rows(level, len(qs), len(ps))


def ext_digits(c1, qs, ps, dnum, level):
    """ModUp of c1 (level, N) NTT form: the live digits, each (level + K, N) NTT form over
    ql u ps, the digit's own rows c1 itself."""
    qs, ps, ql, allm, _ = _setup(qs, ps, level)
    c1 = np.asarray(c1).astype(object)
    c = _inv(c1, ql)
    out = []
    for lo, hi in level_ref.level_digits(level, len(qs), dnum):
        others = [i for i in range(level + len(ps)) if not lo <= i < hi]
        conv = pyoracle.baseconv(c[lo:hi], ql[lo:hi], [allm[i] for i in others])
        ext = np.empty((level + len(ps), c.shape[-1]), dtype=object)
        ext[lo:hi] = c[lo:hi]
        for k, i in enumerate(others):
            ext[i] = conv[k]
        en = _fwd(ext, allm)
        en[lo:hi] = c1[lo:hi]
        out.append(en)
    return out


def _inner(ext, idx, rot_b, rot_a, rows, mods):
    """The gathered inner product of the live digits with the key rows `rows`."""
    acc0 = np.zeros(ext[0].shape, dtype=object)
    acc1 = np.zeros_like(acc0)
    for j, e in enumerate(ext):
        g = e[..., idx]
        acc0 = (acc0 + g * np.asarray(rot_b[j])[rows].astype(object)) % mods
        acc1 = (acc1 + g * np.asarray(rot_a[j])[rows].astype(object)) % mods
    return acc0, acc1


def rotate_hoisted(ct, ks, keys, qs, ps, dnum, level, log_n):
    """ct (2, level, N) -> [len(ks), 2, level, N]."""
    qs, ps, ql, allm, rows = _setup(qs, ps, level)
    ct = np.asarray(ct).astype(object)
    ext = ext_digits(ct[1], qs, ps, dnum, level)
    mods, col = pyoracle._mods_col(allm), pyoracle._mods_col(ql)
    out = []
    for k, (rot_b, rot_a) in zip(ks, keys):
        idx = pyoracle.automorphism_ntt_index(int(k), log_n)
        acc0, acc1 = _inner(ext, idx, rot_b, rot_a, rows, mods)
        out.append(np.stack([(ct[0][..., idx] + _moddown(acc0, ql, ps)) % col,
                             _moddown(acc1, ql, ps)]))
    return np.stack(out)


def rotate_sum_hoisted(ct, ks, keys, pts, qs, ps, dnum, level, log_n):
    """ct (2, level, N), pts[r] (L + K, N) -> (2, level, N)."""
    qs, ps, ql, allm, rows = _setup(qs, ps, level)
    P = math.prod(ps)
    ct = np.asarray(ct).astype(object)
    c0, c1 = ct[0], ct[1]
    n = c1.shape[-1]
    mods, col = pyoracle._mods_col(allm), pyoracle._mods_col(ql)
    ext = ext_digits(c1, qs, ps, dnum, level) if any(int(k) != 1 for k in ks) else None
    a0 = np.zeros((len(allm), n), dtype=object)
    a1 = np.zeros_like(a0)
    s0 = np.zeros((level, n), dtype=object)
    pcol = np.array([P % q for q in ql], dtype=object).reshape(-1, 1)
    for k, key, pt in zip(ks, keys, pts):
        k = int(k)
        pt = np.asarray(pt)[rows].astype(object)
        if k == 1:
            s0 = (s0 + pt[:level] * c0) % col
            a1[:level] = (a1[:level] + pt[:level] * (pcol * c1 % col)) % col
            continue
        idx = pyoracle.automorphism_ntt_index(k, log_n)
        acc0, acc1 = _inner(ext, idx, key[0], key[1], rows, mods)
        a0 = (a0 + pt * acc0) % mods
        a1 = (a1 + pt * acc1) % mods
        s0 = (s0 + pt[:level] * c0[..., idx]) % col
    return np.stack([(s0 + _moddown(a0, ql, ps)) % col, _moddown(a1, ql, ps)])


def rotate_sum_multi(cts, ks, keys, qs, ps, dnum, level, log_n):
    """cts[r] (2, level, N) -> (2, level, N)."""
    qs, ps, ql, allm, rows = _setup(qs, ps, level)
    mods, col = pyoracle._mods_col(allm), pyoracle._mods_col(ql)
    n = np.asarray(cts[0]).shape[-1]
    a0 = np.zeros((len(allm), n), dtype=object)
    a1 = np.zeros_like(a0)
    s0 = np.zeros((level, n), dtype=object)
    s1 = np.zeros_like(s0)
    for ct, k, key in zip(cts, ks, keys):
        k = int(k)
        c0 = np.asarray(ct[0]).astype(object)
        c1 = np.asarray(ct[1]).astype(object)
        if k == 1:
            s0 = (s0 + c0) % col
            s1 = (s1 + c1) % col
            continue
        idx = pyoracle.automorphism_ntt_index(k, log_n)
        acc0, acc1 = _inner(ext_digits(c1, qs, ps, dnum, level), idx, key[0], key[1], rows, mods)
        a0 = (a0 + acc0) % mods
        a1 = (a1 + acc1) % mods
        s0 = (s0 + c0[..., idx]) % col
    return np.stack([(s0 + _moddown(a0, ql, ps)) % col, (s1 + _moddown(a1, ql, ps)) % col])


def linear_transform(ct, baby, baby_keys, giant, giant_keys, pts, qs, ps, dnum, level, log_n):
    """sum_g rot_{giant[g]}(sum_b pts[g][b] rot_{baby[b]}(ct)): the inner sums rotate_sum_hoisted,
    the outer one rotate_sum_multi."""
    inner = [rotate_sum_hoisted(ct, baby, baby_keys, row, qs, ps, dnum, level, log_n)
             for row in pts]
    return rotate_sum_multi(inner, giant, giant_keys, qs, ps, dnum, level, log_n)
