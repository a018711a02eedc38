"""Reference for the level-aware key-switch, multiply-relinearise and rotation (fhe_*_level,
include/fhecore.h): the oracle's hybrid key-switch restated for the first `level` Q-limbs of a chain
of L, with the truncated digit ranges written out.

The key is the top-level key (dnum, L + K, N), unchanged: its gadget factor P g_j is P mod q_i on the
limbs of digit j and 0 on the other Q-limbs whatever the number of live limbs, so level l uses
  * Q-limbs 0 .. l-1,
  * digits D_j = [j alpha, min(l, (j + 1) alpha)) for j < ceil(l / alpha), alpha = ceil(L / dnum) the
    top-level digit width,
  * key rows {0 .. l-1} u {L .. L+K-1} of those digits.
Composed from pyoracle primitives (baseconv, tensor_ntt, rescale_coeff, automorphism_ntt); the NTTs
go through coracle (the C restatement, bit-identical to pyoracle.rns_ntt_*) for speed."""
import math

import numpy as np

import coracle
import pyoracle


def _fwd(x, mods):
    return coracle.ntt_fwd(np.asarray(x, dtype=np.uint64), mods).astype(object)


def _inv(x, mods):
    return coracle.ntt_inv(np.asarray(x, dtype=np.uint64), mods).astype(object)


def alpha_of(L, dnum):
    return -(-L // dnum)


def level_digits(level, L, dnum):
    """Digit ranges of level `level`: the top-level width, the last one cut at `level`."""
    a = alpha_of(L, dnum)
    return [(lo, min(level, lo + a)) for lo in range(0, level, a)]


def key_rows(level, L, K):
    """Rows of one digit of the top-level key that level `level` reads."""
    return list(range(level)) + list(range(L, L + K))


def _moddown(acc, ql, ps):
    """pyoracle.moddown_ntt with the C NTTs: (acc_Q - NTT(conv_{P->Q}(INTT acc_P))) P^-1."""
    l = len(ql)
    conv = _fwd(pyoracle.baseconv(_inv(acc[l:], ps), ps, ql), ql)
    P = math.prod(ps)
    return np.stack([(acc[i] - conv[i]) * pow(P % q, -1, q) % q for i, q in enumerate(ql)])


def keyswitch_level(d2, evk_b, evk_a, qs, ps, dnum, level):
    """d2 (level, N) NTT form over qs[:level]; evk_b / evk_a (dnum, L + K, N), the top-level key
    -> (ks0, ks1), each (level, N) NTT form, object arrays."""
    qs, ps = [int(q) for q in qs], [int(p) for p in ps]
    L, K = len(qs), len(ps)
    ql = qs[:level]
    allm = ql + ps
    rows = key_rows(level, L, K)
    mods = pyoracle._mods_col(allm)
    c = _inv(d2, ql)
    acc0 = np.zeros((level + K, c.shape[-1]), dtype=object)
    acc1 = np.zeros_like(acc0)
    for j, (lo, hi) in enumerate(level_digits(level, L, dnum)):
        others = [i for i in range(level + K) if not lo <= i < hi]
        conv = pyoracle.baseconv(c[lo:hi], ql[lo:hi], [allm[i] for i in others])
        ext = np.empty((level + K, c.shape[-1]), dtype=object)
        ext[lo:hi] = c[lo:hi]
        for k, i in enumerate(others):
            ext[i] = conv[k]
        en = _fwd(ext, allm)
        acc0 = (acc0 + en * np.asarray(evk_b[j])[rows].astype(object)) % mods
        acc1 = (acc1 + en * np.asarray(evk_a[j])[rows].astype(object)) % mods
    return _moddown(acc0, ql, ps), _moddown(acc1, ql, ps)


def rescale_ntt(x, ql):
    """pyoracle.rescale_ntt with the C NTTs: (l, N) NTT form -> (l - 1, N)."""
    return _fwd(pyoracle.rescale_coeff(_inv(x, ql), ql), ql[:-1])


def mul_relin_level(a, b, evk_b, evk_a, qs, ps, dnum, level, rescale):
    """a, b (2, level, N) NTT form -> Relin(a x b) (2, level, N), or rescaled (2, level - 1, N)."""
    ql = [int(q) for q in qs[:level]]
    d = pyoracle.tensor_ntt(np.asarray(a).astype(object), np.asarray(b).astype(object), ql)
    ks0, ks1 = keyswitch_level(d[2], evk_b, evk_a, qs, ps, dnum, level)
    col = pyoracle._mods_col(ql)
    out = np.stack([(d[0] + ks0) % col, (d[1] + ks1) % col])
    if rescale:
        out = np.stack([rescale_ntt(out[0], ql), rescale_ntt(out[1], ql)])
    return out


def rotate_level(ct, k, rot_b, rot_a, qs, ps, dnum, level, log_n):
    """ct (2, level, N) NTT form -> (sigma_k c0 + KS0(sigma_k c1), KS1(sigma_k c1))."""
    ql = [int(q) for q in qs[:level]]
    ct = np.asarray(ct).astype(object)
    c0 = pyoracle.automorphism_ntt(ct[0], k, log_n)
    c1 = pyoracle.automorphism_ntt(ct[1], k, log_n)
    ks0, ks1 = keyswitch_level(c1, rot_b, rot_a, qs, ps, dnum, level)
    col = pyoracle._mods_col(ql)
    return np.stack([(c0 + ks0) % col, ks1 % col])
