"""Reference for the real / imaginary split and merge (fhe_conj_split_level / fhe_conj_merge_level;
include/fhecore.h), defined in COEFFICIENT form so that it checks the library's NTT-domain rule
(the constant psi^(N/2) on the first half of a row, its negative on the second) instead of
restating it: X^(N/2) p is the negacyclic shift of p's coefficients by N/2,

    (X^(N/2) p)[i + N/2] = p[i]   (i < N/2),      (X^(N/2) p)[i - N/2] = -p[i]   (i >= N/2).

    split:  re = ct + cc,   im = -X^(N/2) (ct - cc)
    merge:  out = a + X^(N/2) b

Operands (..., l, N) NTT form over the first l moduli; NTTs through coracle."""
import numpy as np

import coracle
import pyoracle


def _col(ql):
    return pyoracle._mods_col(ql)


def mul_x_half(x, ql):
    """X^(N/2) x for x (..., l, N) NTT form, canonical residues -> the same, object array."""
    c = coracle.ntt_inv(np.asarray(x).astype(np.uint64), ql).astype(object)
    h = c.shape[-1] // 2
    y = np.concatenate([-c[..., h:], c[..., :h]], axis=-1) % _col(ql)
    return coracle.ntt_fwd(y.astype(np.uint64), ql).astype(object)


def conj_split(ct, cc, qs, level):
    ql = [int(q) for q in qs[:level]]
    ct, cc = np.asarray(ct).astype(object), np.asarray(cc).astype(object)
    re = (ct + cc) % _col(ql)
    im = (-mul_x_half((ct - cc) % _col(ql), ql)) % _col(ql)
    return re, im


def conj_merge(a, b, qs, level):
    ql = [int(q) for q in qs[:level]]
    return (np.asarray(a).astype(object) + mul_x_half(b, ql)) % _col(ql)
