"""Reference for ModRaise (fhe_mod_raise; include/fhecore.h) in exact Python integers over object
arrays, written from its definition: for every polynomial p and limb l < out_level

    x = INTT_0(in[p][0])                        coefficient form, 0 <= x < q_0
    c = x if x <= (q_0 - 1) / 2, else x - q_0   the centred representative
    out[p][l] = NTT_l(c mod q_l)                canonical residues

The NTTs are the oracle's (coracle, pinned against pyoracle in tests/test_oracle.py); the lift
and the reduction are Python-integer arithmetic."""
import numpy as np

import coracle


def centred_lift(ct, qs):
    """ct (..., l >= 1, N) NTT form -> the centred coefficients c of limb 0, (..., N) Python
    integers with |c| <= (q_0 - 1) / 2."""
    q0 = int(qs[0])
    x = coracle.ntt_inv(np.asarray(ct)[..., :1, :].astype(np.uint64), [q0])[..., 0, :].astype(object)
    return np.where(x <= (q0 - 1) // 2, x, x - q0)


def mod_raise(ct, qs, in_level, out_level):
    """ct (..., in_level, N) NTT form, canonical residues -> (..., out_level, N) object array."""
    ct = np.asarray(ct)
    assert ct.shape[-2] == in_level and 1 <= in_level <= len(qs) and 1 <= out_level <= len(qs)
    ql = [int(q) for q in qs[:out_level]]
    c = centred_lift(ct, qs)
    res = np.stack([(c % q).astype(np.uint64) for q in ql], axis=-2)
    return coracle.ntt_fwd(res, ql).astype(object)
