"""Reference for the fixed-Hamming-weight secret (fhe_keygen_secret_sparse; include/fhecore.h),
written from its definition with pyoracle's Philox and numpy's argsort:

    r_c = philox4x32_10((c, 0xffffffff, 0, TAG), seed),   key_c = (r_c.x << 32) | c
    the h coefficients with the smallest keys are nonzero: +1 if (r_c.y & 1) == 0, else -1

The keys are distinct (their low words are), so the set does not depend on how it is found."""
import numpy as np

import pyoracle

TAG = 4  # distinct from pyoracle.TAG's values


def coefficients(seed, h, log_n):
    """The secret's signed coefficients, int64 [N] with exactly h entries of +-1."""
    n = 1 << log_n
    assert TAG not in pyoracle.TAG.values() and 1 <= h <= n
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    draws = [pyoracle.philox4x32_10((c, 0xFFFFFFFF, 0, TAG), k0, k1) for c in range(n)]
    keys = np.array([(x << 32) | c for c, (x, _, _, _) in enumerate(draws)], dtype=np.uint64)
    s = np.zeros(n, dtype=np.int64)
    for c in np.argsort(keys)[:h]:
        s[c] = 1 if draws[c][1] & 1 == 0 else -1
    return s


def keygen_secret_sparse(seed, h, allm, log_n):
    """sk [L + K][N] in NTT form (object array), the layout of pyoracle.keygen_secret."""
    s = [int(v) for v in coefficients(seed, h, log_n)]
    return pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, allm), allm)
