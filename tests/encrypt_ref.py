"""Reference for batched encryption at any level (fhe_encrypt_level, fhe_encrypt_sk_level;
include/fhecore.h): the Philox draws of oracle/pyoracle.py restated over numpy uint64 arrays (one
array operation per round instead of one Python call per coefficient), and the two definitions

    public key   ct[i][0][l] = NTT_l(e0) + pk[0][l] NTT_l(u) + pt_i[l]
                 ct[i][1][l] = NTT_l(e1) + pk[1][l] NTT_l(u)
    secret key   ct[i][1][l] = a[l],   ct[i][0][l] = NTT_l(e) - a[l] s[l] + pt_i[l]

with ciphertext i drawing at poly j = index0 + i.  The transforms and the modular products are
coracle's (exact); nothing here depends on the library under test.  tests/test_encrypt_cpu.py ties
the vectorised draws to pyoracle.philox4x32_10 / pyoracle.sample and the definitions to
pyoracle.encrypt / encrypt_sk."""
import numpy as np

import coracle
from pyoracle import TAG

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) (broadcast against each other) under the key
    (k0, k1): four uint64 arrays holding 32-bit words."""
    x, y, z, w = (np.asarray(v, dtype=np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x, np.uint64(0xCD9E8D57) * z  # 32 x 32 bits: no wrap
        x, y, z, w = (p1 >> _S32) ^ y ^ k0, p1 & _M32, (p0 >> _S32) ^ w ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return x, y, z, w


def _popcount(v):
    v = v - ((v >> np.uint64(1)) & np.uint64(0x5555555555555555))
    v = (v & np.uint64(0x3333333333333333)) + ((v >> np.uint64(2)) & np.uint64(0x3333333333333333))
    v = (v + (v >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return (v * np.uint64(0x0101010101010101)) >> np.uint64(56)


def _mulhi(a, b):
    """The high 64 bits of the 128-bit products a * b (uint64 arrays)."""
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)


def sample_small(kind, seed, tag, poly, n):
    """int64 [n]: the ternary or centred-binomial (eta = 21) integers of (seed, tag, poly); the
    same on every limb."""
    x, y, _, _ = philox(np.arange(n, dtype=np.uint64), 0xFFFFFFFF, poly, tag, seed, seed >> 32)
    if kind == "ternary":
        return (x % np.uint64(3)).astype(np.int64) - 1
    assert kind == "error"
    bits = (y << _S32) | x
    m21 = np.uint64(0x1FFFFF)
    return _popcount(bits & m21).astype(np.int64) - _popcount((bits >> np.uint64(21)) & m21).astype(np.int64)


def sample_uniform(seed, tag, poly, limbs, n):
    """uint64 [len(limbs), n]: floor(r q / 2^128) of a 128-bit draw; limbs = [(ctx limb index, q)]."""
    out = np.empty((len(limbs), n), dtype=np.uint64)
    for r, (li, q) in enumerate(limbs):
        x, y, z, w = philox(np.arange(n, dtype=np.uint64), li, poly, tag, seed, seed >> 32)
        lo, hi, q = (y << _S32) | x, (w << _S32) | z, np.uint64(q)
        # (hi q + ((lo q) >> 64)) >> 64: the low words' sum carries into the high word
        low = hi * q
        t = low + _mulhi(lo, q)
        out[r] = _mulhi(hi, q) + (t < low).astype(np.uint64)
    return out


def sample(kind, seed, tag, poly, limbs, n):
    """pyoracle.sample's result as uint64 [len(limbs), n]."""
    if kind == "uniform":
        return sample_uniform(seed, tag, poly, limbs, n)
    return residues(sample_small(kind, seed, tag, poly, n), [q for _, q in limbs])


def residues(v, qs):
    """int64 [n] -> canonical residues uint64 [len(qs), n]."""
    return np.stack([(v % np.int64(q)).astype(np.uint64) for q in qs])


def _pt_rows(pt, i, level):
    if pt is None:
        return None
    pt = np.asarray(pt, dtype=np.uint64)
    if pt.ndim == 2:
        pt = pt[None]
    return np.ascontiguousarray(pt[i if pt.shape[0] > 1 else 0][:level])


def encrypt(seed, pt, pk, qs, log_n, level=None, batch=1, index0=0):
    """uint64 [batch, 2, level, N].  pk [2, L, N]; pt None, [rows, N] or [pt_batch, rows, N] with
    rows >= level and pt_batch 1 or batch; qs the context's L Q-primes."""
    n = 1 << log_n
    level = len(qs) if level is None else level
    ql = [int(q) for q in qs[:level]]
    pk = np.asarray(pk, dtype=np.uint64)
    out = np.empty((batch, 2, level, n), dtype=np.uint64)
    for i in range(batch):
        j = index0 + i
        u = coracle.ntt_fwd(residues(sample_small("ternary", seed, TAG["enc_u"], j, n), ql), ql)
        e0 = coracle.ntt_fwd(residues(sample_small("error", seed, TAG["enc_e0"], j, n), ql), ql)
        e1 = coracle.ntt_fwd(residues(sample_small("error", seed, TAG["enc_e1"], j, n), ql), ql)
        c0 = coracle.vec_op("add", e0, coracle.vec_op("mul", pk[0, :level], u, ql), ql)
        p = _pt_rows(pt, i, level)
        out[i, 0] = c0 if p is None else coracle.vec_op("add", c0, p, ql)
        out[i, 1] = coracle.vec_op("add", e1, coracle.vec_op("mul", pk[1, :level], u, ql), ql)
    return out


def encrypt_sk(seed, pt, sk, qs, log_n, level=None, batch=1, index0=0):
    """uint64 [batch, 2, level, N]; sk [L + K, N] (rows l < level read)."""
    n = 1 << log_n
    level = len(qs) if level is None else level
    ql = [int(q) for q in qs[:level]]
    s = np.ascontiguousarray(np.asarray(sk, dtype=np.uint64)[:level])
    out = np.empty((batch, 2, level, n), dtype=np.uint64)
    for i in range(batch):
        j = index0 + i
        a = sample_uniform(seed, TAG["enc_a"], j, list(enumerate(ql)), n)
        e = coracle.ntt_fwd(residues(sample_small("error", seed, TAG["enc_e"], j, n), ql), ql)
        c0 = coracle.vec_op("sub", e, coracle.vec_op("mul", a, s, ql), ql)
        p = _pt_rows(pt, i, level)
        out[i, 0] = c0 if p is None else coracle.vec_op("add", c0, p, ql)
        out[i, 1] = a
    return out


def decrypt(ct, sk, qs):
    """ct [..., 2, l, N] -> c0 + c1 s over its l limbs, uint64 [..., l, N]."""
    ct = np.asarray(ct, dtype=np.uint64)
    lv = ct.shape[-2]
    ql = [int(q) for q in qs[:lv]]
    flat = ct.reshape(-1, 2, lv, ct.shape[-1])
    s = np.ascontiguousarray(np.asarray(sk, dtype=np.uint64)[:lv])
    out = np.stack([coracle.vec_op("add", np.ascontiguousarray(c[0]),
                                   coracle.vec_op("mul", np.ascontiguousarray(c[1]), s, ql), ql)
                    for c in flat])
    return out.reshape(*ct.shape[:-3], lv, ct.shape[-1])


def noise_limb0(ct, pt, sk, qs):
    """The centred limb-0 coefficients of decrypt(ct) - pt, int64 [..., N]: the ciphertext's
    noise when it is below q_0 / 2.  pt broadcasts against ct's batch shape."""
    q0 = int(qs[0])
    d = decrypt(ct, sk, qs)[..., :1, :]
    if pt is not None:
        p = np.broadcast_to(np.asarray(pt, dtype=np.uint64)[..., :1, :], d.shape)
        d = coracle.vec_op("sub", np.ascontiguousarray(d), np.ascontiguousarray(p), [q0])
    c = coracle.ntt_inv(np.ascontiguousarray(d), [q0])[..., 0, :]
    return np.where(c > np.uint64(q0 // 2), c.astype(np.int64) - np.int64(q0), c.astype(np.int64))


# |noise| bounds from eta = 21 (|e| <= 21) and ternary u, s: public key e0 + e_pk u + e1 s with
# e_pk u and e1 s each a sum of N products of magnitude <= 21; secret key e alone
def noise_bound(log_n, secret):
    return 21 if secret else 21 * (2 * (1 << log_n) + 1)
