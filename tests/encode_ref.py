"""Reference for the device CKKS encoder / decoder (fhe_encode / fhe_decode; include/fhecore.h):
the HEAAN / Lattigo special FFT over the rotation group, restated in numpy with the butterfly
network and the float64 rounding fixed, so that the device agrees with it bit for bit.

n = N/2 slots, M = 2N, rot[j] = 5^j mod M, W[k] = (cos, sin)(math.pi * k / N) for k < M, every
entry straight from libm.  One complex product (dr, di) (wr, wi) is the four rounded products
dr wr, di wi, dr wi, di wr and the two rounded sums p1 - p2, p3 + p4: real and imaginary parts
live in separate float64 arrays and every product and sum is its own numpy operation (numpy's
complex multiply may fuse).

    encode   v = z;  for len = n, n/2 .. 2 (lh = len/2, lq = 4 len):
                 w = W[(lq - rot[j] % lq) (M/lq)];  (a, b) -> (a + b, (a - b) w)
             v = v[bitrev];  s = delta / n;  c[k] = rint(Re v[k] s), c[k + n] = rint(Im v[k] s)
             row r = NTT_limb(c mod q_limb), canonical
    decode   x_i = INTT_i(limb i), i < min(level, 2);  V = the value centred over q_0 (q_0 q_1);
             x = float(V) (one rounding);  v[k] = (x[k], x[k + n]);  v = v[bitrev]
             for len = 2, 4 .. n:  w = W[(rot[j] % lq) (M/lq)];  (a, b) -> (a + b w, a - b w)
             z = v / delta
"""
import math

import numpy as np

import coracle

_TABLES = {}


def roots(log_n):
    """(cos, sin) [2N] float64 each, entry k = math.cos / math.sin of math.pi * k / N."""
    n = 1 << log_n
    a = [math.pi * k / n for k in range(2 * n)]
    return (np.array([math.cos(x) for x in a], dtype=np.float64),
            np.array([math.sin(x) for x in a], dtype=np.float64))


def _tables(log_n):
    if log_n not in _TABLES:
        n = 1 << log_n
        rot = np.empty(n // 2, dtype=np.int64)
        e = 1
        for j in range(n // 2):
            rot[j] = e
            e = e * 5 % (2 * n)
        ln = log_n - 1
        idx = np.arange(n // 2)
        rev = np.zeros(n // 2, dtype=np.int64)
        for b in range(ln):
            rev |= ((idx >> b) & 1) << (ln - 1 - b)
        _TABLES[log_n] = (roots(log_n), rot, rev)
    return _TABLES[log_n]


def special_ifft(re, im, log_n):
    """(..., N/2) float64 pairs -> the same, before the 1/n scaling (encode's direction)."""
    (wc, ws), rot, rev = _tables(log_n)
    n = 1 << (log_n - 1)
    m = 4 * n
    re = np.array(re, dtype=np.float64)
    im = np.array(im, dtype=np.float64)
    shape = re.shape
    ln = n
    while ln >= 2:
        lh, lq = ln // 2, 4 * ln
        k = (lq - rot[:lh] % lq) * (m // lq)
        wr, wi = wc[k], ws[k]
        r = re.reshape(*shape[:-1], n // ln, 2, lh)
        i = im.reshape(*shape[:-1], n // ln, 2, lh)
        ar, ai, br, bi = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        sr = ar + br
        si = ai + bi
        dr = ar - br
        di = ai - bi
        p1 = dr * wr
        p2 = di * wi
        p3 = dr * wi
        p4 = di * wr
        re = np.stack([sr, p1 - p2], axis=-2).reshape(shape)
        im = np.stack([si, p3 + p4], axis=-2).reshape(shape)
        ln //= 2
    return re[..., rev], im[..., rev]


def special_fft(re, im, log_n):
    """(..., N/2) float64 pairs -> the same (decode's direction)."""
    (wc, ws), rot, rev = _tables(log_n)
    n = 1 << (log_n - 1)
    m = 4 * n
    re = np.array(re, dtype=np.float64)[..., rev]
    im = np.array(im, dtype=np.float64)[..., rev]
    shape = re.shape
    ln = 2
    while ln <= n:
        lh, lq = ln // 2, 4 * ln
        k = (rot[:lh] % lq) * (m // lq)
        wr, wi = wc[k], ws[k]
        r = re.reshape(*shape[:-1], n // ln, 2, lh)
        i = im.reshape(*shape[:-1], n // ln, 2, lh)
        ar, ai, yr, yi = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        p1 = yr * wr
        p2 = yi * wi
        p3 = yr * wi
        p4 = yi * wr
        br = p1 - p2
        bi = p3 + p4
        re = np.stack([ar + br, ar - br], axis=-2).reshape(shape)
        im = np.stack([ai + bi, ai - bi], axis=-2).reshape(shape)
        ln *= 2
    return re, im


def encode_coeffs(z, delta, log_n):
    """z (..., N/2) complex -> signed int64 coefficients (..., N); |c| < 2^62 is the caller's."""
    z = np.asarray(z, dtype=np.complex128)
    n = 1 << (log_n - 1)
    assert z.shape[-1] == n
    re, im = special_ifft(z.real, z.imag, log_n)
    s = float(delta) / n
    c = np.concatenate([np.rint(re * s), np.rint(im * s)], axis=-1)
    assert np.abs(c).max(initial=0) < 2.0 ** 62
    return c.astype(np.int64)


def rows_limbs(level, special, L, K):
    """The context limb of every row of an encoded plaintext."""
    return list(range(level)) + ([L + k for k in range(K)] if special else [])


def residues(c, qs):
    """Signed coefficients (..., N) -> canonical residues (..., len(qs), N) uint64."""
    c = np.asarray(c).astype(object)
    return np.stack([(c % int(q)).astype(np.uint64) for q in qs], axis=-2)


def encode(z, delta, log_n, qs):
    """z (..., N/2) -> NTT-form rows (..., len(qs), N) uint64 over the moduli qs (the caller
    picks the rows' limbs: rows_limbs)."""
    qs = [int(q) for q in qs]
    return coracle.ntt_fwd(residues(encode_coeffs(z, delta, log_n), qs), qs).astype(np.uint64)


def centred(pt, qs, level):
    """pt (..., rows >= min(level, 2), N) NTT form -> the centred value V as Python integers
    (..., N): over q_0 at level 1, over q_0 q_1 above."""
    pt = np.asarray(pt)
    q0 = int(qs[0])
    x0 = coracle.ntt_inv(pt[..., :1, :].astype(np.uint64), [q0])[..., 0, :].astype(object)
    if level == 1:
        return np.where(x0 <= (q0 - 1) // 2, x0, x0 - q0)
    q1 = int(qs[1])
    x1 = coracle.ntt_inv(pt[..., 1:2, :].astype(np.uint64), [q1])[..., 0, :].astype(object)
    t = ((x1 - x0 % q1) * pow(q0 % q1, -1, q1)) % q1
    v = x0 + q0 * t
    return np.where(v <= (q0 * q1 - 1) // 2, v, v - q0 * q1)


def decode_coeffs(x, delta, log_n):
    """x (..., N) float64 coefficients -> complex slots (..., N/2)."""
    x = np.asarray(x, dtype=np.float64)
    n = 1 << (log_n - 1)
    re, im = special_fft(x[..., :n], x[..., n:], log_n)
    d = np.float64(delta)
    z = np.empty(re.shape, dtype=np.complex128)
    z.real = re / d
    z.imag = im / d
    return z


def decode(pt, delta, log_n, qs, level):
    """pt (..., rows, N) NTT form -> complex slots (..., N/2); float(V) rounds to nearest even."""
    v = centred(pt, qs, level)
    x = np.array([float(int(a)) for a in v.reshape(-1)], dtype=np.float64).reshape(v.shape)
    return decode_coeffs(x, delta, log_n)
