"""Reference for sparse packing (fhe_encode_sparse / fhe_decode_sparse, SubSum and the sparse path
of fhecore.bootstrap): n_s = 2^log_slots slots, gap = N / (2 n_s), the message a polynomial in
Y = X^gap.  (pyoracle.sparse_secret_coefficients is the sparse *secret*; this is about packing.)

    encode   encode_ref.encode of the vector tiled gap times: an n_s-periodic slot vector has no
             coefficient off the multiples of gap, and the tiled transform's first log2(gap) stages
             only double, so this is the size-n_s transform placed on the grid, bit for bit
    decode   the centred value of the grid coefficients only (the projection onto the subring),
             then encode_ref.decode_coeffs of the ring of degree 2 n_s
    subsum   acc = t; acc <- acc + sigma_{5^(n_s 2^i)}(acc), i < log2(gap), on coefficient vectors
             by signed permutation: gap t[k gap] on the grid, 0 elsewhere

and the parameters of the case the CPU and GPU bootstrap tests share (tests/cases.py SPARSE):
bootstrap_ref's chain, secret and parameters at N = 2^10 with log_slots = 6 (gap 8: three SubSum
steps), 64 slots uniform in the square encoded at bootstrap_ref's message ratio (IN_SCALE)."""
import numpy as np

import bootstrap_ref as br
import encode_ref
import pyoracle

LOG_SLOTS = 6
PARAMS = dict(br.PARAMS, log_slots=LOG_SLOTS)
# The scale the case's input is encoded at.  What EvalMod sees is the message ratio |m_k| / q_0 of
# the coefficients, and at one scale s and one slot magnitude a plaintext of n_s slots has
# coefficients of size s / sqrt(n_s): sqrt(gap) times full packing's.  Encoded at delta like
# bootstrap_ref's 512 slots, these 64 would meet EvalMod's cubic term (2 pi)^2 (m / q_0)^3 / 6 with
# gap^(3/2) per coefficient, summed over 2 n_s coefficients and not N (sqrt(gap) less): about
# gap = 8 times the slot error, whatever the packing of the bootstrap that refreshes them
# (cubic_term below: 1.975e-4 against 2.87e-5, no ciphertext involved).  A sparse input keeps
# bootstrap_ref's message ratio when it is encoded at delta / sqrt(gap); the Bootstrapper takes any
# input scale and returns it.
IN_SCALE = br.DELTA / float(np.sqrt(1 << (br.LOG_N - 1 - LOG_SLOTS)))


def gap(log_n, log_slots):
    assert 0 <= log_slots <= log_n - 1
    return 1 << (log_n - 1 - log_slots)


def tiled(z, log_n, log_slots):
    z = np.asarray(z, dtype=np.complex128)
    assert z.shape[-1] == 1 << log_slots
    return np.tile(z, gap(log_n, log_slots))


def encode_coeffs(z, delta, log_n, log_slots):
    return encode_ref.encode_coeffs(tiled(z, log_n, log_slots), delta, log_n)


def encode(z, delta, log_n, log_slots, qs):
    """z (..., n_s) -> NTT-form rows (..., len(qs), N): encode_ref.encode of the tiled vector."""
    return encode_ref.encode(tiled(z, log_n, log_slots), delta, log_n, qs)


def decode(pt, delta, log_n, log_slots, qs, level):
    """pt (..., rows, N) NTT form -> complex slots (..., n_s), from the grid coefficients only."""
    v = encode_ref.centred(pt, qs, level)[..., ::gap(log_n, log_slots)]
    x = np.array([float(int(a)) for a in v.reshape(-1)], dtype=np.float64).reshape(v.shape)
    return encode_ref.decode_coeffs(x, delta, log_slots + 1)


def automorphism(c, elt):
    """sigma_elt on signed coefficient vectors (..., N): X^i -> X^(i elt), X^N = -1."""
    c = np.asarray(c)
    n = c.shape[-1]
    at = np.arange(n) * elt % (2 * n)
    out = np.zeros_like(c)
    out[..., at % n] = np.where(at >= n, -c, c)
    return out


def subsum(t, log_slots):
    """The trace onto the subring of Y = X^gap, by log2(gap) automorphisms and additions."""
    acc = np.asarray(t)
    n = acc.shape[-1]
    log_n = n.bit_length() - 1
    for i in range(log_n - 1 - log_slots):
        acc = acc + automorphism(acc, pyoracle.galois_elt((1 << log_slots) << i, n))
    return acc


def cubic_term(z, delta, q0, log_slots):
    """Maximum slot error of replacing every encoded coefficient m by q_0 sin(2 pi m / q_0) / 2 pi:
    what an exact EvalMod leaves of the slots z, with no noise."""
    c = encode_ref.encode_coeffs(z, delta, log_slots + 1).astype(np.float64)
    e = q0 * np.sin(2 * np.pi * c / q0) / (2 * np.pi)
    return float(np.abs(encode_ref.decode_coeffs(e, delta, log_slots + 1) - z).max())


# ---- the shared case's rotation keys (the case itself: tests/cases.py SPARSE) ---------------------

def rotation_elements(log_slots=LOG_SLOTS):
    """The Galois elements of the SubSum steps, of every baby / giant step of the six small
    factors (taken on the full ring) and of the conjugation."""
    from fhecore import bootstrap as bs

    n = 1 << br.LOG_N
    steps = {(1 << log_slots) << i for i in range(br.LOG_N - 1 - log_slots)}
    for inverse, groups in ((True, PARAMS["cts_groups"]), (False, PARAMS["stc_groups"])):
        for n1, n2, stride, offset in bs.factor_layouts(br.LOG_N, groups, inverse, log_slots):
            steps |= {stride * (b + offset) for b in range(n1)} | {stride * g * n1 for g in range(n2)}
    return sorted({pyoracle.galois_elt(s, n) for s in steps if s} | {2 * n - 1})
