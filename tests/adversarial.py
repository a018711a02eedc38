"""Structured inputs for rescale, base conversion and the key-switch family: the values a uniform
draw of 50- to 63-bit residues does not reach (tests/test_adversarial_cpu.py checks that each family
does what it says; tests/test_gpu_adversarial.py runs the kernels on them).

  * rescale_boundary: the dropped residue sits on both sides of the centred lift's wrap
    (csrc/modarith.hpp lift_centred: x = h and x = h + 1, h = (q_last - 1) / 2) and at the ends of
    its range, and a third of the surviving words rescale to exactly 0;
  * conv_worst: every y_i = [x_i (S / s_i)^-1]_{s_i} of the fast base conversion is s_i - 1, the
    top of the sums sum_i y_i ((S / s_i) mod t) of ModUp and ModDown;
  * ks_d2 / ks_keys: key-switch operands at 0 and q - 1, the ModUp worst case, and selector keys
    that make ks1 exactly 0 and steer ks0 = ModDown(NTT(ModUp(digit j))).

numpy and pyoracle only; no state, no side effects on import; everything is a function of its
arguments (the uniform part of rescale_boundary is seeded).  Arrays are uint64 in the layout of the
call they feed."""
import math

import numpy as np

import pyoracle


def _const_rows(vals, n):
    return np.repeat(np.array([int(v) for v in vals], dtype=np.uint64)[:, None], n, axis=1)


def _ntt(x, mods):
    return np.asarray(pyoracle.rns_ntt_fwd(np.asarray(x).astype(object), mods), dtype=np.uint64)


def far_chain():
    """The `far` chain of tests/test_gpu_wide.py, (4 Q moduli, 2 P moduli): primes below 2^60 that
    are not within 1/16 below a power of two (the 8q kernels), q = 1 mod 2^13, so they serve every
    N <= 2^12."""
    step = 2 << 12
    out = []
    for f, b in zip([0.70, 0.80, 0.90, 0.60, 0.75, 0.85], [59, 56, 50, 58, 57, 52]):
        q = (int(f * (1 << b)) - 1) // step * step + 1
        while not pyoracle.is_prime(q):
            q -= step
        out.append(q)
    return out[:4], out[4:]


# ---- rescale ------------------------------------------------------------------------------------

def rescale_edges(q_last):
    """The seven distinct residues of the dropped limb: the ends of [0, q_last), and h - 1 .. h + 2
    around the wrap of the centred lift (x <= h lifts to x, x >= h + 1 to x - q_last)."""
    q_last = int(q_last)
    h = (q_last - 1) // 2
    return [0, 1, h - 1, h, h + 1, h + 2, q_last - 1]


def rescale_boundary(moduli, log_n, polys, seed=0):
    """[polys][l][N] coefficient form over moduli (l >= 2), the last of them dropped by the rescale.

    Last limb: coefficient i of poly p is rescale_edges[(i + p) % 7].  Limb j < l - 1, by
    (i + p) % 3: 0 -> the centred lift of that position's last-limb value mod q_j (the rescaled word
    is exactly 0), 1 -> q_j - 1, 2 -> uniform (seeded).  7 and 3 are coprime, so every edge meets
    every kind of word."""
    moduli = [int(q) for q in moduli]
    l, n = len(moduli), 1 << log_n
    assert l >= 2
    ql = moduli[-1]
    h = ql // 2
    edges = rescale_edges(ql)
    rng = np.random.default_rng(seed)
    out = np.empty((polys, l, n), dtype=np.uint64)
    i = np.arange(n)
    for p in range(polys):
        last = np.array([edges[(k + p) % 7] for k in range(n)], dtype=object)
        out[p, l - 1] = last.astype(np.uint64)
        centred = (last + h) % ql - h  # in [-h, h]
        third = (i + p) % 3
        for j, q in enumerate(moduli[:-1]):
            row = rng.integers(0, q, size=n, dtype=np.uint64)
            row[third == 0] = (centred % q).astype(np.uint64)[third == 0]
            row[third == 1] = q - 1
            out[p, j] = row
    return out


def rescale_boundary_ntt(moduli, log_n, polys, seed=0):
    """rescale_boundary in NTT form: the kernel's own INTT lands on the edge values."""
    return _ntt(rescale_boundary(moduli, log_n, polys, seed), [int(q) for q in moduli])


# ---- base conversion ----------------------------------------------------------------------------

def conv_worst(src, log_n):
    """[len(src)][N] coefficient form: every coefficient of limb i is (s_i - 1) ((S / s_i) mod s_i)
    mod s_i, so that y_i = x_i (S / s_i)^-1 mod s_i = s_i - 1 for every i."""
    src = [int(s) for s in src]
    S = math.prod(src)
    return _const_rows([(s - 1) * ((S // s) % s) % s for s in src], 1 << log_n)


def conv_fraction(src, dst):
    """Per target t: the unreduced sum sum_i (s_i - 1) ((S / s_i) mod t) that conv_worst produces,
    as a fraction of the bound alpha max(s) t the kernels' accumulators are sized for."""
    src = [int(s) for s in src]
    S = math.prod(src)
    return [sum((s - 1) * ((S // s) % int(t)) for s in src) / (len(src) * max(src) * int(t))
            for t in dst]


# ---- key-switch ---------------------------------------------------------------------------------

D2_KINDS = ("zero", "qm1", "modup_worst", "alt")


def ks_d2(kind, qs, ps, dnum, log_n, level=None):
    """[level][N] NTT form over the live Q-limbs qs[:level] (level None: all of qs).
    zero; qm1: q - 1 in every NTT-form word (the largest own-digit operand of the inner product);
    modup_worst: the forward NTT of conv_worst, digit by digit (pyoracle.digit_ranges at the
    level); alt: the forward NTT
    of coefficients alternating 0 and q - 1.  ps is unused (the signature of the call it feeds)."""
    qs = [int(q) for q in qs]
    L = len(qs)
    level = L if level is None else int(level)
    ql, n = qs[:level], 1 << log_n
    if kind == "zero":
        return np.zeros((level, n), dtype=np.uint64)
    if kind == "qm1":
        return _const_rows([q - 1 for q in ql], n)
    if kind == "modup_worst":
        c = np.concatenate([conv_worst(ql[lo:hi], log_n)
                            for lo, hi in pyoracle.digit_ranges(L, dnum, level)])
        return _ntt(c, ql)
    if kind == "alt":
        c = _const_rows([q - 1 for q in ql], n)
        c[:, 0::2] = 0
        return _ntt(c, ql)
    raise ValueError(kind)


def ks_keys(kind, allm, dnum, log_n):
    """(evk_b, evk_a), each [dnum][L + K][N] NTT form over allm = Q u P.
    tm1: every word t - 1; zero; select_<j> (j a digit index, or "last" for dnum - 1): evk_b[j] all
    ones, every other word of both keys 0, so that ks1 = 0 and
    ks0 = ModDown(NTT(ModUp(digit j)))."""
    allm = [int(m) for m in allm]
    n = 1 << log_n
    shape = (dnum, len(allm), n)
    if kind == "zero":
        return np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=np.uint64)
    if kind == "tm1":
        k = np.broadcast_to(_const_rows([t - 1 for t in allm], n), shape)
        return np.ascontiguousarray(k), np.ascontiguousarray(k)
    if kind.startswith("select_"):
        j = kind[len("select_"):]
        j = dnum - 1 if j == "last" else int(j)
        assert 0 <= j < dnum
        b = np.zeros(shape, dtype=np.uint64)
        b[j] = 1
        return b, np.zeros(shape, dtype=np.uint64)
    raise ValueError(kind)
