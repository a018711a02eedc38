"""CPU model of the fused HomMult row kernel's pair form (csrc/ntt.hip hm_row_pairs, the
k_hommult_row<16, 16, true> instantiation): the last forward stage and the first inverse stage
are not run; the tensor multiplies degree-1 polynomials mod X^2 - z^2 on the adjacent pairs
instead, and the column inverse folds 2 N^-1 in place of N^-1.  Restated in Python integers:

  * the identity that gives z^2 from the previous stage's twiddle, and its sign rule;
  * the operand ranges (a0, a1, b0, b1 < 2q, b1' <= 2q) and, on worst-case operands, the bounds of
    every accumulated sum (below q 2^64, mont_redc_x's precondition) and of every partial-product
    column (the asserts inside the mul2_wide61 / dot_wide61 models);
  * the 6-stage forward and 3-stage first inverse range schedules;
  * exhaustively at a toy size, that truncated forward + pair tensor + truncated inverse + 2 N^-1
    equals the full pipeline.

The guarantee all bounds rest on is lz16's q < 2^60 (context.cpp): 4 terms below (2q)(2q) sum
below 16 q^2 <= q 2^64."""
import random

import numpy as np
import pytest

import pyoracle
from test_modarith_model import (M32, M64, _lz16, dot_wide61, mont_redc_x, mul2_wide61, shoup_fast,
                                 shoup_q3, top_bits)


def _lz16_extremes(log_n=16, bits=60):
    """The largest and the smallest lz16 modulus the generator can produce at `bits`: primes
    q = 1 mod 2N in [2^bits - 2^(bits-4), 2^bits)."""
    hi = pyoracle.gen_moduli(log_n, 1, bits=bits)[0]
    step = 2 << log_n
    lo_bound = (1 << bits) - (1 << (bits - 4))
    q = (lo_bound + step - 1) // step * step + 1
    while not pyoracle.is_prime(q):
        q += step
    assert _lz16(hi) and _lz16(q) and q >= lo_bound and q < hi
    return [hi, q]


QS = _lz16_extremes()
# the arithmetic bound itself (not a prime; odd, so REDC is defined): the top of what lz16 admits
Q_TOP = (1 << 60) - 1


# ---- z^2 from the previous stage ------------------------------------------------------------

@pytest.mark.parametrize("q,log_n", [(QS[0], 16), (QS[1], 16), (pyoracle.gen_moduli(10, 1)[0], 10),
                                     (97, 4)])
def test_zeta_square_is_previous_stage_twiddle(q, log_n):
    """psi^brv order: tw[2k]^2 = tw[k], tw[2k + 1]^2 = -tw[k] for every k >= 1.  The kernel's use:
    the pair at position p of 7-stage row r has last-stage twiddle tw[(r << 6) + (p >> 1)], so
    z^2 = +/- tw[(r << 5) + (p >> 2)], minus when bit 1 of p is set."""
    tw, twi, _ = pyoracle.twiddles(q, log_n)
    n = 1 << log_n
    for k in range(1, n // 2):
        assert tw[2 * k] * tw[2 * k] % q == tw[k]
        assert tw[2 * k + 1] * tw[2 * k + 1] % q == q - tw[k]
        assert tw[2 * k] * twi[2 * k] % q == 1  # the inverse table holds z^-1 at the same index
    if log_n == 16:
        for r in (512, 513, 700, 1023):          # rows 2^9 + row of the 512 x 128 view
            for p in range(0, 128, 2):
                z = tw[(r << 6) + (p >> 1)]
                prev = tw[(r << 5) + (p >> 2)]
                assert z * z % q == (q - prev if (p >> 1) & 1 else prev)


# ---- the pair tensor's sums on worst-case operands --------------------------------------------

def pair_d0(a, b, b1p):
    """(a0 b0 + a1 b1', a0 b1 + a1 b0) as 128-bit sums (mul2_wide61)."""
    return mul2_wide61(a[0], b[0], a[1], b1p), mul2_wide61(a[0], b[1], a[1], b[0])


def pair_d1(a0, a1, b0, b1, b0p, b1p):
    """The 4-term sums over (A0, B1) and (A1, B0) (dot_wide61<4>, the kernel's operand order)."""
    xa = [a0[0], a0[1], a1[0], a1[1]]
    return (dot_wide61(xa, [b1[0], b1p, b0[0], b0p]),
            dot_wide61(xa, [b1[1], b1[0], b0[1], b0[0]]))


def b1_prime(b1, w, q, odd):
    """The B groups' b1' = z^2 b1: shoup_fast's [0, 2q) for +w, 2q minus it for -w."""
    r = shoup_fast(b1, w, (w << 64) // q, q)
    assert 0 <= r < 2 * q and r % q == b1 * w % q
    out = 2 * q - r if odd else r
    assert 0 <= out <= 2 * q and out < 1 << 61
    assert out % q == (b1 * (q - w if odd else w)) % q
    return out


@pytest.mark.parametrize("q", QS + [Q_TOP])
def test_pair_sums_worst_case(q):
    """Every operand at the top of its range: a0, a1, b0, b1 = 2q - 1, b1' = 2q.  The sums stay
    below q 2^64 and every partial-product column inside its word (asserted in the models); the
    models equal exact integer arithmetic; REDC returns t R^-1 in (0, 2q)."""
    assert q < 1 << 60  # the lz16 guarantee the bound rests on
    top, topp = 2 * q - 1, 2 * q
    assert topp < 1 << 61 and (topp >> 32) < 1 << 29
    R_inv = pow(1 << 64, -1, q)
    a = (top, top)
    e, o = pair_d0(a, (top, top), topp)
    assert e == top * top + top * topp and o == 2 * top * top
    e4, o4 = pair_d1(a, a, (top, top), (top, top), topp, topp)
    assert e4 == 2 * (top * top + top * topp) and o4 == 4 * top * top
    for t in (e, o, e4, o4):
        assert t < 16 * q * q <= q << 64
        r = mont_redc_x(t, q)
        assert 0 < r < 2 * q and r % q == t * R_inv % q
    # the middle column of the 4-term sum at the operands' word-level maxima (any q < 2^60):
    # 8 products of a 32-bit by a 29-bit half, and the 32-bit addend of the high chain
    m = 8 * M32 * ((1 << 29) - 1)
    assert m < 1 << 64 and (m >> 32) + 1 + 3 <= M32


@pytest.mark.parametrize("q", QS)
def test_pair_sums_random_and_edges(q):
    rng = random.Random(q + 31)
    R_inv = pow(1 << 64, -1, q)
    edge = [0, 1, q - 1, q, 2 * q - 1]
    for trial in range(4000):
        pick = (lambda: rng.choice(edge)) if trial < 1500 else (lambda: rng.randrange(2 * q))
        a0, a1 = (pick(), pick()), (pick(), pick())
        b0, b1 = (pick(), pick()), (pick(), pick())
        w = rng.choice([0, 1, q - 1, rng.randrange(q)])
        odd = trial & 1
        z2 = (q - w) % q if odd else w
        b0p, b1p = b1_prime(b0[1], w, q, odd), b1_prime(b1[1], w, q, odd)
        outs = list(pair_d0(a0, b0, b0p)) + list(pair_d0(a1, b1, b1p))
        outs += list(pair_d1(a0, a1, b0, b1, b0p, b1p))
        want = [a0[0] * b0[0] + z2 * a0[1] * b0[1], a0[0] * b0[1] + a0[1] * b0[0],
                a1[0] * b1[0] + z2 * a1[1] * b1[1], a1[0] * b1[1] + a1[1] * b1[0],
                a0[0] * b1[0] + a1[0] * b0[0] + z2 * (a0[1] * b1[1] + a1[1] * b0[1]),
                a0[0] * b1[1] + a0[1] * b1[0] + a1[0] * b0[1] + a1[1] * b0[0]]
        for t, wv in zip(outs, want):
            assert t < q << 64
            r = mont_redc_x(t, q)
            assert 0 < r < 2 * q and r % q == wv * R_inv % q


# ---- range schedules ---------------------------------------------------------------------------

def fwd_stage_out(r, H=16):
    """ntt.hip fwd_stage_out: a CT stage's output range from X-operands below r q."""
    return (2 if r + 3 > H else r) + 3


def fwd_range(r0, stages, H=16):
    for _ in range(stages):
        r0 = fwd_stage_out(r0, H)
    return r0


@pytest.mark.parametrize("q", QS)
def test_forward_six_stage_schedule(q):
    """Column pass: 9 stages from canonical inputs (below 14q).  Rows: 3 + 3 stages, every value
    below 16q, the outputs below 8q, which top_bits takes below 2q (the tensor's operand range)."""
    rin0 = fwd_range(1, 9)
    rin1 = fwd_range(rin0, 3)
    rout = fwd_range(rin1, 3)
    assert (rin0, rin1, rout) == (14, 11, 8)
    r = rin0
    for _ in range(6):
        r = fwd_stage_out(r)
        assert r <= 16 and r * q <= 1 << 64
    assert 4 < rout <= 16  # round_compute's condition for the one-step final reduction
    rng = random.Random(q + 5)
    for x in [0, q, 2 * q - 1, rout * q - 1] + [rng.randrange(rout * q) for _ in range(2000)]:
        y = top_bits(x, q)
        assert y < 2 * q and y % q == x % q


def gs_red(r):
    return 2 if r > 8 else r


def gs_in(j, k, r0=3):
    """ntt.hip gs_in with the round's input range r0."""
    r = r0
    for b in range(k):
        r = 3 if (j >> b) & 1 else 2 * gs_red(r)
    return r


@pytest.mark.parametrize("q", QS)
def test_inverse_three_stage_first_round(q):
    """The first inverse round after the pair tensor: 3 GS stages on element bits 0-2 (position
    bits 1-3; element bit 3 is the pair's own bit and is not butterflied), inputs the REDC outputs
    below 2q.  Ranges run 2 -> 4 -> 8 -> 16 with no reduction inside the round; the end takes every
    element above 3q below 2q.  Outputs congruent to the exact GS butterflies'."""
    rng = random.Random(q + 17)
    KB = 3
    for trial in range(300):
        hi = 2 * q - 1
        x = [hi] * 16 if trial == 0 else [rng.choice([1, hi, rng.randrange(1, 2 * q)])
                                          for _ in range(16)]
        ref = [v % q for v in x]
        tw = {(b, j): rng.randrange(q) for b in range(KB) for j in range(16)}
        for b in range(KB):
            for j in range(16):
                if (j >> b) & 1:
                    continue
                jj = j | (1 << b)
                r = gs_in(j, b, 2)
                assert gs_in(jj, b, 2) == r and r in (2, 3, 4, 6, 8)
                assert gs_red(r) == r  # no reduction inside the round
                assert x[j] < r * q and x[jj] < r * q
                u, v, w = x[j], x[jj], tw[(b, j)]
                s, d = u + v, u - v + r * q
                assert s < 16 * q <= 1 << 64 and 0 < d < 16 * q
                x[j], x[jj] = s, shoup_q3(d, w, (w << 64) // q, q)
                ref[j], ref[jj] = (ref[j] + ref[jj]) % q, (ref[j] - ref[jj]) * w % q
        for j in range(16):
            r = gs_in(j, KB, 2)
            assert r <= 16 and x[j] < r * q
            if r > 3:
                x[j] = top_bits(x[j], q)
                assert x[j] < 2 * q
            assert x[j] < 3 * q and x[j] % q == ref[j]  # the next round's input range


# ---- the whole pipeline at a toy size ------------------------------------------------------------

def _fwd_truncated(a, q, tw):
    """pyoracle.ntt_fwd without its last stage (m = n / 2, the adjacent pairs)."""
    a = list(a)
    n = len(a)
    t, m = n, 1
    while m < n // 2:
        t //= 2
        for i in range(m):
            s = tw[m + i]
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = a[j], a[j + t] * s % q
                a[j], a[j + t] = (u + v) % q, (u - v) % q
        m *= 2
    return a


def _inv_truncated(a, q, twi, fold):
    """pyoracle.ntt_inv without its first stage (the adjacent pairs), times `fold`."""
    a = list(a)
    n = len(a)
    t, m = 2, n // 2
    while m > 1:
        h = m // 2
        j1 = 0
        for i in range(h):
            s = twi[h + i]
            for j in range(j1, j1 + t):
                u, v = a[j], a[j + t]
                a[j], a[j + t] = (u + v) % q, (u - v) * s % q
            j1 += 2 * t
        t *= 2
        m = h
    return [x * fold % q for x in a]


def _pair_mul(A, B, q, tw, sign_seen):
    """Pair tensor of two truncated transforms: pair i uses z^2 = +/- tw[(n/2 + i) >> 1]."""
    n = len(A)
    out = [0] * n
    for i in range(n // 2):
        k = n // 2 + i
        z2 = tw[k >> 1] if k % 2 == 0 else q - tw[k >> 1]
        sign_seen.add((i, k % 2))
        a0, a1, b0, b1 = A[2 * i], A[2 * i + 1], B[2 * i], B[2 * i + 1]
        b1p = z2 * b1 % q
        out[2 * i] = (a0 * b0 + a1 * b1p) % q
        out[2 * i + 1] = (a0 * b1 + a1 * b0) % q
    return out


@pytest.mark.parametrize("q,log_n", [(97, 4), (193, 5)])
def test_truncated_pipeline_equals_full(q, log_n):
    """Every pair index, both signs: unit vectors at every (i, j) and random polynomials through
    truncated forward + pair tensor + truncated inverse + 2 N^-1 against the full transforms, and the
    three HomMult outputs against pyoracle.hommult."""
    n = 1 << log_n
    tw, twi, n_inv = pyoracle.twiddles(q, log_n)
    fold = 2 * n_inv % q
    rng = random.Random(q)
    seen = set()

    def full(a, b):
        fa, fb = pyoracle.ntt_fwd(a, q), pyoracle.ntt_fwd(b, q)
        return pyoracle.ntt_inv([x * y % q for x, y in zip(fa, fb)], q)

    def trunc(a, b):
        return _inv_truncated(_pair_mul(_fwd_truncated(a, q, tw), _fwd_truncated(b, q, tw), q, tw,
                                        seen), q, twi, fold)

    cases = []
    for i in range(n):
        for j in range(n):
            a, b = [0] * n, [0] * n
            a[i], b[j] = rng.randrange(1, q), rng.randrange(1, q)
            cases.append((a, b))
    cases += [([rng.randrange(q) for _ in range(n)], [rng.randrange(q) for _ in range(n)])
              for _ in range(50)]
    cases.append(([q - 1] * n, [q - 1] * n))
    for a, b in cases:
        got = trunc(a, b)
        assert got == full(a, b)
        assert got == [int(v) for v in pyoracle.negacyclic_mul(a, b, q)]
    assert seen == {(i, (n // 2 + i) % 2) for i in range(n // 2)} and {s for _, s in seen} == {0, 1}
    # the ciphertext tensor: d0 = A0 B0, d1 = A0 B1 + A1 B0 (4-term pair sums), d2 = A1 B1
    for _ in range(20):
        ct = [[rng.randrange(q) for _ in range(n)] for _ in range(4)]
        A0, A1, B0, B1 = (_fwd_truncated(p, q, tw) for p in ct)
        d0 = _pair_mul(A0, B0, q, tw, seen)
        d2 = _pair_mul(A1, B1, q, tw, seen)
        d1 = [(x + y) % q for x, y in zip(_pair_mul(A0, B1, q, tw, seen),
                                          _pair_mul(A1, B0, q, tw, seen))]
        got = [_inv_truncated(p, q, twi, fold) for p in (d0, d1, d2)]
        a = np.array([[ct[0]], [ct[1]]], dtype=np.uint64)
        b = np.array([[ct[2]], [ct[3]]], dtype=np.uint64)
        ref = pyoracle.hommult(a, b, [q])
        for k in range(3):
            assert got[k] == [int(v) for v in ref[k][0]]
