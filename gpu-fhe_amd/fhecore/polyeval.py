"""Chebyshev series on a ciphertext: the polynomial evaluation of CKKS bootstrapping's EvalMod,
composed on the host from mul_relin and lincomb (include/fhecore.h; no C entry of its own).

    chebyshev_eval(backend, ct, coeffs)  ->  sum_{j <= d} coeffs[j] T_j(x),  slots x in [-1, 1]
    eval_mod(backend, ct, K, degree, double_angles)  ->  sin(2 pi K x) / (2 pi)   (EvalMod itself:
        the series of a scaled cosine, then double-angle steps; at the end of this file)

Baby steps T_1 .. T_m (m a power of two, m^2 >= d + 1) and giants T_2m, T_4m, ... come from
T_2a = 2 T_a^2 - 1 and T_a+b = 2 T_a T_b - T_a-b, each one mul_relin(rescale) and one lincomb; T_k
sits ceil(log2 k) levels below the input.  The series is split recursively by Chebyshev division,
p = q T_g + r (g = 2^j m, T_k = 2 T_g T_k-g - T_2g-k for g < k < 2g), down to leaves
sum_{j < m} c_j T_j, each ONE lincomb(rescale=True) whose integer scalars are
round(c_j S q_l / scale(T_j)): after the rescale the leaf sits exactly at the scale S chosen for it,
whatever the drift of the individual T_j, and S is chosen top-down so that both sides of every
addition q T_g + r meet at exactly one scale.

Scales.  CKKS tracks value * scale; a product's scale is s_a s_b / q_l after its rescale.  The
chain this evaluator is meant for has every prime close to the scaling factor (e.g.
gen_moduli(log_n, L + K, bits=50) with delta = 2^50), so every scale stays within a factor
1 +- 2^-30 or so of delta.  Scales are exact Fractions here.  The one place two scales that were
not chosen meet is T_a+b = 2 T_a T_b - T_a-b: the ratio of the two must be within 2^-20 of an
integer (1 on the intended chain; the relative error that leaves, ~2^-30, is part of the measured
accuracy), else ValueError -- mismatched scales are never added silently.

Levels.  A degree-d series consumes at most ceil(log2(d + 1)) + 1 levels (levels_needed: d = 7: 4,
d = 15: 5, d = 63: 7) and ValueError is raised before any work if the input has fewer to give.  The result still needs
head room: at scale ~q_0 a result at level 1 wraps, so plan for a result level >= 2.

Backends.  The evaluator hands the backend INTEGER scalars, so every backend performs the same
exact modular computation: GpuBackend (this library) and a CPU restatement give the same bits.
A backend has
    moduli                                   the Q-primes q_0 .. q_{L-1}
    mul_relin(a, b, rescale)                 a, b at one level -> Relin(a b) [rescaled]
    lincomb(cts, ints, const, rescale, level)  sum ints[i] cts[i] (+ ints[len(cts)]) at `level`
    drop_level(a, level)
    mul_sum_relin(as_, bs, rescale, level)   Relin(sum as_[i] bs[i]) at `level` [rescaled]; operands
                                             at any level >= level (inner_product only)
on its own ciphertext arrays [..., 2, l, N].
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

_TOL = Fraction(1, 1 << 20)


@dataclass
class Ct:
    """A ciphertext [..., 2, level, N] (a device tensor, or whatever the backend computes on) with
    its level and its scale (Fraction, or a float that is converted exactly)."""
    data: object
    level: int
    scale: object


class GpuBackend:
    """The backend over a fhecore Context and its relinearisation key (evk_b, evk_a)."""

    def __init__(self, ctx, relin_key):
        self.ctx = ctx
        self.key = relin_key
        self.moduli = list(ctx.moduli)

    def mul_relin(self, a, b, rescale):
        return self.ctx.mul_relin(a, b, self.key[0], self.key[1], rescale=rescale)

    def lincomb(self, cts, scalars, const, rescale, level):
        tab = self.ctx.encode_scalars(scalars, exact=True)
        return self.ctx.lincomb(cts, tab, const=const, rescale=rescale, level=level)

    def drop_level(self, a, level):
        return self.ctx.drop_level(a, level)

    def mul_sum_relin(self, as_, bs, rescale, level):
        return self.ctx.mul_sum_relin(as_, bs, self.key[0], self.key[1], rescale=rescale,
                                      level=level)


def _ilog2_ceil(k: int) -> int:
    return (k - 1).bit_length()


def _match(s_prod: Fraction, s_old: Fraction):
    """Integer multipliers (k_prod, k_old) bringing the two scales together, and the common scale."""
    r = s_prod / s_old
    k = round(r)
    if k >= 1 and abs(r - k) <= _TOL:  # s_prod = k s_old
        return 1, k, s_prod
    k = round(1 / r)
    if k >= 1 and abs(1 / r - k) <= _TOL:  # s_old = k s_prod
        return k, 1, s_prod * k
    raise ValueError(f"chebyshev_eval: scales {float(s_prod):.6g} and {float(s_old):.6g} meet in an "
                     "addition and their ratio is not an integer: every prime of the chain must "
                     "be close to the scaling factor")


def _out_level(n: int, g: int, m: int, l0: int) -> int:
    """The level at which a sub-series of n <= g = 2^j m coefficients comes out for an input at
    level l0 (T_k sits at l0 - ceil(log2 k)); mirrors _Eval.run."""
    if g == m:
        return l0 - _ilog2_ceil(max(m - 1, 1)) - 1
    h = g // 2
    if n <= h:
        return _out_level(n, h, m, l0)
    lq = min(_out_level(n - h, h, m, l0), l0 - _ilog2_ceil(h))
    return min(lq - 1, _out_level(h, h, m, l0))


def _plan(degree: int):
    """(m, g): baby-step count and the power-of-two multiple of it above the degree."""
    m = 2
    while m * m < degree + 1:
        m *= 2
    g = m
    while g <= degree:
        g *= 2
    return m, g


def levels_needed(degree: int) -> int:
    """Levels a degree-`degree` series consumes: at most ceil(log2(degree + 1)) + 1 (exactly that
    when degree + 1 is a power of two >= 8)."""
    m, g = _plan(degree)
    return -_out_level(degree + 1, g, m, 0)


class _Eval:
    def __init__(self, be, ct, m):
        self.be = be
        self.q = [int(q) for q in be.moduli]
        self.m = m
        self.T = {1: Ct(ct.data, ct.level, Fraction(ct.scale))}

    def at(self, c: Ct, level: int):
        return c.data if c.level == level else self.be.drop_level(c.data, level)

    def product(self, a: Ct, b: Ct) -> Ct:
        """mul_relin at the lower of the two levels, rescaled."""
        lv = min(a.level, b.level)
        d = self.be.mul_relin(self.at(a, lv), self.at(b, lv), True)
        return Ct(d, lv - 1, a.scale * b.scale / self.q[lv - 1])

    def cheb(self, k: int) -> Ct:
        if k in self.T:
            return self.T[k]
        if k % 2 == 0:  # T_2a = 2 T_a^2 - 1
            a = self.cheb(k // 2)
            p = self.product(a, a)
            d = self.be.lincomb([p.data], [2, -round(p.scale)], True, False, p.level)
            t = Ct(d, p.level, p.scale)
        else:  # T_a+b = 2 T_a T_b - T_a-b, a the largest power of two below k
            a = 1 << (k.bit_length() - 1)
            b = k - a
            ta, tb, tc = self.cheb(a), self.cheb(b), self.cheb(a - b)
            p = self.product(ta, tb)
            kp, kc, s = _match(p.scale, tc.scale)
            d = self.be.lincomb([p.data, tc.data], [2 * kp, -kc], False, False, p.level)
            t = Ct(d, p.level, s)
        self.T[k] = t
        return t

    def run(self, c, g: int, scale: Fraction) -> Ct:
        """sum_k c[k] T_k for len(c) <= g = 2^j m, at exactly `scale`."""
        if g == self.m:
            lv = self.leaf_level
            ql = self.q[lv - 1]
            c = list(c) + [Fraction(0)] * (self.m - len(c))
            ks = [round(c[j] * scale * ql / self.T[j].scale) for j in range(1, self.m)]
            ks.append(round(c[0] * scale * ql))
            d = self.be.lincomb([self.T[j].data for j in range(1, self.m)], ks, True, True, lv)
            return Ct(d, lv - 1, scale)
        h = g // 2
        if len(c) <= h:
            return self.run(c, h, scale)
        # Chebyshev division by T_h: T_k = 2 T_h T_k-h - T_2h-k for h < k < 2h
        quo = [c[h]] + [2 * c[k] for k in range(h + 1, len(c))]
        rem = list(c[:h])
        for k in range(h + 1, len(c)):
            rem[2 * h - k] -= c[k]
        th = self.T[h]
        lv = min(_out_level(len(quo), h, self.m, self.T[1].level), th.level)
        q = self.run(quo, h, scale * self.q[lv - 1] / th.scale)
        p = self.product(q, th)
        r = self.run(rem, h, scale)
        if p.scale != r.scale:
            raise ValueError("chebyshev_eval: quotient and remainder scales differ")
        lo = min(p.level, r.level)
        return Ct(self.be.lincomb([p.data, r.data], [1, 1], False, False, lo), lo, scale)


def chebyshev_eval(backend, ct: Ct, coeffs, target_scale=None) -> Ct:
    """sum_j coeffs[j] T_j(x) on the slots of ct (values in [-1, 1]), degree len(coeffs) - 1 <= 63.
    Returns a Ct levels_needed(degree) levels below ct at exactly target_scale (default: ct's)."""
    c = [Fraction(v) for v in coeffs]
    d = len(c) - 1
    if d < 0 or d > 63:
        raise ValueError("chebyshev_eval: degree must be 0 .. 63")
    m, g = _plan(d)
    need = -_out_level(d + 1, g, m, 0)
    if ct.level - need < 1 or ct.level > len(backend.moduli):
        raise ValueError(f"chebyshev_eval: degree {d} consumes {need} levels and the input is at "
                         f"level {ct.level}: too few levels")
    ev = _Eval(backend, ct, m)
    for k in range(2, m):
        ev.cheb(k)
    h = m
    while h < g:
        ev.cheb(h)
        h *= 2
    ev.leaf_level = min(ev.T[j].level for j in range(1, m))
    scale = Fraction(ct.scale if target_scale is None else target_scale)
    return ev.run(c, g, scale)


def eval_mod_levels(degree: int, double_angles: int) -> int:
    """Levels eval_mod consumes: the Chebyshev series, then one per double-angle step."""
    return levels_needed(degree) + double_angles


def eval_mod(backend, ct: Ct, K: int, degree: int = 31, double_angles: int = 2) -> Ct:
    """sin(2 pi K v) / (2 pi) on the slots v of ct (real, in [-1, 1]; chebyshev_eval's contract):
    for K v = I + eps with I an integer -- a ciphertext after mod_raise and CoeffToSlot, scaled
    into [-1, 1] -- this is eps up to (2 pi)^2 |eps|^3 / 6: the q_0 I term is gone.

    With r = double_angles: the Chebyshev interpolant of cos((2 pi K v - pi / 2) / 2^r) of the
    given degree (chebyshev_eval at its default target scale), then r double-angle steps
    cos 2a = 2 cos^2 a - 1, each one mul_relin(rescale) and one lincomb -- the even branch of the
    evaluator's T_2a -- which end at cos(2 pi K v - pi / 2) = sin(2 pi K v).  The factor 1 / (2 pi)
    is a change of the declared scale (scale * 2 pi, the float 2 pi as an exact Fraction): no level
    and no multiplication.  Consumes eval_mod_levels(degree, double_angles) levels; ValueError
    before any work if the input has fewer to give, or K < 1."""
    import math

    import numpy as np

    r = int(double_angles)
    if K < 1 or r < 0:
        raise ValueError("eval_mod: K must be at least 1 and double_angles non-negative")
    if 0 <= degree <= 63:  # (another degree is chebyshev_eval's error)
        need = eval_mod_levels(degree, r)
        if ct.level - need < 1 or ct.level > len(backend.moduli):
            raise ValueError(f"eval_mod: degree {degree} with {r} double angles consumes {need} "
                             f"levels and the input is at level {ct.level}: too few levels")
    w, div = 2.0 * math.pi * K, float(1 << r)
    c = np.polynomial.chebyshev.chebinterpolate(lambda v: np.cos((w * v - math.pi / 2) / div),
                                                degree)
    out = chebyshev_eval(backend, ct, [Fraction(float(v)) for v in c])
    q = [int(m) for m in backend.moduli]
    for _ in range(r):  # cos 2a = 2 cos^2 a - 1
        d = backend.mul_relin(out.data, out.data, True)
        p = Ct(d, out.level - 1, out.scale * out.scale / q[out.level - 1])
        d = backend.lincomb([p.data], [2, -round(p.scale)], True, False, p.level)
        out = Ct(d, p.level, p.scale)
    return Ct(out.data, out.level, out.scale * Fraction(2.0 * math.pi))


def inner_product(backend, xs, ys) -> Ct:
    """sum_i xs[i] * ys[i] over two lists of Ct (up to 16 terms) with ONE relinearisation and ONE
    rescale (backend.mul_sum_relin; fhe_mul_sum_relin_level): less work and less noise than a
    mul_relin per term.  Every product xs[i].scale * ys[i].scale must be one scale (ValueError
    otherwise: mismatched scales are never added silently); the sum is taken at the lowest level l
    of the operands and returned at level l - 1 with scale s_x s_y / q_{l-1}."""
    if not xs or len(xs) != len(ys):
        raise ValueError("inner_product: two lists of one length, at least one term")
    scale = Fraction(xs[0].scale) * Fraction(ys[0].scale)
    for x, y in zip(xs, ys):
        if Fraction(x.scale) * Fraction(y.scale) != scale:
            raise ValueError("inner_product: the products do not share one scale")
    lv = min(c.level for c in (*xs, *ys))
    if lv < 2 or lv > len(backend.moduli):
        raise ValueError(f"inner_product: the lowest level is {lv}: the rescale needs 2 .. L")
    d = backend.mul_sum_relin([x.data for x in xs], [y.data for y in ys], True, lv)
    return Ct(d, lv - 1, scale / int(backend.moduli[lv - 1]))
