"""CKKS bootstrapping for full packing (N/2 slots) and sparse packing (n_s = 2^log_slots slots),
composed on the host from the library's public calls (include/fhecore.h; no C entry of its own,
like fhecore.polyeval):

    mod_raise [-> SubSum] -> CoeffToSlot -> conjugate + conj_split -> eval_mod (batch of 2)
              -> conj_merge -> SlotToCoeff

    dft_factors(log_n, groups, inverse)      the CoeffToSlot / SlotToCoeff matrices as diagonals
    place_strided_diagonals(...)             their baby-step / giant-step layout (host, numpy)
    encode_strided_diagonals(ctx, ...)       the same, encoded on the device (one fhe_encode call)
    Bootstrapper(backend, params).bootstrap(ct)

The factors.  n = N/2 slots, M = 2N, rot[j] = 5^j mod M, W[k] = exp(i pi k / N) (the table of
fhe_encode_roots).  fhe_encode runs the stages len = n, n/2 .. 2 (lh = len/2, lq = 4 len)
    (a, b) -> (a + b, (a - b) w),   w = W[(lq - rot[j] % lq) (M/lq)]
then a bit-reversal; fhe_decode a bit-reversal, then the stages len = 2, 4 .. n
    (a, b) -> (a + b w, a - b w),   w = W[(rot[j] % lq) (M/lq)].
CoeffToSlot is encode's stage network and SlotToCoeff decode's, both WITHOUT the bit-reversal: what
lies between them (conj_split, eval_mod, conj_merge) is slot-wise, so the two permutations cancel.
Each stage is a matrix with the diagonals 0, +lh and -lh (diagonal k: d_k[j] = A[j][(j + k) mod n];
at len = n the two shifts are the same diagonal n/2 and their entries add).  Consecutive stages
are merged into `groups` factors: for B applied after A, (B A)_{ka + kb} = b_kb * roll(a_ka, -kb).

Scales.  A ciphertext's slots are its raw integers divided by its declared scale.  ModRaise leaves
the raw coefficients t = m + q_0 I.  The CoeffToSlot factors carry delta / (2 n K q_0) in total
(its groups-th root each), so with the declared scale set to delta the slots after the split are
t_k / (K q_0): eval_mod's contract.  eval_mod returns m_k / q_0 at its own scale s_e (about
2 pi delta: its factor 1 / (2 pi) is a change of the declared scale).  The SlotToCoeff factors carry
q_0 / (2 pi delta) in total -- q_0 / delta, times the 1 / (2 pi) that brings s_e back to delta --
and the result is declared at  s_in s_e c / q_0  (c the product actually encoded, an exact
Fraction), which is the input's scale up to the evaluator's drift (~2^-30).  Every factor's
diagonals are encoded at the scale of the prime its rescale divides by, so a linear transform and
its rescale leave the declared scale where it was, exactly.

Sparse packing (BootstrapParams.log_slots < log_n - 1).  The message is a polynomial in Y = X^gap,
gap = N / (2 n_s), and the ciphertext's slot vector is n_s-periodic.  ModRaise leaves
t = m(Y) + q_0 I(X) with I spread over all N coefficients; SubSum,
    acc = t;  for i < log2(gap):  acc <- acc + sigma_{5^(n_s 2^i)}(acc)    (a rotation by n_s 2^i),
is the trace onto the subring: gap t[k gap] at the multiples of gap and 0 elsewhere, that is
gap (m(Y) + q_0 I'(Y)) with I'_k = I_{k gap}, so |I'| <= (h + 2) / 2, K and h <= 2K - 4 stand.
The two transforms are the stage network of the ring of degree 2 n_s (dft_factors(...,
log_slots): log_slots stages, tables sliced from the ring's, W_s[k] = W[k gap] and
5^j mod 4 n_s = rot[j] mod 4 n_s) as length-n_s diagonals; encoded sparsely they are those
diagonals tiled gap times, and their rotation steps are taken on the full ring (on a periodic
vector the steps k and k - n_s act alike).  The inverse network of a periodic slot vector gives
n_s times the Y-coefficients, SubSum gave gap: n_s gap = n, so the CoeffToSlot constant
delta / (2 n K q_0) and every scale rule above are those of full packing.  The result is a sparse
ciphertext: it decodes with log_slots.

The secret must be sparse: |I| <= (h + 2) / 2 must stay within eval_mod's K - 1, so h <= 2K - 4
(Context.keygen_secret(hamming_weight=h)).

Backends.  Like fhecore.polyeval the composition hands its backend integers and float64 slot
vectors only, so GpuBackend (below) and a CPU restatement compute the same bits.  A backend has
polyeval's calls (moduli, mul_relin, lincomb, drop_level) plus
    log_n                                    the ring degree's logarithm
    mod_raise(a, level)                      a at any level -> `level` limbs
    load_factor(z, baby, giant, delta)       z complex [n2, n1, n] (sparse packing: [n2, n1, n_s],
                                             encoded as the tiled vector) -> a handle for
                                             linear_transform
                                             (the plaintexts over Q u P and the rotation keys of
                                             the slot steps baby[b], giant[g]; step 0 takes none)
    linear_transform(a, factor), rescale(a)
    rotate(a, step)                          the slot rotation by `step` (SubSum; sparse packing only)
    conjugate(a), conj_split(a, c), conj_merge(a, b)
    stack(a, b), unstack(x)                  a batch of 2 and back
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from . import polyeval
from .polyeval import Ct

_BSGS_MAX = 16  # fhe_linear_transform: at most 16 baby steps and 16 giant steps


# ----------------------------------------------------------------------------- the factors

def _tables(log_n, log_slots=None):
    """(W [4 n_s], rot [n_s]) of the ring of degree 2 n_s, sliced from the table of the ring of
    degree 2^log_n (fhe_encode_roots refuses rings below 2^10): W_s[k] = W[k gap]."""
    from .context import encode_roots

    n = 1 << (log_n - 1)
    r = encode_roots(log_n)
    w = r[:, 0] + 1j * r[:, 1]
    rot = np.empty(n, dtype=np.int64)
    e = 1
    for j in range(n):
        rot[j] = e
        e = e * 5 % (4 * n)
    if log_slots is None or log_slots == log_n - 1:
        return w, rot
    ns = 1 << log_slots
    return w[::n // ns], rot[:ns] % (4 * ns)


def _slot_bits(log_n, log_slots):
    if log_slots is None:
        return log_n - 1
    if not 0 <= log_slots <= log_n - 1:
        raise ValueError(f"log_slots must be in [0, {log_n - 1}]")
    return int(log_slots)


def _stage(n, ln, w, rot, inverse):
    """The diagonals {k: complex [n]} of one stage of block length ln."""
    lh, lq, m = ln // 2, 4 * ln, 4 * n
    pos = np.arange(n) % ln
    first = pos < lh
    j = pos % lh
    if inverse:  # encode: (a, b) -> (a + b, (a - b) w)
        tw = w[(lq - rot[j] % lq) * (m // lq)]
        plus, minus = np.where(first, 1.0, 0.0), np.where(first, 0.0, tw)
    else:  # decode: (a, b) -> (a + b w, a - b w)
        tw = w[(rot[j] % lq) * (m // lq)]
        plus, minus = np.where(first, tw, 0.0), np.where(first, 0.0, 1.0)
    out = {0: np.where(first, 1.0, -tw).astype(np.complex128)}
    for k, v in ((lh % n, plus), ((n - lh) % n, minus)):
        out[k] = out.get(k, 0) + v.astype(np.complex128)  # len = n: +lh and -lh coincide
    return out


def _compose(a, b):
    """The diagonals of B A (A applied first)."""
    n = len(next(iter(a.values())))
    out = {}
    for kb, vb in b.items():
        for ka, va in a.items():
            k = (ka + kb) % n
            out[k] = out.get(k, 0) + vb * np.roll(va, -kb)
    return out


def stage_lengths(log_n, inverse, log_slots=None):
    """Block lengths of the stage network in the order of application (log_slots: of the ring of
    degree 2^(log_slots + 1), 2 .. n_s)."""
    lens = [1 << s for s in range(1, _slot_bits(log_n, log_slots) + 1)]  # 2 .. n
    return lens[::-1] if inverse else lens


def group_sizes(stages, groups):
    """Stages per factor: as even as possible, the larger groups first."""
    if not 1 <= groups <= stages:
        raise ValueError(f"dft_factors: groups must be in [1, {stages}]")
    q, r = divmod(stages, groups)
    return [q + 1] * r + [q] * (groups - r)


def dft_factors(log_n, groups, inverse, log_slots=None):
    """The special FFT's stage network as `groups` slot matrices, first applied first: a list of
    {diagonal index: complex128 [N/2]}.  inverse=True is CoeffToSlot (fhe_encode's stages,
    len = n .. 2), inverse=False SlotToCoeff (fhe_decode's, len = 2 .. n); neither includes the
    bit-reversal.  SlotToCoeff o CoeffToSlot = n id.  log_slots: the network of the ring of degree
    2^(log_slots + 1) as length-n_s diagonals, its tables sliced from the ring's; tiled
    N / 2^(log_slots + 1) times they act on the n_s-periodic slot vectors of the full ring."""
    n = 1 << _slot_bits(log_n, log_slots)
    w, rot = _tables(log_n, log_slots)
    lens = stage_lengths(log_n, inverse, log_slots)
    out, at = [], 0
    for size in group_sizes(len(lens), groups):
        f = _stage(n, lens[at], w, rot, inverse)
        for ln in lens[at + 1:at + size]:
            f = _compose(f, _stage(n, ln, w, rot, inverse))
        out.append(f)
        at += size
    return out


def factor_layouts(log_n, groups, inverse, log_slots=None):
    """(n1, n2, stride, offset) per factor of dft_factors: s merged stages whose smallest half
    length is `stride` have the diagonals stride * a, |a| <= 2^s - 1 (offset = -(2^s - 1),
    2^(s+1) - 1 of them), except the factor holding the stage len = n, where the shifts wrap and
    a = 0 .. 2^s - 1 covers them (offset 0).  log_slots: n = n_s; the steps are taken on the full
    ring, where on an n_s-periodic vector k and k - n_s act alike."""
    n = 1 << _slot_bits(log_n, log_slots)
    lens = stage_lengths(log_n, inverse, log_slots)
    out, at = [], 0
    for s in group_sizes(len(lens), groups):
        grp = lens[at:at + s]
        at += s
        stride = min(grp) // 2
        if n in grp:
            total, offset = n // stride, 0
        else:
            total, offset = (2 << s) - 1, -((1 << s) - 1)
        n1 = 1 << -(-(total - 1).bit_length() // 2)
        n2 = -(-total // n1)
        out.append((n1, n2, stride, offset))
    return out


def place_strided_diagonals(diags, n, n1, n2, stride=1, offset=0):
    """The baby-step / giant-step layout of a slot matrix whose diagonals sit at multiples of
    `stride`: diagonal stride (g n1 + b + offset) mod n goes to z[g][b], rolled towards higher
    indices by stride g n1, so that with rot_s(v)[j] = v[(j + s) mod n]
        A v = sum_g rot_{stride g n1}( sum_b z[g][b] * rot_{stride (b + offset)}(v) ).
    Returns (z complex128 [n2, n1, n], baby steps, giant steps) -- slot steps, not Galois elements.
    ValueError if a diagonal has no place or two places address one diagonal."""
    z = np.zeros((n2, n1, n), dtype=np.complex128)
    left = {int(k) % n: np.asarray(v, dtype=np.complex128).reshape(n) for k, v in diags.items()}
    if len(left) != len(diags):
        raise ValueError("place_strided_diagonals: two diagonal indices agree mod n")
    seen = set()
    for g in range(n2):
        for b in range(n1):
            k = stride * (g * n1 + b + offset) % n
            if k in seen:
                raise ValueError(f"place_strided_diagonals: diagonal {k} has two places")
            seen.add(k)
            if k in left:
                z[g, b] = np.roll(left.pop(k), stride * g * n1)
    if left:
        raise ValueError(f"place_strided_diagonals: diagonals {sorted(left)} have no place in "
                         f"stride {stride} x ({n2} x {n1}) from offset {offset}")
    baby = [stride * (b + offset) for b in range(n1)]
    giant = [stride * g * n1 for g in range(n2)]
    return z, baby, giant


def encode_strided_diagonals(ctx, diags, n1, n2, delta, stride=1, offset=0):
    """Context.encode_diagonals for diagonals at multiples of `stride`, starting at `offset`
    (place_strided_diagonals): returns (baby_elts, giant_elts, pts) for Context.linear_transform,
    baby_elts[b] = galois_elt(stride (b + offset)), giant_elts[g] = galois_elt(stride g n1),
    pts[g][b] [L + K, N] at scale delta.  All n1 n2 encodings are one fhe_encode call."""
    z, baby, giant = place_strided_diagonals(diags, ctx.n // 2, n1, n2, stride, offset)
    enc = ctx.encode(z, delta, level=ctx.L, special=True)
    return ([ctx.galois_elt(s) for s in baby], [ctx.galois_elt(s) for s in giant],
            [[enc[g, b] for b in range(n1)] for g in range(n2)])


# ----------------------------------------------------------------------------- the GPU backend

class GpuBackend(polyeval.GpuBackend):
    """The bootstrap backend over a fhecore Context.  With `sk` it makes the relinearisation
    key, the conjugation key and (in load_factor) the rotation keys of every baby / giant step
    itself; `relin_key` and `rot_keys` ({Galois element: (rot_b, rot_a)}) supply keys made
    elsewhere.  seed: the keys made here take the nonces seed, seed + 1, ... in the order they are
    made (reproducible tests; None draws each from the OS CSPRNG, fhecore.h SECURITY note)."""

    def __init__(self, ctx, sk=None, relin_key=None, rot_keys=None, seed=None):
        self.sk, self._seed = sk, seed
        if relin_key is None:
            if sk is None:
                raise ValueError("GpuBackend: give the secret key or the keys")
            relin_key = ctx.keygen_relin(sk, self._nonce())
        super().__init__(ctx, relin_key)
        self.log_n = ctx.log_n
        self.rot_keys = dict(rot_keys or {})

    def _nonce(self):
        if self._seed is None:
            return None
        self._seed += 1
        return self._seed - 1

    def _key(self, elt):
        if elt == 1:
            return None
        if elt not in self.rot_keys:
            if self.sk is None:
                raise ValueError(f"GpuBackend: no rotation key for Galois element {elt}")
            self.rot_keys[elt] = self.ctx.keygen_rotation(self.sk, elt, self._nonce())
        return self.rot_keys[elt]

    def mod_raise(self, a, level):
        return self.ctx.mod_raise(a, level)

    def load_factor(self, z, baby, giant, delta):
        c = self.ctx
        ns = z.shape[-1]
        sparse = None if ns == c.n // 2 else ns.bit_length() - 1
        enc = c.encode(z, delta, level=c.L, special=True, log_slots=sparse)
        be, ge = [c.galois_elt(s) for s in baby], [c.galois_elt(s) for s in giant]
        pts = [[enc[g, b] for b in range(len(be))] for g in range(len(ge))]
        return (be, [self._key(e) for e in be], ge, [self._key(e) for e in ge], pts)

    def linear_transform(self, a, factor):
        return self.ctx.linear_transform(a, *factor)

    def rescale(self, a):
        return self.ctx.rescale(a)

    def conjugate(self, a):
        elt = 2 * self.ctx.n - 1
        return self.ctx.rotate(a, elt, *self._key(elt))

    def rotate(self, a, step):
        elt = self.ctx.galois_elt(step)
        return self.ctx.rotate(a, elt, *self._key(elt))

    def conj_split(self, a, c):
        return self.ctx.conj_split(a, c)

    def conj_merge(self, a, b):
        return self.ctx.conj_merge(a, b)

    def stack(self, a, b):
        import torch

        return torch.stack([a, b])

    def unstack(self, x):
        return x[0], x[1]


# ----------------------------------------------------------------------------- the composition

@dataclass
class BootstrapParams:
    K: int = 16                # eval_mod's range: |I| <= K - 1
    degree: int = 31
    double_angles: int = 3
    cts_groups: int = 3
    stc_groups: int = 3
    delta: float = 2.0 ** 50   # the scale eval_mod works at: the chain's primes sit close to it
    hamming_weight: int = 28   # the declared weight of the secret
    log_slots: int | None = None  # sparse packing: 2^log_slots slots; None = log_n - 1, full


class Bootstrapper:
    """bootstrap(ct) refreshes a ciphertext at any level >= 1 to level
    L - cts_groups - eval_mod_levels - stc_groups (out_level).  The constructor builds the six
    factors, has the backend encode their diagonals and make their keys once, and refuses
    (ValueError) a declared Hamming weight above 2K - 4, a chain too short for the result to
    keep a level, and a log_slots outside [max(cts_groups, stc_groups), log_n - 1]."""

    def __init__(self, backend, params=None, **kw):
        p = params if params is not None else BootstrapParams(**kw)
        if params is not None and kw:
            raise ValueError("Bootstrapper: give params or keywords, not both")
        self.be, self.p, self.log_n = backend, p, int(backend.log_n)
        if p.K < 2 or p.hamming_weight < 1:
            raise ValueError("Bootstrapper: K >= 2 and a positive Hamming weight")
        if p.hamming_weight > 2 * p.K - 4:
            raise ValueError(f"Bootstrapper: a secret of Hamming weight {p.hamming_weight} lets "
                             f"|I| reach (h + 2) / 2 > K - 1 = {p.K - 1}: h <= 2K - 4 = "
                             f"{2 * p.K - 4}")
        q = [int(m) for m in backend.moduli]
        self.L = len(q)
        self.em_levels = polyeval.eval_mod_levels(p.degree, p.double_angles)
        self.out_level = self.L - p.cts_groups - self.em_levels - p.stc_groups
        if self.out_level < 1:
            raise ValueError(f"Bootstrapper: the chain of {self.L} primes is too short: "
                             f"{p.cts_groups} + {self.em_levels} + {p.stc_groups} levels are "
                             "consumed and the result needs one")
        lo = max(p.cts_groups, p.stc_groups)
        if p.log_slots is not None and not lo <= p.log_slots <= self.log_n - 1:
            raise ValueError(f"Bootstrapper: log_slots must be in [{lo}, {self.log_n - 1}] (a "
                             "factor needs a stage)")
        full = p.log_slots is None or p.log_slots == self.log_n - 1
        self.log_slots = None if full else int(p.log_slots)
        # SubSum: the rotations by n_s 2^i that sum the gap copies of the subring's coefficients
        self.subsum_steps = [] if full else [
            (1 << self.log_slots) << i for i in range(self.log_n - 1 - self.log_slots)]
        n = 1 << (self.log_n - 1)
        q0 = q[0]
        # CoeffToSlot: total delta / (2 n K q_0); SlotToCoeff: q_0 / (2 pi delta).  Sparse: SubSum's
        # gap times the small network's n_s is the same n
        c_cts = (p.delta / (2.0 * n * p.K * q0)) ** (1.0 / p.cts_groups)
        c_stc = (q0 / (2.0 * math.pi * p.delta)) ** (1.0 / p.stc_groups)
        lv = self.L
        self.cts, mult = self._load(True, p.cts_groups, c_cts, lv, q)
        # the declared scale after CoeffToSlot at which the slots are (t_k + i t_{k+n}) / (2 K q_0)
        self.scale_cts = mult * (2 * n * p.K * q0)
        lv -= p.cts_groups + self.em_levels
        self.stc, mult = self._load(False, p.stc_groups, c_stc, lv, q)
        self.mult_stc = mult / q0  # the result's scale is s_in s_e mult_stc

    def _load(self, inverse, groups, const, level, q):
        """The factors' handles and the exact product of what their encodings multiply the raw
        integers by, relative to the rescales that follow: prod const * float(q_l) / q_l."""
        ls = self.log_slots
        n = 1 << (self.log_n - 1 if ls is None else ls)
        out, mult = [], Fraction(1)
        layouts = factor_layouts(self.log_n, groups, inverse, ls)
        factors = dft_factors(self.log_n, groups, inverse, ls)
        for f, (n1, n2, stride, offset) in zip(factors, layouts):
            if n1 > _BSGS_MAX or n2 > _BSGS_MAX:
                raise ValueError(f"Bootstrapper: a factor of {n1} x {n2} baby / giant steps exceeds "
                                 f"linear_transform's {_BSGS_MAX}: use more groups")
            z, baby, giant = place_strided_diagonals({k: v * const for k, v in f.items()}, n, n1, n2,
                                                     stride, offset)
            delta = float(q[level - 1])  # the prime this factor's rescale divides by
            out.append(self.be.load_factor(z, baby, giant, delta))
            mult *= Fraction(const) * Fraction(delta) / q[level - 1]
            level -= 1
        return out, mult

    def _transform(self, a, factors):
        for f in factors:
            a = self.be.rescale(self.be.linear_transform(a, f))
        return a

    def bootstrap(self, ct: Ct, mark=None) -> Ct:
        """mark: called with the phase's name after each of mod_raise, subsum (sparse packing
        only), coeff_to_slot, split (conjugation included), eval_mod, merge, slot_to_coeff
        (tools/bootstrap_times.py)."""
        be, p = self.be, self.p
        mark = mark or (lambda name: None)
        if not 1 <= ct.level <= self.L:
            raise ValueError(f"bootstrap: the input is at level {ct.level}, expected 1 .. {self.L}")
        a = be.mod_raise(ct.data, self.L)            # reads limb 0 only: no drop needed
        mark("mod_raise")
        if self.subsum_steps:
            for step in self.subsum_steps:
                a = be.lincomb([a, be.rotate(a, step)], [1, 1], False, False, self.L)
            mark("subsum")
        a = self._transform(a, self.cts)
        mark("coeff_to_slot")
        re, im = be.conj_split(a, be.conjugate(a))   # slots t_k / (K q_0), t_{k+n} / (K q_0)
        x = be.stack(re, im)
        mark("split")
        lv = self.L - p.cts_groups
        e = polyeval.eval_mod(be, Ct(x, lv, self.scale_cts), p.K, p.degree, p.double_angles)
        mark("eval_mod")
        a = be.conj_merge(*be.unstack(e.data))
        mark("merge")
        a = self._transform(a, self.stc)
        mark("slot_to_coeff")
        return Ct(a, self.out_level, Fraction(ct.scale) * e.scale * self.mult_stc)
