"""References for fhecore.bootstrap: the float64 plaintext model of the pipeline, and the parameters,
chain and rotation elements of the case the CPU and GPU tests share (tests/cases.py BOOTSTRAP):

  log_n = 10, L = 18, 5 special primes, dnum = 4; q_0 the largest 55-bit prime of the ring, the
  other 22 primes the 50-bit chain, delta = 2^50; a secret of Hamming weight 28
  (pyoracle.sparse_secret_coefficients);
  K = 16, degree 31, 3 double angles, 3 + 3 factors: 3 + 9 + 3 levels, the result at level 3;
  512 slots uniform in the square [-1, 1]^2, fixed seeds, keys from pyoracle.

The size of q_0 over delta = 2^50 is chosen with `model` below.  EvalMod returns m / q_0 with its
own cubic term (2 pi)^2 (m / q_0)^3 / 6, and SlotToCoeff multiplies every error in it by q_0 / delta:
a larger q_0 shrinks the cubic term (by 4 per bit, after the multiplication) and grows the
evaluator's noise (by 2 per bit).  model() at log_n = 10, seed 3, maximum slot error:

    q_0 bits   exact sine     interpolant     exact sine + 1e-8      interpolant + 1e-8
       54       1.07e-04       1.07e-04            1.08e-04               1.08e-04
       55       2.67e-05       2.68e-05            4.02e-05               4.03e-05
       56       6.68e-06       6.83e-06            5.48e-05               5.51e-05
       58       4.18e-07       3.75e-06            2.23e-04               2.25e-04
       60       2.61e-08       1.46e-05            8.94e-04               8.99e-04

(1e-8: normal noise of that deviation on every EvalMod output, the size of cases.EVALMOD_ERR.)
With the evaluator's noise the minimum is at 55 bits: that is the choice."""
import numpy as np

import pyoracle

LOG_N, L, NSPECIAL, DNUM = 10, 18, 5, 4
Q0_BITS, BITS = 55, 50
DELTA = 2.0 ** 50
HAMMING = 28
SK_SEED = 31
PARAMS = dict(K=16, degree=31, double_angles=3, cts_groups=3, stc_groups=3, delta=DELTA,
              hamming_weight=HAMMING)
OUT_LEVEL = 3


def apply_factors(factors, v, const=1.0):
    for f in factors:
        v = sum(d * const * np.roll(v, -k) for k, d in f.items())
    return v


def model_slots(count, seed):
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, count) + 1j * g.uniform(-1, 1, count)


def model(log_n, q0, delta=DELTA, K=16, degree=31, double_angles=3, groups=3, exact_sine=True,
          noise=0.0, seed=3):
    """The pipeline on float64 slot vectors with the Bootstrapper's constants: slots uniform in
    [-1, 1]^2, I uniform in [-(K-1), K-1], t = m + q_0 I, CoeffToSlot with delta / (2 n K q_0)
    (the declared scale delta divided out), the split, sin(2 pi K v) / (2 pi) exactly or by
    eval_mod's interpolant and double angles, optional normal noise on its output, the merge,
    SlotToCoeff with q_0 / delta.  Returns the maximum slot error."""
    from fhecore import bootstrap as bs

    n = 1 << (log_n - 1)
    g = np.random.default_rng(seed)
    z = g.uniform(-1, 1, n) + 1j * g.uniform(-1, 1, n)
    cts, stc = bs.dft_factors(log_n, groups, True), bs.dft_factors(log_n, groups, False)
    w = apply_factors(cts, z) * delta / n  # c_k + i c_{k+n}, in the network's order
    m = np.rint(w.real) + 1j * np.rint(w.imag)
    big_i = g.integers(-(K - 1), K, n) + 1j * g.integers(-(K - 1), K, n)
    raw = apply_factors(stc, m + q0 * big_i)  # the raised ciphertext's slots times its scale
    y = apply_factors(cts, raw, (1 / (2.0 * n * K * q0)) ** (1 / groups))

    def eval_mod(v):
        if exact_sine:
            e = np.sin(2 * np.pi * K * v) / (2 * np.pi)
        else:
            c = np.polynomial.chebyshev.chebinterpolate(
                lambda x: np.cos((2 * np.pi * K * x - np.pi / 2) / 2 ** double_angles), degree)
            e = np.polynomial.chebyshev.chebval(v, c)
            for _ in range(double_angles):
                e = 2 * e * e - 1
            e = e / (2 * np.pi)
        return e + g.normal(0, noise, n) if noise else e

    merged = eval_mod(2 * y.real) + 1j * eval_mod(2 * y.imag)
    out = apply_factors(stc, merged, (q0 / delta) ** (1 / groups))
    return float(np.abs(out - z).max())


# ---- the shared case's chain and rotation keys (the case itself: tests/cases.py BOOTSTRAP) --------

def moduli():
    q0 = [int(q) for q in pyoracle.gen_moduli(LOG_N, 1, bits=Q0_BITS)]
    rest = [int(q) for q in pyoracle.gen_moduli(LOG_N, L - 1 + NSPECIAL, bits=BITS)]
    return q0 + rest[:L - 1], rest[L - 1:]


def rotation_elements():
    """The Galois elements of every baby / giant step of the six factors, and the conjugation."""
    from fhecore import bootstrap as bs

    n = 1 << LOG_N
    steps = set()
    for inverse, groups in ((True, PARAMS["cts_groups"]), (False, PARAMS["stc_groups"])):
        for n1, n2, stride, offset in bs.factor_layouts(LOG_N, groups, inverse):
            steps |= {stride * (b + offset) for b in range(n1)} | {stride * g * n1 for g in range(n2)}
    return sorted({pyoracle.galois_elt(s, n) for s in steps if s % (n // 2)} | {2 * n - 1})
