"""The EvalMod case the CPU and GPU tests share (fhecore.polyeval.eval_mod), computed once per
process on plain_ref.CpuBackend:

  log_n = 10, L = 12, 3 special primes, dnum = 4, a 50-bit chain, delta = 2^50, fixed seeds;
  mod-range K = 16 (eval_mod's parameter, not the special-prime count), degree 31, 3 double angles:
  6 + 3 = 9 levels, so the result is at level 3;
  slots v = (I + eps) / 16, I uniform in [-15, 15], eps uniform in [-2^-8, 2^-8].

The result's slots hold sin(2 pi K v) / (2 pi), which is eps up to (2 pi)^2 |eps|^3 / 6."""
import functools
import math
import random

import numpy as np

import plain_ref
import pyoracle

LOG_N, L, NSPECIAL, DNUM, BITS = 10, 12, 3, 4, 50
DELTA = 2.0 ** 50
K, DEGREE, DOUBLE_ANGLES = 16, 31, 3
EPS_MAX = 2.0 ** -8
# the cubic term the choice of eps accepts: EvalMod's own error must stay below it (a condition,
# not a measurement)
CAP = (2 * math.pi) ** 2 * EPS_MAX ** 3 / 6
# maximum slot error of eval_mod on the CPU backend against float64 sin(2 pi K v) / (2 pi),
# measured once (deterministic under the seeds below).  In plain float64 the polynomial and the
# double angles alone give 5.5e-10 at these parameters; the rest is the evaluator's scale drift
# (the primes sit ~2^-30 off delta, chebyshev_eval's docstring) and the encryption and rescale
# noise, doubled by each of the three double-angle steps.
EVALMOD_ERR = 1.051e-08
# over the constant: float differences between numpy builds in the decode only
MARGIN = 1.05


@functools.lru_cache(maxsize=None)
def setup():
    """Keys and the encrypted input from pyoracle with fixed seeds: dict of host arrays."""
    import coracle
    from fhecore.ckks import Encoder, to_rns

    n = 1 << LOG_N
    m = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + NSPECIAL, bits=BITS)]
    qs, ps = m[:L], m[L:]
    rng = random.Random(4321)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    evk_b, evk_a = pyoracle.gen_relin_key(s, qs, ps, DNUM, rng)
    sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, m), m)
    v, eps = slots(n // 2)
    enc = Encoder(n)
    pt = coracle.ntt_fwd(to_rns(enc.encode(v, DELTA), qs), qs)
    ct = pyoracle.encrypt_sk(78, pt, sk_ntt, qs, LOG_N)
    return dict(qs=qs, ps=ps, evk_b=evk_b, evk_a=evk_a, sk_ntt=sk_ntt, v=v, eps=eps, ct=ct, enc=enc,
                pt=pt)


def slots(count):
    """(v, eps): v = (I + eps) / K."""
    g = np.random.default_rng(6)
    big_i = g.integers(-(K - 1), K, count)
    eps = g.uniform(-EPS_MAX, EPS_MAX, count)
    return (big_i + eps) / K, eps


def target(v):
    return np.sin(2 * np.pi * K * v) / (2 * np.pi)


def decode(dec, level, scale):
    """A decrypted plaintext (level, N), NTT form -> the real parts of the slots."""
    import coracle
    from fhecore.ckks import from_rns

    su = setup()
    ql = su["qs"][:level]
    coef = from_rns(coracle.ntt_inv(np.asarray(dec, dtype=np.uint64), ql), ql)
    return su["enc"].decode(coef, float(scale)).real


def decrypt_decode(data, level, scale):
    su = setup()
    dec = pyoracle.decrypt(np.asarray(data).astype(object), su["sk_ntt"], su["qs"][:level])
    return decode(dec, level, scale)


def backend():
    su = setup()
    return plain_ref.CpuBackend(su["qs"], su["ps"], DNUM, su["evk_b"], su["evk_a"])


@functools.lru_cache(maxsize=None)
def evalmod_cpu():
    """eval_mod on the CPU backend: (Ct with a (2, 3, N) object array, max slot error)."""
    from fhecore import polyeval

    su = setup()
    out = polyeval.eval_mod(backend(), polyeval.Ct(su["ct"], L, DELTA), K, DEGREE, DOUBLE_ANGLES)
    got = decrypt_decode(out.data, out.level, out.scale)
    return out, float(np.abs(got - target(su["v"])).max())
