"""What the reference-based tests share: the C oracle's NTT pair for pyoracle's ntt= argument, and
the seeded inputs and cases behind tests/golden/level_refs.json, the digests that pin pyoracle's
key-switch family at every level (tests/golden/make_golden.py level_refs writes them,
tests/test_level_hoist_cpu.py recomputes them)."""
import hashlib
import random

import numpy as np

import coracle
import pyoracle


def _fwd(x, mods):
    return coracle.ntt_fwd(np.asarray(x, dtype=np.uint64), mods).astype(object)


def _inv(x, mods):
    return coracle.ntt_inv(np.asarray(x, dtype=np.uint64), mods).astype(object)


def c_ntt():
    """(fwd, inv) for pyoracle's ntt= argument: the C restatement's transforms, bit-identical to
    pyoracle.rns_ntt_fwd / rns_ntt_inv and much faster at N >= 2^10."""
    return _fwd, _inv


def relin_setup(log_n, L, K, dnum, seed):
    """Moduli, a ternary secret and its real relinearisation key; rng is left where the key
    generation stopped, for the caller's own draws."""
    n = 1 << log_n
    m = pyoracle.gen_moduli(log_n, L + K)
    qs, ps = [int(q) for q in m[:L]], [int(p) for p in m[L:]]
    rng = random.Random(seed)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    evk_b, evk_a = pyoracle.gen_relin_key(s, qs, ps, dnum, rng)
    return n, qs, ps, rng, s, evk_b, evk_a


def hoist_world(log_n=10, L=5, K=2, dnum=3):
    """Moduli, a ternary secret, three real ciphertexts, rotation keys and plaintext diagonals
    (ranges as in tests/test_gpu_rotsum.py) from random.Random(2024)."""
    n = 1 << log_n
    mods = pyoracle.gen_moduli(log_n, L + K, 60)
    qs, ps = [int(q) for q in mods[:L]], [int(p) for p in mods[L:]]
    allm = qs + ps
    rng = random.Random(2024)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    ntt = lambda v, m: _fwd(pyoracle._to_rns(v, m), m)  # noqa: E731
    s_n = ntt(s, qs)
    col = pyoracle._mods_col(qs)
    cts, msgs = [], []
    for _ in range(3):
        m = [rng.randrange(-1000, 1000) for _ in range(n)]
        a = np.stack([np.array([rng.randrange(q) for _ in range(n)], dtype=object) for q in qs])
        e = ntt([rng.randrange(-3, 4) for _ in range(n)], qs)
        cts.append(np.stack([(-a * s_n + e + ntt(m, qs)) % col, a]).astype(np.uint64))
        msgs.append(m)
    ks = [1, pyoracle.galois_elt(1, n), pyoracle.galois_elt(-2, n), 2 * n - 1]
    keys = {}
    for k in ks[1:]:
        kb, ka = pyoracle.gen_rot_key(s, k, qs, ps, dnum, rng)
        keys[k] = (kb.astype(np.uint64), ka.astype(np.uint64))
    pt_int = [[rng.randrange(-3, 4) for _ in range(n)] for _ in range(4)]
    pts = [coracle.ntt_fwd(np.asarray(pyoracle._to_rns(p, allm), dtype=np.uint64), allm)
           for p in pt_int]
    return dict(log_n=log_n, dnum=dnum, qs=qs, ps=ps, s_n=s_n, cts=cts, msgs=msgs, ks=ks, keys=keys,
                pt_int=pt_int, pts=pts)


def small_world(log_n, L, K, dnum):
    """A hoist_world-shaped dict on relin_setup(log_n, L, K, dnum, seed=20 + L) (the shapes of
    tests/test_levels_cpu.py): uniform ciphertexts and plaintexts drawn after the key, which
    serves every Galois element (the pinned results are words, not decryptions)."""
    n, qs, ps, rng, _, evk_b, evk_a = relin_setup(log_n, L, K, dnum, seed=20 + L)

    def uniform(mods):
        return np.stack([np.array([rng.randrange(q) for _ in range(n)], dtype=np.uint64)
                         for q in mods])

    cts = [np.stack([uniform(qs), uniform(qs)]) for _ in range(3)]
    pts = [uniform(qs + ps) for _ in range(4)]
    ks = [1, pyoracle.galois_elt(1, n), pyoracle.galois_elt(-2, n), 2 * n - 1]
    key = (evk_b.astype(np.uint64), evk_a.astype(np.uint64))
    return dict(log_n=log_n, dnum=dnum, qs=qs, ps=ps, cts=cts, ks=ks, keys={k: key for k in ks[1:]},
                pts=pts)


PIN_SMALL = [(6, 5, 2, 3), (6, 7, 4, 2)]


def cut(ct, level):
    return np.ascontiguousarray(np.asarray(ct)[..., :level, :])


def level_cases(w, level):
    """{name: f(ops, **kw)}: the seven operations on the world w at `level`; ops is pyoracle (or
    anything with its signatures), kw its level= / ntt= keywords."""
    qs, ps, dnum, log_n, ks = w["qs"], w["ps"], w["dnum"], w["log_n"], w["ks"]
    a, b, c = (cut(t, level) for t in w["cts"])
    kb, ka = w["keys"][ks[1]]
    tail = (qs, ps, dnum)
    keys = [w["keys"].get(k) for k in ks]
    mk = [ks[1], 1, ks[3]]
    baby, giant = [1, ks[1]], [1, ks[2]]
    cases = {
        "keyswitch": lambda o, **kw: np.stack(o.keyswitch(a[1], kb, ka, *tail, **kw)),
        "rotate": lambda o, **kw: o.rotate(a, ks[1], kb, ka, *tail, log_n, **kw),
        "mul_relin": lambda o, **kw: o.mul_relin(a, b, kb, ka, *tail, False, **kw),
        "rotate_hoisted": lambda o, **kw: o.rotate_hoisted(a, ks[1:], keys[1:], *tail, log_n, **kw),
        "rotate_sum_hoisted": lambda o, **kw: o.rotate_sum_hoisted(a, ks, keys, w["pts"], *tail,
                                                                   log_n, **kw),
        "rotate_sum_multi": lambda o, **kw: o.rotate_sum_multi(
            [a, b, c], mk, [w["keys"].get(k) for k in mk], *tail, log_n, **kw),
        "linear_transform": lambda o, **kw: o.linear_transform(
            a, baby, [w["keys"].get(k) for k in baby], giant, [w["keys"].get(k) for k in giant],
            [w["pts"][:2], w["pts"][2:]], *tail, log_n, **kw),
    }
    if level >= 2:
        cases["mul_relin_rescale"] = lambda o, **kw: o.mul_relin(a, b, kb, ka, *tail, True, **kw)
    return cases


def level_digests(w, ops, ntt):
    """{"shape/op/level": sha256 of the result's uint64 bytes} for every case at every level."""
    L = len(w["qs"])
    shape = f"n{w['log_n']}_L{L}_K{len(w['ps'])}_d{w['dnum']}"
    out = {}
    for level in range(1, L + 1):
        for name, f in level_cases(w, level).items():
            words = np.ascontiguousarray(np.asarray(f(ops, level=level, ntt=ntt), dtype=np.uint64))
            out[f"{shape}/{name}/{level}"] = hashlib.sha256(words.tobytes()).hexdigest()
    return out


# ---- tests/golden/op_refs.json: the operations that joined pyoracle after the key-switch family ----
# (make_golden.py --op-refs writes the digests, tests/test_op_refs_cpu.py recomputes them)

PIN_OPS = PIN_SMALL + [(10, 4, 2, 2)]
SPARSE_H = (1, 28, None)  # None: h = N


def words(x):
    """Python integers or int64 (signed: two's complement) -> the uint64 words that are hashed."""
    return np.ascontiguousarray(np.asarray(np.asarray(x).astype(object) % (1 << 64), dtype=np.uint64))


def op_cases(w, level):
    """{name: f(ops, ntt)}: every operation of the plaintext-arithmetic, mul-sum, ModRaise and
    split / merge families on the world w at `level`, inputs at mixed levels where the operation
    takes them; ops is pyoracle (or anything with its signatures)."""
    qs, ps, dnum = w["qs"], w["ps"], w["dnum"]
    L = len(qs)
    a, b, c = w["cts"]  # all at level L
    up = min(level + 1, L)
    kb, ka = w["keys"][w["ks"][1]]
    scalars = [-(1 << 70) + 12345, (1 << 59) + 7, 1]
    mixed = [cut(a, level), b, cut(c, up)]
    As, Bs = [cut(a, level), b, cut(c, up), a], [b, cut(c, up), cut(c, up), cut(a, level)]
    cases = {
        "lincomb": lambda o, ntt: o.lincomb(mixed, scalars, qs, level=level, ntt=ntt),
        "lincomb_const": lambda o, ntt: o.lincomb(mixed, scalars, qs, level=level,
                                                  const=-(1 << 65) + 99, ntt=ntt),
        "mul_plain": lambda o, ntt: o.mul_plain(cut(a, level), w["pts"][0], qs, level=level, ntt=ntt),
        "tensor_sum": lambda o, ntt: o.tensor_sum(As, Bs, qs, level=level),
        "relin": lambda o, ntt: o.relin(o.tensor_sum(As, Bs, qs, level=level), kb, ka, qs, ps, dnum,
                                        False, level=level, ntt=ntt),
        "mul_sum_relin": lambda o, ntt: o.mul_sum_relin(As, Bs, kb, ka, qs, ps, dnum, False,
                                                        level=level, ntt=ntt),
        "centred_lift": lambda o, ntt: o.centred_lift(cut(a, level), qs, ntt),
        "mul_x_half": lambda o, ntt: o.mul_x_half(cut(a, level), qs[:level], ntt),
        "conj_split": lambda o, ntt: np.stack(o.conj_split(cut(a, level), cut(b, level), qs,
                                                           level=level, ntt=ntt)),
        "conj_merge": lambda o, ntt: o.conj_merge(cut(a, level), cut(b, level), qs, level=level,
                                                  ntt=ntt),
    }
    if level >= 2:
        cases.update({
            "rescale_ct": lambda o, ntt: o.rescale_ct(cut(a, level), qs[:level], ntt),
            "lincomb_rescale": lambda o, ntt: o.lincomb(mixed, scalars, qs, level=level,
                                                        const=-(1 << 65) + 99, rescale=True, ntt=ntt),
            "mul_plain_rescale": lambda o, ntt: o.mul_plain(cut(a, level), w["pts"][0], qs,
                                                            level=level, rescale=True, ntt=ntt),
            "relin_rescale": lambda o, ntt: o.relin(o.tensor_sum(As, Bs, qs, level=level), kb, ka, qs,
                                                    ps, dnum, True, level=level, ntt=ntt),
            "mul_sum_relin_rescale": lambda o, ntt: o.mul_sum_relin(As, Bs, kb, ka, qs, ps, dnum,
                                                                    True, level=level, ntt=ntt),
        })
    return cases


def world_cases(w):
    """{name: f(ops, ntt)}: the cases that are not per level.  mod_raise from level 1 and from
    level 3 (a batch of two ciphertexts) to 1, 2 and L; the sparse secret at h = 1, 28 and N."""
    qs, ps, log_n = w["qs"], w["ps"], w["log_n"]
    L = len(qs)
    both = np.stack(w["cts"][:2])
    cases = {}
    for i in (1, 3):
        for o_ in (1, 2, L):
            cases[f"mod_raise_{i}_{o_}"] = (lambda o, ntt, i=i, o_=o_:
                                            o.mod_raise(cut(both, i), qs, i, o_, ntt=ntt))
    for h in SPARSE_H:
        h = h or 1 << log_n
        cases[f"sparse_secret_coefficients_h{h}"] = (lambda o, ntt, h=h:
                                                     o.sparse_secret_coefficients(41, h, log_n))
        cases[f"keygen_secret_sparse_h{h}"] = (lambda o, ntt, h=h:
                                               o.keygen_secret_sparse(41, h, qs + ps, log_n))
    return cases


def op_digests(w, ops, ntt):
    """{"shape/op/level": sha256 of words(result)}; level 0 marks the cases of world_cases."""
    L = len(w["qs"])
    shape = f"n{w['log_n']}_L{L}_K{len(w['ps'])}_d{w['dnum']}"
    runs = [(0, world_cases(w))] + [(level, op_cases(w, level)) for level in range(1, L + 1)]
    return {f"{shape}/{name}/{level}": hashlib.sha256(words(f(ops, ntt)).tobytes()).hexdigest()
            for level, cases in runs for name, f in cases.items()}
