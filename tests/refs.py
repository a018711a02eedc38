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
