"""Times fhe_rotate_sum_hoisted (8 terms) and fhe_linear_transform (4 x 4) at several levels of the
key-switch configuration (N = 2^16, L = 16, K = 4, dnum = 4, batch 32) with the top-level keys and
plaintexts, and prints one JSON line per (operation, level) beside the level's share of the
top-level work, dl (l + K) / (dnum (L + K)) -- report only: whether lower levels get proportionally
cheaper.  Device events around `--steps` calls after `--warmup` calls of the same shape.

  python tools/level_hoist_times.py [--levels 16 12 8 4] [--steps 50] [--warmup 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-fhe_amd"))
import fhecore as fc  # noqa: E402


def uniform(gen, mods, lead, n):
    """Residues in [0, q_l) per limb: int64 device tensor [*lead, len(mods), n]."""
    return torch.stack([torch.remainder(torch.randint(0, 2**62, lead + (n,), generator=gen,
                                                      device="cuda", dtype=torch.int64), q)
                        for q in mods], dim=len(lead)).contiguous()


def timed_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 12, 8, 4])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("level_hoist_times: needs a HIP device")
    log_n, L, K, dnum, R, n1, n2 = 16, 16, 4, 4, 8, 4, 4
    n, B = 1 << log_n, args.batch
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    alpha = -(-L // dnum)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    key = lambda: (uniform(gen, ctx.all_moduli, (dnum,), n),  # noqa: E731
                   uniform(gen, ctx.all_moduli, (dnum,), n))
    elts = [1] + [ctx.galois_elt(r) for r in range(1, R)]
    keys = [None] + [key() for _ in range(1, R)]
    pts = [uniform(gen, ctx.all_moduli, (), n) for _ in range(max(R, n1 * n2))]
    baby = [1] + [ctx.galois_elt(b) for b in range(1, n1)]
    giant = [1] + [ctx.galois_elt(g * n1) for g in range(1, n2)]
    bkeys, gkeys = [None] + keys[1:n1], [None] + keys[n1:n1 + n2 - 1]
    lpts = [pts[g * n1:(g + 1) * n1] for g in range(n2)]
    lib = fc.load()
    ws = ctx.workspace(max(lib.fhe_rotate_sum_hoisted_workspace(ctx.handle, B),
                           lib.fhe_linear_transform_workspace(ctx.handle, n2, B)))
    top = {}
    for level in args.levels:
        ct = uniform(gen, ctx.moduli[:level], (B, 2), n)
        out = torch.empty_like(ct)
        ops = {
            "rotate_sum_hoisted": lambda: ctx.rotate_sum_hoisted(ct, elts, keys, pts[:R],
                                                                 workspace=ws, out=out),
            "linear_transform": lambda: ctx.linear_transform(ct, baby, bkeys, giant, gkeys, lpts,
                                                             workspace=ws, out=out),
        }
        dl = -(-level // alpha)
        for name, fn in ops.items():
            ms = timed_ms(fn, args.steps, args.warmup)
            if level == L:
                top[name] = ms
            print(json.dumps({
                "op": name, "level": level, "digits": dl, "batch": B, "ms_per_call": round(ms, 4),
                "work_ratio": round(dl * (level + K) / (dnum * (L + K)), 4),
                "time_ratio": round(ms / top[name], 4) if name in top else None}), flush=True)


if __name__ == "__main__":
    main()
