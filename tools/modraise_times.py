"""Times ModRaise (fhe_mod_raise) at the key-switch configuration (N = 2^16, L = 16, K = 4,
dnum = 4, batch 32), from level 1 to levels 16 and 4, in one process, three forms of one result:

  * fused:    the shipped path of narrow contexts -- inverse NTT of limb 0, the lift folded into
              the column-forward pass of the limbs above it (k_lift_col), row-forward pass,
              copy of limb 0;
  * unfused:  the path of wide contexts forced on the same context (FHECORE_MODRAISE_UNFUSED=1,
              read by every call) -- a separate spread pass into the output, then a whole forward
              NTT in place;
  * composed: the same result from public whole-tensor calls -- ctx.intt of limb 0, a torch
              elementwise centred lift (residues below 2^60 fit int64), ctx.ntt over the limbs
              (composed_mod_raise below; tests/test_gpu_modraise.py checks it against mod_raise).

Device events around `--steps` calls after `--warmup` calls of the same shape; the three forms of
one case are timed back to back, `--rounds` times alternating, and the median is reported.  One
JSON line per case: ms per call of the three forms, the ratios, and the fused call's algorithmic
bytes, 8 * 2 * batch * N * (1 + out_level), over its time as a fraction of the 8 TB/s HBM peak.

  python tools/modraise_times.py [--levels 16 4] [--steps 50] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-fhe_amd"))
import fhecore as fc  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (MI355X spec)
UNFUSED = "FHECORE_MODRAISE_UNFUSED"


def composed_mod_raise(ctx, ct, level):
    """mod_raise(ct, level) from ctx.intt, torch and ctx.ntt: ct [..., 2, l, N] int64 residues of
    a context whose moduli are all below 2^62 (the centred lift and torch.remainder stay in
    int64)."""
    q0 = ctx.moduli[0]
    x = ctx.intt(ct[..., :1, :].contiguous())  # [..., 2, 1, N]
    c = torch.where(x > (q0 - 1) // 2, x - q0, x)
    res = torch.cat([torch.remainder(c, q) for q in ctx.moduli[:level]], dim=-2)
    return ctx.ntt_(res)


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
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("modraise_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B = 1 << log_n, args.batch
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    q0 = ctx.moduli[0]
    ct = torch.remainder(torch.randint(0, 2**62, (B, 2, 1, n), generator=gen, device="cuda",
                                       dtype=torch.int64), q0)  # level 1
    ws = ctx.workspace(fc.load().fhe_mod_raise_workspace(ctx.handle, B))
    sink = open(args.out, "a") if args.out else None
    os.environ.pop(UNFUSED, None)

    for level in args.levels:
        out = torch.empty(B, 2, level, n, dtype=torch.int64, device="cuda")

        def fused():
            ctx.mod_raise(ct, level, workspace=ws, out=out)

        def unfused():
            os.environ[UNFUSED] = "1"
            try:
                ctx.mod_raise(ct, level, workspace=ws, out=out)
            finally:
                del os.environ[UNFUSED]

        def composed():
            composed_mod_raise(ctx, ct, level)

        want = composed_mod_raise(ctx, ct, level)
        for form in (fused, unfused):
            out.zero_()
            form()
            torch.cuda.synchronize()
            assert torch.equal(out, want), f"{form.__name__} mod_raise differs from its composition"
        del want
        f, u, c = [], [], []
        for _ in range(args.rounds):
            f.append(timed_ms(fused, args.steps, args.warmup))
            u.append(timed_ms(unfused, args.steps, args.warmup))
            c.append(timed_ms(composed, args.steps, args.warmup))
        f, u, c = (statistics.median(v) for v in (f, u, c))
        nbytes = 8 * 2 * B * n * (1 + level)
        rec = {"op": "mod_raise", "in_level": 1, "out_level": level, "batch": B, "log_n": log_n,
               "fused_ms": round(f, 4), "unfused_ms": round(u, 4), "composed_ms": round(c, 4),
               "unfused_over_fused": round(u / f, 3), "composed_over_fused": round(c / f, 3),
               "fused_algorithmic_bytes": nbytes, "fused_GBps": round(nbytes / f / 1e6, 1),
               "fused_frac_hbm_peak": round(nbytes / (f * 1e-3) / HBM_PEAK, 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        del out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
