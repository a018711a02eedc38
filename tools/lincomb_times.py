"""Times the fused plaintext arithmetic against its composition from whole-tensor passes, at the
key-switch configuration (N = 2^16, L = 16, K = 4, dnum = 4, batch 32), levels 16 and 4, all with
rescale off, in one process:

  * lincomb with 2, 4 and 8 terms (fhe_lincomb_level, 8 (terms + 1) B per element) against the same
    combination from ctx.vec('mul') with pre-materialised constant rows [batch][2][l][N] and
    ctx.vec('add') (24 B per element per pass, 2 terms - 1 passes);
  * mul_plain (fhe_mul_plain_level, one plaintext for the batch) against ctx.vec('mul') on both
    components (the plaintext expanded to [batch][2][l][N] beforehand).

Device events around `--steps` calls after `--warmup` calls of the same shape; fused and composed
forms of one case are timed back to back, `--rounds` times alternating, and the median is reported.
One JSON line per case: ms per call of both forms, their ratio, and the fused form's algorithmic
bytes over its time as a fraction of the 8 TB/s HBM peak.

  python tools/lincomb_times.py [--levels 16 4] [--steps 50] [--warmup 20] [--out FILE]"""
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
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--terms", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lincomb_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B = 1 << log_n, args.batch
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    tmax = max(args.terms)
    ks = [3 ** (40 + t) for t in range(tmax)]
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def compare(fused, composed):
        f, c = [], []
        for _ in range(args.rounds):
            f.append(timed_ms(fused, args.steps, args.warmup))
            c.append(timed_ms(composed, args.steps, args.warmup))
        return statistics.median(f), statistics.median(c)

    for level in args.levels:
        ql = ctx.moduli[:level]
        elems = B * 2 * level * n
        cts = [uniform(gen, ql, (B, 2), n) for _ in range(tmax)]
        out, tmp = torch.empty_like(cts[0]), torch.empty_like(cts[0])
        # the composition's constants: one [batch][2][l][N] tensor per term, every element k mod q_l
        rows = [torch.tensor([k % q for q in ql], dtype=torch.int64, device="cuda")
                .view(1, 1, level, 1).expand(B, 2, level, n).contiguous() for k in ks]
        for terms in args.terms:
            tab = ctx.encode_scalars(ks[:terms], exact=True)

            def fused():
                ctx.lincomb(cts[:terms], tab, level=level, out=out)

            def composed():
                ctx.vec("mul", cts[0], rows[0], out=out)
                for t in range(1, terms):
                    ctx.vec("mul", cts[t], rows[t], out=tmp)
                    ctx.vec("add", out, tmp, out=out)

            composed()
            want = out.clone()
            fused()
            torch.cuda.synchronize()
            assert torch.equal(out, want), "fused lincomb differs from its composition"
            f, c = compare(fused, composed)
            nbytes = 8 * (terms + 1) * elems
            emit({"op": "lincomb", "terms": terms, "level": level, "batch": B, "log_n": log_n,
                  "fused_ms": round(f, 4), "composed_ms": round(c, 4), "speedup": round(c / f, 3),
                  "fused_bytes_per_elem": 8 * (terms + 1),
                  "composed_bytes_per_elem": 24 * (2 * terms - 1),
                  "fused_GBps": round(nbytes / f / 1e6, 1),
                  "fused_frac_hbm_peak": round(nbytes / (f * 1e-3) / HBM_PEAK, 4)})
        pt = uniform(gen, ctx.all_moduli, (), n)  # [L + K][N], read in place at every level
        pt_exp = pt[:level].view(1, 1, level, n).expand(B, 2, level, n).contiguous()
        ctx.vec("mul", cts[0], pt_exp, out=tmp)
        ctx.mul_plain(cts[0], pt, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, tmp), "fused mul_plain differs from vec mul"
        f, c = compare(lambda: ctx.mul_plain(cts[0], pt, out=out),
                       lambda: ctx.vec("mul", cts[0], pt_exp, out=tmp))
        nbytes = 16 * elems + 8 * level * n  # ct in and out, the plaintext once
        emit({"op": "mul_plain", "level": level, "batch": B, "log_n": log_n,
              "fused_ms": round(f, 4), "composed_ms": round(c, 4), "speedup": round(c / f, 3),
              "fused_bytes_per_elem": 16, "composed_bytes_per_elem": 24,
              "fused_GBps": round(nbytes / f / 1e6, 1),
              "fused_frac_hbm_peak": round(nbytes / (f * 1e-3) / HBM_PEAK, 4)})
        del cts, rows, out, tmp, pt_exp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
