"""Times the sum of ciphertext products with one relinearisation (fhe_mul_sum_relin_level) against
its composition from today's calls, at the key-switch configuration (N = 2^16, L = 16, K = 4,
dnum = 4, batch 32), levels 16 and 4, 1, 2, 4, 8 and 16 terms, in one process:

  * fused: one mul_sum_relin(rescale=True);
  * composed: one mul_relin(rescale=False) per term, then one lincomb with unit scalars and
    rescale=True over the products (the sum and the rescale in lincomb's one pass plus its rescale:
    the cheapest composition the library offers).  At one term the composition is
    mul_relin(rescale=True) itself, and the record carries its run-to-run spread over the rounds.

All 2 x terms operands are distinct tensors, so no operand is served from a cache.  Device events
around `--steps` calls after `--warmup` calls of the same shape; the two forms of one case are timed
back to back, `--rounds` times alternating, and the median is reported.  The tensor kernels are timed
alone through the library's per-launch events (fhe_prof_begin / fhe_prof_end): k_tensor_sum_ntt's
algorithmic bytes, 8 (4 terms + 3) per element, over its time as a share of the 8 TB/s HBM peak,
beside k_tensor_ntt's (56 bytes per element) in the same process.  One JSON line per case.

  python tools/mulsum_times.py [--levels 16 4] [--terms 1 2 4 8 16] [--steps 20] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-fhe_amd"))
import fhecore as fc  # noqa: E402
from fhecore._capi import check  # noqa: E402

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


def mark_ms(fn, name, reps=10):
    """Milliseconds per call of fn spent in the library launches marked `name`."""
    lib = fc.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap = 64 * reps + 16
    fn()
    torch.cuda.synchronize()
    check(lib.fhe_prof_begin(cap, st), "fhe_prof_begin")
    for _ in range(reps):
        fn()
    ms = (ctypes.c_float * cap)()
    cnt = ctypes.c_uint32()
    names = ctypes.create_string_buffer(64 * cap)
    check(lib.fhe_prof_end(ms, cap, ctypes.byref(cnt), names, 64 * cap), "fhe_prof_end")
    return sum(v for nm, v in zip(names.value.decode().split("\n"), ms[:cnt.value])
               if nm == name) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--terms", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mulsum_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B = 1 << log_n, args.batch
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    lib = fc.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    tmax = max(args.terms)
    kb, ka = uniform(gen, ctx.all_moduli, (dnum,), n), uniform(gen, ctx.all_moduli, (dnum,), n)
    ws = ctx.workspace(lib.fhe_mul_relin_workspace(ctx.handle,
                                                   lib.fhe_keyswitch_pass_batch(ctx.handle, B)))
    lws = ctx.workspace(lib.fhe_lincomb_workspace(ctx.handle, B))
    ones = ctx.encode_scalars([1] * tmax, exact=True)
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for level in args.levels:
        ql = ctx.moduli[:level]
        elems = B * level * n  # per tensor component
        As = [uniform(gen, ql, (B, 2), n) for _ in range(tmax)]
        Bs = [uniform(gen, ql, (B, 2), n) for _ in range(tmax)]
        prods = [torch.empty_like(As[0]) for _ in range(tmax)]
        out = torch.empty(B, 2, level - 1, n, dtype=torch.int64, device="cuda")
        ref = torch.empty_like(out)

        def mul_relin():
            ctx.mul_relin(As[0], Bs[0], kb, ka, rescale=True, workspace=ws, out=ref)

        t_ms = mark_ms(mul_relin, "tensor_ntt")
        tensor_share = 56 * elems / (t_ms * 1e-3) / HBM_PEAK
        for terms in args.terms:
            def fused():
                ctx.mul_sum_relin(As[:terms], Bs[:terms], kb, ka, rescale=True, level=level,
                                  workspace=ws, out=out)

            def composed():
                if terms == 1:
                    return mul_relin()
                for t in range(terms):
                    ctx.mul_relin(As[t], Bs[t], kb, ka, rescale=False, workspace=ws, out=prods[t])
                ctx.lincomb(prods[:terms], ones, rescale=True, level=level, workspace=lws, out=ref)

            composed()
            fused()
            torch.cuda.synchronize()
            # (from two terms up the forms differ in the key-switch's rounding: one ModDown of the
            # summed d2 against one per term; tests/test_gpu_mulsum.py holds the exact checks)
            assert terms > 1 or torch.equal(out, ref), "one-term mul_sum_relin differs from mul_relin"
            f, c = [], []
            for _ in range(args.rounds):
                f.append(timed_ms(fused, args.steps, args.warmup))
                c.append(timed_ms(composed, args.steps, args.warmup))
            fm, cm = statistics.median(f), statistics.median(c)
            # (one term at the operands' level runs k_tensor_ntt: no tensor_sum_ntt mark)
            k_ms = mark_ms(fused, "tensor_sum_ntt") or None
            nbytes = 8 * (4 * terms + 3) * elems
            emit({"op": "mul_sum_relin", "terms": terms, "level": level, "batch": B, "log_n": log_n,
                  "fused_ms": round(fm, 4), "composed_ms": round(cm, 4),
                  "speedup": round(cm / fm, 3),
                  "fused_ms_rounds": [round(v, 4) for v in f],
                  "composed_ms_rounds": [round(v, 4) for v in c],
                  "tensor_sum_ms": k_ms and round(k_ms, 4),
                  "tensor_sum_bytes_per_elem": 8 * (4 * terms + 3),
                  "tensor_sum_frac_hbm_peak": k_ms and round(nbytes / (k_ms * 1e-3) / HBM_PEAK, 4),
                  "tensor_ntt_ms": round(t_ms, 4),
                  "tensor_ntt_frac_hbm_peak": round(tensor_share, 4)})
        del As, Bs, prods, out, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
