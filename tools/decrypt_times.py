"""Times fhe_decrypt_slots against what a caller wrote before it, fhe_decrypt -> fhe_decode(_sparse),
in the same process, at the key-switch configuration (N = 2^16, L = 16, K = 4, dnum = 4, batch 32):
levels 16, 4, 2 and 1, full packing and 2^10 slots.

The two forms are checked word for word before anything is timed.  Device events around `--steps`
calls after `--warmup` calls; per round the new call is timed before and after the composed one,
`--rounds` times.  One JSON line per case: the median ms of either form, `spread_ms` (what the new
call's two medians differ by in this run), the ratio, `slower_beyond_spread` (new - composed >
spread: the one thing that must not happen), the unfused form (FHECORE_DECRYPT_UNFUSED), the bytes
either form's decrypting step moves by the algorithm (composed: 4 level words per coefficient;
fused first pass: 3 nl + nl, nl = min(level, 2)) and the per-launch marks of both forms from the
library's own events (fhe_prof_begin / fhe_prof_end; a mark spans everything since the mark before
it, so the composed form's fhe_decrypt, which has no mark of its own, is inside ntt_row_inv).  A
call takes about 0.1 ms, hence the many steps per timed window.

  python tools/decrypt_times.py [--steps 1000] [--warmup 50] [--rounds 3] [--out FILE]"""
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

SEED = 0x5EED_0000_0000


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


def marks_of(fn, reps=5):
    """ms per call of every per-launch mark of fn's library launches."""
    lib = fc.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap = 32 * reps + 16
    check(lib.fhe_prof_begin(cap, st), "fhe_prof_begin")
    for _ in range(reps):
        fn()
    ms = (ctypes.c_float * cap)()
    cnt = ctypes.c_uint32()
    names = ctypes.create_string_buffer(64 * cap)
    check(lib.fhe_prof_end(ms, cap, ctypes.byref(cnt), names, 64 * cap), "fhe_prof_end")
    per = {}
    for nm, v in zip(names.value.decode().split("\n"), ms[:cnt.value]):
        per[nm] = per.get(nm, 0.0) + v / reps
    per.pop("begin", None)
    return {k: round(v, 4) for k, v in per.items()}


def with_env(name, value, fn):
    os.environ[name] = value
    try:
        return fn()
    finally:
        del os.environ[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 4, 2, 1])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decrypt_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B, delta = 1 << log_n, args.batch, 2.0 ** 50
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    lib = fc.load()
    os.environ.pop("FHECORE_DECRYPT_UNFUSED", None)
    sk = ctx.keygen_secret(seed=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(43)
    ws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, B))
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for level in args.levels:
        pt = torch.empty(B, level, n, dtype=torch.int64, device="cuda")
        for ls in (log_n - 1, 10):
            z = torch.view_as_complex(torch.rand(B, 1 << ls, 2, generator=gen, device="cuda",
                                                 dtype=torch.float64) * 2 - 1)
            ct = ctx.encrypt_slots(z, delta, sk, secret=True, level=level, log_slots=ls, seed=SEED)
            out = torch.empty(B, 1 << ls, dtype=torch.complex128, device="cuda")
            ref = torch.empty_like(out)

            def new():
                ctx.decrypt_slots(ct, sk, delta, log_slots=ls, workspace=ws, out=out)

            def composed():
                # fhe_decrypt into a plaintext kept across calls, as a careful caller would
                check(lib.fhe_decrypt(ctx.handle, ctypes.c_void_p(pt.data_ptr()),
                                      ctypes.c_void_p(ct.data_ptr()),
                                      ctypes.c_void_p(sk.data_ptr()), B, level, None), "fhe_decrypt")
                ctx.decode(pt, delta, level=level, log_slots=ls, workspace=ws, out=ref)

            new()
            composed()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), ref.view(torch.int64)), \
                f"level {level} log_slots {ls}: decrypt_slots differs from decode(decrypt)"
            unfused_out = torch.empty_like(out)

            def unfused():
                ctx.decrypt_slots(ct, sk, delta, log_slots=ls, workspace=ws, out=unfused_out)

            a, m, b = [], [], []
            for _ in range(args.rounds):
                a.append(timed_ms(new, args.steps, args.warmup))
                m.append(timed_ms(composed, args.steps, args.warmup))
                b.append(timed_ms(new, args.steps, args.warmup))
            ma, mb, mc = (statistics.median(v) for v in (a, b, m))
            mn = statistics.median(a + b)
            spread = abs(ma - mb)
            unfused_ms = with_env("FHECORE_DECRYPT_UNFUSED", "1",
                                  lambda: timed_ms(unfused, args.steps, args.warmup))
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), unfused_out.view(torch.int64)), \
                f"level {level} log_slots {ls}: the unfused form differs"
            nl = min(level, 2)
            rec = {"op": "decrypt_slots", "level": level, "log_slots": ls, "batch": B,
                   "log_n": log_n, "new_ms": round(mn, 4), "new_before_ms": round(ma, 4),
                   "new_after_ms": round(mb, 4), "spread_ms": round(spread, 4),
                   "new_min_max_ms": [round(min(a + b), 4), round(max(a + b), 4)],
                   "composed_ms": round(mc, 4),
                   "composed_min_max_ms": [round(min(m), 4), round(max(m), 4)],
                   "composed_over_new": round(mc / mn, 3),
                   "slower_beyond_spread": bool(mn - mc > spread),
                   "unfused_ms": round(unfused_ms, 4),
                   "decrypt_step_bytes": {"composed": 4 * level * B * n * 8,
                                          "fused_first_pass": 4 * nl * B * n * 8},
                   "marks_ms": marks_of(new), "composed_marks_ms": marks_of(composed)}
            emit(rec)
            del ct, out, ref, unfused_out, z
        del pt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
