"""Times batched encryption (fhe_encrypt_level, fhe_encrypt_sk_level, fhe_encrypt_slots) at the
key-switch configuration (N = 2^16, L = 16, K = 4, dnum = 4, batch 32), at level L and at level 4,
each against what a caller wrote before them, in the same process:

  pk, sk     32 x fhe_encrypt / fhe_encrypt_sk of a top-level plaintext, one seed each
             (-> drop_level below the top)
  slots_pk,  32 x fhe_encode at the top level -> fhe_encrypt / fhe_encrypt_sk (-> drop_level)
  slots_sk

Element 0 of the new call equals the loop's first ciphertext (same seed) and is checked before
anything is timed.  Device events around `--steps` calls after `--warmup` calls; per round the new
call is timed before and after the loop, `--rounds` times.  One JSON line per case: the median ms
of either form, `spread_ms` (what the new call's two medians differ by in this run), the ratio,
`faster_beyond_spread` (loop - new > spread), the new call's algorithmic bytes (the ciphertexts
written, the plaintexts or slots and the live key rows read) over its time as a fraction of the
8 TB/s HBM peak, and the draw / transform / finish shares from the library's own per-launch events
(fhe_prof_begin / fhe_prof_end); `pass_batch` is the ciphertexts per pass the call takes by
default.  The public-key cases also record the new call with the batch cut
into passes (FHECORE_ENCRYPT_PASS) and on the unfused route (FHECORE_ENCRYPT_UNFUSED).

  python tools/encrypt_times.py [--steps 20] [--warmup 5] [--rounds 3] [--out FILE]"""
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
    return per


def with_env(name, value, fn):
    os.environ[name] = value
    try:
        return fn()
    finally:
        del os.environ[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encrypt_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B, delta = 1 << log_n, args.batch, 2.0 ** 50
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    lib = fc.load()
    for name in ("FHECORE_ENCRYPT_PASS", "FHECORE_ENCRYPT_UNFUSED"):
        os.environ.pop(name, None)
    sk = ctx.keygen_secret(seed=1)
    pk = ctx.keygen_public(sk, seed=2)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(43)
    z = torch.view_as_complex(torch.rand(B, n // 2, 2, generator=gen, device="cuda",
                                         dtype=torch.float64) * 2 - 1)
    pts = ctx.encode(z, delta)  # [B, L, N]
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for level in (L, 4):
        ws = ctx.workspace(lib.fhe_encrypt_workspace(ctx.handle, level, B))
        out = torch.empty(B, 2, level, n, dtype=torch.int64, device="cuda")
        for form in ("pk", "sk", "slots_pk", "slots_sk"):
            secret = form.endswith("sk")
            key = sk if secret else pk
            old = ctx.encrypt_sk if secret else ctx.encrypt

            if form.startswith("slots"):
                def new():
                    ctx.encrypt_slots(z, delta, key, secret=secret, level=level, seed=SEED,
                                      workspace=ws, out=out)

                def loop_one(i):
                    ct = old(ctx.encode(z[i], delta), key, SEED + i)
                    return ct if level == L else ctx.drop_level(ct, level)
                read = B * 8 * n
            else:
                def new():
                    (ctx.encrypt_sk if secret else ctx.encrypt)(pts, key, SEED, level=level,
                                                                workspace=ws, out=out)

                def loop_one(i):
                    ct = old(pts[i], key, SEED + i)
                    return ct if level == L else ctx.drop_level(ct, level)
                read = B * 8 * n * level

            def loop():
                for i in range(B):
                    loop_one(i)

            new()
            first = loop_one(0)
            torch.cuda.synchronize()
            assert torch.equal(out[0], first), f"{form} level {level}: element 0 differs from the loop's"
            del first
            a, m, b = [], [], []
            for _ in range(args.rounds):
                a.append(timed_ms(new, args.steps, args.warmup))
                m.append(timed_ms(loop, max(1, args.steps // 4), 1))
                b.append(timed_ms(new, args.steps, args.warmup))
            ma, mb, ml = (statistics.median(v) for v in (a, b, m))
            mn = statistics.median(a + b)
            spread = abs(ma - mb)
            marks = marks_of(new)
            total = sum(marks.values())
            share = {k: round(v / total, 3) for k, v in marks.items()} if total else {}
            nbytes = B * 2 * level * n * 8 + read + (1 if secret else 2) * level * n * 8
            rec = {"op": "encrypt", "form": form, "level": level, "batch": B, "log_n": log_n,
                   "pass_batch": ws.numel() // ((4 + level) * n),
                   "new_ms": round(mn, 4), "new_before_ms": round(ma, 4),
                   "new_after_ms": round(mb, 4), "spread_ms": round(spread, 4),
                   "loop_ms": round(ml, 4), "loop_over_new": round(ml / mn, 2),
                   "faster_beyond_spread": bool(ml - mn > spread),
                   "algorithmic_bytes": nbytes,
                   "frac_hbm_peak": round(nbytes / (mn * 1e-3) / HBM_PEAK, 4),
                   "shares": share, "marks_ms": {k: round(v, 4) for k, v in marks.items()}}
            if form == "pk":
                for p in (4, 8, 16):
                    rec[f"pass{p}_ms"] = round(with_env(
                        "FHECORE_ENCRYPT_PASS", str(p),
                        lambda: timed_ms(new, args.steps, args.warmup)), 4)
                rec["unfused_ms"] = round(with_env(
                    "FHECORE_ENCRYPT_UNFUSED", "1",
                    lambda: timed_ms(new, args.steps, args.warmup)), 4)
            emit(rec)
        del out, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
