"""Times the device encoder / decoder (fhe_encode / fhe_decode) at the key-switch configuration
(N = 2^16, L = 16, K = 4, dnum = 4, count 32) in one process:

  encode  level L with the P rows (a [L + K][N] diagonal), and level 4 without them
  decode  level 2

each against
  * unfused:  the path of wide contexts forced on the same context (FHECORE_ENCODE_UNFUSED=1, read
              by every call): a separate lift into the output, then whole forward NTTs in place
              (encode only: decode has one form);
  * composed: the same result from torch and public calls -- torch.fft over the 2N-th roots,
              rounding, torch.remainder per limb and ctx.ntt (composed_encode), ctx.intt, a
              centring and torch.fft (composed_decode; it centres limb 0 alone, which is enough
              for the coefficients timed here and less work than fhe_decode's two limbs).  Equal
              to the device path within rounding, not bit for bit; timed only;
  * host:     fhecore.ckks.Encoder.encode -> to_rns -> to_device -> ctx.ntt, including the upload
              (encode only; wall clock around a synchronised call).

Device events around `--steps` calls after `--warmup` calls of the same shape; the device forms of
one case are timed back to back, `--rounds` times alternating, and the median is reported.  One
JSON line per case: ms per call of every form, the ratios, the call's algorithmic bytes --
count (8N + 8N rows) for encode, count (8N limbs read + 8N) for decode -- over its time as a
fraction of the 8 TB/s HBM peak, and the special FFT's share of the call from the library's own
per-launch events (fhe_prof_begin / fhe_prof_end).

With `--log-slots A B ..` the sparse calls are timed instead (fhe_encode_sparse /
fhe_decode_sparse at 2^A, 2^B .. slots): encode at level L with the P rows and decode at level 2,
each against today's only other route, fhe_encode of the vector tiled N / 2^(log_slots + 1) times
(fhe_decode of the whole plaintext).  Per round the tiled call is timed before and after the
sparse one; the record holds the median of either position, their difference (`tiled_spread_ms`:
what two medians of one call differ by in this run), the sparse median, and `within_spread`:
whether sparse - tiled <= that spread.  The tiled call is fhe_encode itself, so its time next to
the first record above is the full path's before and after.

  python tools/encode_times.py [--steps 50] [--warmup 20] [--log-slots 8 10 12 14] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-fhe_amd"))
import fhecore as fc  # noqa: E402
from fhecore import ckks  # noqa: E402
from fhecore._capi import check  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (MI355X spec)
UNFUSED = "FHECORE_ENCODE_UNFUSED"


def _pos(ctx):
    return torch.from_numpy(ckks.Encoder(ctx.n).pos).to("cuda")


def composed_encode(ctx, z, delta, level, special, pos):
    """ctx.encode(z, delta, level, special) from torch.fft, torch.remainder and ctx.ntt, for
    level == L when special (the rows are then the context's limbs in order)."""
    n = ctx.n
    a = torch.zeros(*z.shape[:-1], 2 * n, dtype=torch.complex128, device=z.device)
    a[..., pos] = z
    c = torch.round(torch.fft.fft(a)[..., :n].real * (2.0 / n) * delta).to(torch.int64)
    mods = ctx.all_moduli[:level + ctx.K] if special else ctx.moduli[:level]
    return ctx.ntt_(torch.stack([torch.remainder(c, q) for q in mods], dim=-2))


def composed_decode(ctx, pt, delta, pos):
    """Slots of plaintexts whose centred coefficients fit q_0: ctx.intt of limb 0, the centring,
    torch.fft."""
    n, q0 = ctx.n, ctx.moduli[0]
    x = ctx.intt(pt[..., :1, :].contiguous())[..., 0, :]
    c = torch.where(x > (q0 - 1) // 2, x - q0, x).to(torch.float64)
    b = torch.zeros(*c.shape[:-1], 2 * n, dtype=torch.complex128, device=pt.device)
    b[..., :n] = c
    return torch.fft.ifft(b)[..., pos] * (2 * n / delta)


def host_encode(ctx, z_host, delta, level, special):
    mods = ctx.all_moduli[:level + ctx.K] if special else ctx.moduli[:level]
    enc = ckks.Encoder(ctx.n)
    res = np.stack([ckks.to_rns(enc.encode(z, delta), mods) for z in z_host])
    return ctx.ntt_(fc.to_device(res))


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


def fft_share(fn, reps=10):
    """The share of fn's library launches spent in the marks named *_fft."""
    lib = fc.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap = 16 * reps + 16
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
    total = sum(per.values())
    fft = sum(v for k, v in per.items() if k.endswith("_fft"))
    return (fft / total if total else 0.0), {k: round(v, 4) for k, v in per.items()}


def sparse_cases(args, ctx, emit):
    """fhe_encode_sparse / fhe_decode_sparse against the tiled full calls, --log-slots each."""
    lib = fc.load()
    log_n, L, K, B = args.log_n, ctx.L, ctx.K, args.count
    n, delta = 1 << log_n, 2.0 ** 50
    gen = torch.Generator(device="cuda")
    gen.manual_seed(41)
    ews = ctx.workspace(lib.fhe_encode_workspace(ctx.handle, B))
    dws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, B))
    out = torch.empty(B, L + K, n, dtype=torch.int64, device="cuda")
    for ls in args.log_slots:
        ns, gap = 1 << ls, n // (2 << ls)
        z = torch.view_as_complex(torch.rand(B, ns, 2, generator=gen, device="cuda",
                                             dtype=torch.float64) * 2 - 1)
        zt = z.repeat(1, gap).contiguous()
        zo = torch.empty(B, ns, dtype=torch.complex128, device="cuda")
        zf = torch.empty(B, n // 2, dtype=torch.complex128, device="cuda")

        def enc_sparse():
            ctx.encode(z, delta, special=True, workspace=ews, out=out, log_slots=ls)

        def enc_tiled():
            ctx.encode(zt, delta, special=True, workspace=ews, out=out)

        def dec_sparse():
            ctx.decode(pt, delta, level=2, workspace=dws, out=zo, log_slots=ls)

        def dec_tiled():
            ctx.decode(pt, delta, level=2, workspace=dws, out=zf)

        enc_tiled()
        pt = out.clone()
        out.zero_()
        enc_sparse()
        torch.cuda.synchronize()
        assert torch.equal(out, pt), "the sparse encode differs from the tiled one"
        dec_sparse()
        dec_tiled()
        torch.cuda.synchronize()
        assert torch.equal(zo.view(torch.float64), zf[:, :ns].contiguous().view(torch.float64)), \
            "the sparse decode differs from the full one on an exactly sparse plaintext"
        for op, sparse, tiled in (("encode", enc_sparse, enc_tiled), ("decode", dec_sparse, dec_tiled)):
            a, m, b = [], [], []
            for _ in range(args.rounds):
                a.append(timed_ms(tiled, args.steps, args.warmup))
                m.append(timed_ms(sparse, args.steps, args.warmup))
                b.append(timed_ms(tiled, args.steps, args.warmup))
            ma, mm, mb = (statistics.median(v) for v in (a, m, b))
            mt = statistics.median(a + b)
            _, marks = fft_share(sparse)
            _, tmarks = fft_share(tiled)
            emit({"op": op + "_sparse", "log_slots": ls, "log_n": log_n, "count": B,
                  "level": L if op == "encode" else 2, "rows": L + K,
                  "sparse_ms": round(mm, 4), "tiled_ms": round(mt, 4),
                  "tiled_before_ms": round(ma, 4), "tiled_after_ms": round(mb, 4),
                  "tiled_spread_ms": round(abs(ma - mb), 4),
                  "sparse_over_tiled": round(mm / mt, 3),
                  "within_spread": bool(mm - mt <= abs(ma - mb)),
                  "marks_ms": marks, "tiled_marks_ms": tmarks})
        del pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--log-slots", type=int, nargs="*", default=None,
                    help="time the sparse calls at these slot counts instead")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encode_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, 16, 4, 4
    n, B = 1 << log_n, args.count
    delta = 2.0 ** 50
    ctx = fc.Context(log_n, L=L, K=K, dnum=dnum)
    lib = fc.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(37)
    z = torch.view_as_complex(torch.rand(B, n // 2, 2, generator=gen, device="cuda",
                                         dtype=torch.float64) * 2 - 1)
    z_host = z.cpu().numpy()
    pos = _pos(ctx)
    ews = ctx.workspace(lib.fhe_encode_workspace(ctx.handle, B))
    dws = ctx.workspace(lib.fhe_decode_workspace(ctx.handle, B))
    sink = open(args.out, "a") if args.out else None
    os.environ.pop(UNFUSED, None)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if args.log_slots:
        sparse_cases(args, ctx, emit)
        return

    for level, special in ((L, True), (4, False)):
        rows = level + (K if special else 0)
        out = torch.empty(B, rows, n, dtype=torch.int64, device="cuda")

        def fused():
            ctx.encode(z, delta, level=level, special=special, workspace=ews, out=out)

        def unfused():
            os.environ[UNFUSED] = "1"
            try:
                ctx.encode(z, delta, level=level, special=special, workspace=ews, out=out)
            finally:
                del os.environ[UNFUSED]

        def composed():
            composed_encode(ctx, z, delta, level, special, pos)

        fused()
        want = out.clone()
        out.zero_()
        unfused()
        torch.cuda.synchronize()
        assert torch.equal(out, want), "the unfused encode differs from the fused one"
        # composed: the same coefficients within rounding (limb 0, centred)
        q0 = ctx.moduli[0]
        d = torch.remainder(ctx.intt(want[:, :1].contiguous()) -
                            ctx.intt(composed_encode(ctx, z, delta, level, special, pos)[:, :1]
                                     .contiguous()), q0)
        d = torch.minimum(d, q0 - d).max().item()
        assert d <= 4, f"composed encode is {d} units away"
        del want
        f, u, c = [], [], []
        for _ in range(args.rounds):
            f.append(timed_ms(fused, args.steps, args.warmup))
            u.append(timed_ms(unfused, args.steps, args.warmup))
            c.append(timed_ms(composed, args.steps, args.warmup))
        f, u, c = (statistics.median(v) for v in (f, u, c))
        host = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_encode(ctx, z_host, delta, level, special)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        share, marks = fft_share(fused)
        nbytes = B * (8 * n + 8 * n * rows)
        emit({"op": "encode", "level": level, "special": int(special), "count": B, "log_n": log_n,
              "fused_ms": round(f, 4), "unfused_ms": round(u, 4), "composed_ms": round(c, 4),
              "host_ms": round(min(host), 1), "unfused_over_fused": round(u / f, 3),
              "composed_over_fused": round(c / f, 3), "host_over_fused": round(min(host) / f, 1),
              "composed_max_coeff_diff": int(d), "fused_algorithmic_bytes": nbytes,
              "fused_frac_hbm_peak": round(nbytes / (f * 1e-3) / HBM_PEAK, 4),
              "fft_share": round(share, 3), "marks_ms": marks})
        del out
        torch.cuda.empty_cache()

    # decode at level 2, from an [L + K][N] diagonal read in place
    level = 2
    pt = ctx.encode(z, delta, special=True)
    zo = torch.empty(B, n // 2, dtype=torch.complex128, device="cuda")

    def dec():
        ctx.decode(pt, delta, level=level, workspace=dws, out=zo)

    def dec_composed():
        composed_decode(ctx, pt, delta, pos)

    dec()
    err = (zo - z).abs().max().item()
    cerr = (composed_decode(ctx, pt, delta, pos) - z).abs().max().item()
    assert err < 1e-9 and cerr < 1e-9, (err, cerr)
    f, c = [], []
    for _ in range(args.rounds):
        f.append(timed_ms(dec, args.steps, args.warmup))
        c.append(timed_ms(dec_composed, args.steps, args.warmup))
    f, c = statistics.median(f), statistics.median(c)
    share, marks = fft_share(dec)
    nbytes = B * (8 * n * min(level, 2) + 8 * n)
    emit({"op": "decode", "level": level, "pt_rows": L + K, "count": B, "log_n": log_n,
          "device_ms": round(f, 4), "composed_ms": round(c, 4),
          "composed_over_device": round(c / f, 3), "round_trip_max_err": err,
          "composed_round_trip_max_err": cerr, "algorithmic_bytes": nbytes,
          "frac_hbm_peak": round(nbytes / (f * 1e-3) / HBM_PEAK, 4),
          "fft_share": round(share, 3), "marks_ms": marks})


if __name__ == "__main__":
    main()
