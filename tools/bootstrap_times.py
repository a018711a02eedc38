"""Times a full-packing CKKS bootstrap (fhecore.bootstrap.Bootstrapper) at N = 2^16 on a chain long
enough for its default parameters -- L = 24 (q_0 of 55 bits, the rest the 50-bit chain), 6 special
primes, dnum = 4; K = 16, degree 31, 3 double angles, 3 + 3 factors: 3 + 9 + 3 levels, the result
at level 9 -- under device keys with a secret of Hamming weight 28, in one process:

  * per phase (mod_raise, coeff_to_slot, split with its conjugation, eval_mod on the batch of 2,
    merge, slot_to_coeff): device events between the phases of `--steps` bootstraps after
    `--warmup`, the median per phase, and the slot error of the last result;
  * conj_split / conj_merge against their composed forms at the level and batch the bootstrap runs
    them at and at batch 32: split = lincomb (ct + cc), lincomb (ct - cc), mul_plain by the
    plaintext of -+w; merge = mul_plain by +-w, lincomb.  The composed result is checked against
    the fused one first; the two are timed back to back, `--rounds` times alternating, and the
    median and the ratio are reported as measured.

With `--log-slots A B ..` the sparse bootstraps at 2^A, 2^B .. slots (BootstrapParams.log_slots)
run interleaved with the full-packing one, iteration by iteration, in the same process, under the
same secret; one record each, with the phase `subsum` and the slot error, and the split / merge
comparison is left out.

One JSON line per record.

  python tools/bootstrap_times.py [--steps 5] [--warmup 2] [--log-slots 10 12] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-fhe_amd"))
import fhecore as fc  # noqa: E402
from fhecore import bootstrap as bs  # noqa: E402
from fhecore.polyeval import Ct  # noqa: E402

PHASES = ("mod_raise", "subsum", "coeff_to_slot", "split", "eval_mod", "merge", "slot_to_coeff")


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


def x_half_plaintexts(ctx):
    """[L, N] NTT-form plaintexts of X^(N/2) and of -X^(N/2): w_j = psi_j^(N/2) on the first half
    of a row, q_j - w_j on the second (and the other way round)."""
    n, rows = ctx.n, []
    for q, psi in zip(ctx.moduli, ctx.psi):
        w = pow(psi, n // 2, q)
        rows.append(np.array([w] * (n // 2) + [q - w] * (n // 2), dtype=np.uint64))
    plus = np.stack(rows)
    minus = (np.array(ctx.moduli, dtype=np.uint64)[:, None] - plus)
    return fc.to_device(plus), fc.to_device(minus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--L", type=int, default=24)
    ap.add_argument("--K", type=int, default=6, help="special primes")
    ap.add_argument("--dnum", type=int, default=4)
    ap.add_argument("--log-slots", type=int, nargs="*", default=None,
                    help="also run the sparse bootstraps at these slot counts, interleaved")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bootstrap_times: needs a HIP device")
    log_n, L, K, dnum = args.log_n, args.L, args.K, args.dnum
    n = 1 << log_n
    delta = 2.0 ** 50
    rest = fc.gen_moduli(log_n, L - 1 + K, bits=50)
    ctx = fc.Context(log_n, moduli=fc.gen_moduli(log_n, 1, bits=55) + rest[:L - 1],
                     special=rest[L - 1:], dnum=dnum)
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    # ---- the bootstrap, phase by phase: full packing, then every --log-slots, interleaved
    hw = bs.BootstrapParams().hamming_weight
    sk = ctx.keygen_secret(seed=1, hamming_weight=hw)
    g = np.random.default_rng(2)
    runs = []
    for ls in [None] + list(args.log_slots or []):
        params = bs.BootstrapParams(log_slots=ls)
        be = bs.GpuBackend(ctx, sk=sk, seed=100)
        boot = bs.Bootstrapper(be, params)
        ns = n // 2 if ls is None else 1 << ls
        z = g.uniform(-1, 1, ns) + 1j * g.uniform(-1, 1, ns)
        ct = ctx.encrypt_slots(z, delta, sk, secret=True, level=1, log_slots=ls, seed=3)
        runs.append(dict(ls=ls, params=params, be=be, boot=boot, z=z, ct=ct, out=None,
                         times={p: [] for p in PHASES}))
    for it in range(args.warmup + args.steps):
        for r in runs:
            ev, names = [torch.cuda.Event(enable_timing=True)], []
            ev[0].record()

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append(e)
                names.append(name)

            r["out"] = r["boot"].bootstrap(Ct(r["ct"], 1, delta), mark=mark)
            torch.cuda.synchronize()
            if it >= args.warmup:
                for p, a, b in zip(names, ev, ev[1:]):
                    r["times"][p].append(a.elapsed_time(b))
    full_total = None
    for r in runs:
        params, out, ls = r["params"], r["out"], r["ls"]
        got = ctx.decode(ctx.decrypt(out.data, sk), float(out.scale), log_slots=ls).cpu().numpy()
        med = {p: statistics.median(v) for p, v in r["times"].items() if v}
        total = sum(med.values())
        full_total = total if ls is None else full_total
        rec = {"op": "bootstrap", "log_n": log_n, "L": L, "special": K, "dnum": dnum,
               "K": params.K, "degree": params.degree, "double_angles": params.double_angles,
               "cts_groups": params.cts_groups, "stc_groups": params.stc_groups,
               "hamming_weight": params.hamming_weight, "q0_bits": ctx.moduli[0].bit_length(),
               "out_level": out.level, "rotation_keys": len(r["be"].rot_keys),
               "phase_ms": {p: round(v, 3) for p, v in med.items()},
               "total_ms": round(total, 3),
               "max_slot_error": float(np.abs(got - r["z"]).max())}
        if ls is not None:
            rec.update(log_slots=ls, total_over_full_packing=round(total / full_total, 3))
        emit(rec)
    params = runs[0]["params"]
    del runs
    torch.cuda.empty_cache()
    if args.log_slots:
        return

    # ---- split / merge against their composed forms
    level = L - params.cts_groups
    plus, minus = x_half_plaintexts(ctx)
    tab_add = ctx.encode_scalars([1, 1], exact=True)
    tab_sub = ctx.encode_scalars([1, -1], exact=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for batch in (2, 32):
        qcol = torch.tensor(ctx.moduli[:level], dtype=torch.int64, device="cuda")[:, None]
        a, b = (torch.remainder(torch.randint(0, 2 ** 62, (batch, 2, level, n), generator=gen,
                                              device="cuda", dtype=torch.int64), qcol)
                for _ in range(2))
        re, im, t, o = (torch.empty_like(a) for _ in range(4))

        def split():
            ctx.conj_split(a, b, out=(re, im))

        def split_composed():
            ctx.lincomb([a, b], tab_add, out=re)
            ctx.lincomb([a, b], tab_sub, out=t)
            ctx.mul_plain(t, minus, out=im)

        def merge():
            ctx.conj_merge(a, b, out=o)

        def merge_composed():
            ctx.mul_plain(b, plus, out=t)
            ctx.lincomb([a, t], tab_add, out=o)

        for fused, composed, outs in ((split, split_composed, (re, im)),
                                      (merge, merge_composed, (o,))):
            fused()
            want = [x.clone() for x in outs]
            composed()
            torch.cuda.synchronize()
            assert all(torch.equal(x, w) for x, w in zip(outs, want)), \
                f"{fused.__name__}: the composed form differs"
            f, c = [], []
            for _ in range(args.rounds):
                f.append(timed_ms(fused, 20, 5))
                c.append(timed_ms(composed, 20, 5))
            f, c = statistics.median(f), statistics.median(c)
            passes = 4 if fused is split else 3  # words moved per element by the fused call
            nbytes = 8 * passes * batch * 2 * level * n
            emit({"op": "conj_" + fused.__name__, "log_n": log_n, "level": level, "batch": batch,
                  "fused_ms": round(f, 4), "composed_ms": round(c, 4),
                  "composed_over_fused": round(c / f, 3),
                  "fused_algorithmic_bytes": nbytes, "fused_GBps": round(nbytes / f / 1e6, 1)})
        del a, b, re, im, t, o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
