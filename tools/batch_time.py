#!/usr/bin/env python3
"""msm_run_batch against B sequential msm_run calls on the same context (profiles/batch_msm_time.txt).

For BLS12-377 and Ed-on-BLS12-377, n in {2^12, 2^14, 2^16, 2^18} and B in {1, 4, 16, 64}: ms per batched call and per MSM,
and B sequential msm_run calls on the plain path (no_tables) and on window tables (built by msm_precompute).  The forms
alternate inside every repeat, in one process, over device-resident scalars; each figure is the median of the repeats with
the [min, max] spread.  --csweep also times the batched call under explicit windows c = 10 .. 16.
    python3 tools/batch_time.py [--reps 7] [--csweep] [--curves bls377,ed377] [--logn 12,14,16,18] [--batch 1,4,16,64]
    python3 tools/batch_time.py --once 16 16      one batched 2^16 x 16 call after a warm-up (for rocprofv3 --kernel-trace)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from montgomery_amd import _lib  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

CURVES = {"bls377": _lib.CURVE_BLS12_377_G1, "ed377": _lib.CURVE_ED_ON_BLS12_377}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def once(logn, B):
    ctx = MsmContext(CURVES["bls377"])
    n = 1 << logn
    ctx.generate_points(n, seed=7)
    ptrs = [ctx.device_alloc(32 * n) for _ in range(B)]
    for b, p in enumerate(ptrs):
        ctx.generate_scalars(n, seed=100 + b, into=p)
    ctx.run_batch_device(ptrs, n)   # warm-up: workspaces
    ms, out = timed(lambda: ctx.run_batch_device(ptrs, n))
    info = out[0][1]
    print(f"batched 2^{logn} x {B}: {ms:.3f} ms wall, c = {info['c']}, K = {info['K']}, rounds = {info['rounds']}, "
          f"phase_ms = {info['phase_ms']}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--csweep", action="store_true")
    ap.add_argument("--curves", default="bls377,ed377")
    ap.add_argument("--logn", default="12,14,16,18")
    ap.add_argument("--batch", default="1,4,16,64")
    ap.add_argument("--once", nargs=2, type=int, metavar=("LOGN", "B"))
    a = ap.parse_args()
    if a.once:
        once(*a.once)
        return
    Bs = [int(x) for x in a.batch.split(",")]
    print("# msm_run_batch vs B sequential msm_run, device scalars; ms: median [min, max] of", a.reps, "repeats, forms alternating")
    print("# columns: curve, log2 n, B, c/K of the batch | batched ms per call | per MSM | sequential plain per MSM | "
          "sequential tables per MSM | best sequential / batched")
    for cname in a.curves.split(","):
        for logn in [int(x) for x in a.logn.split(",")]:
            n = 1 << logn
            ctx = MsmContext(CURVES[cname])
            ctx.generate_points(n, seed=7)
            ctx.precompute()
            ptrs = [ctx.device_alloc(32 * n) for _ in range(max(Bs))]
            for b, p in enumerate(ptrs):
                ctx.generate_scalars(n, seed=100 + b, into=p)
            for B in Bs:
                P = ptrs[:B]
                forms = {
                    "batch": lambda: ctx.run_batch_device(P, n),
                    "plain": lambda: [ctx.run_device(p, n, no_tables=True) for p in P],
                    "tables": lambda: [ctx.run_device(p, n) for p in P],
                }
                cs = list(range(10, 17)) if a.csweep else []
                for c in cs:
                    forms[f"c{c}"] = (lambda c=c: ctx.run_batch_device(P, n, c=c))
                for f in forms.values():   # warm-up: workspaces, tables
                    f()
                ms = {k: [] for k in forms}
                info = None
                for _ in range(a.reps):
                    for k, f in forms.items():
                        t, out = timed(f)
                        ms[k].append(t)
                        if k == "batch":
                            info = out[0][1]
                best_seq = min(statistics.median(ms["plain"]), statistics.median(ms["tables"]))
                per = lambda k: [x / B for x in ms[k]]  # noqa: E731
                print(f"{cname:6s} 2^{logn} B={B:3d} c={info['c']:2d}/K={info['K']:2d} | {fmt(ms['batch'])} | {fmt(per('batch'))} | "
                      f"{fmt(per('plain'))} | {fmt(per('tables'))} | {best_seq / statistics.median(ms['batch']):5.2f}x", flush=True)
                if cs:
                    print("        c sweep, batched ms per call: " + "  ".join(f"c{c} {statistics.median(ms[f'c{c}']):.3f}" for c in cs),
                          flush=True)
            for p in ptrs:
                ctx.device_free(p)
            ctx.close()


if __name__ == "__main__":
    main()
