#!/usr/bin/env python3
"""msm_points_ntt timed (profiles/points_ntt_time.txt).

Per curve and n = 2^log2n, from a resident set of n points into a second point set:
  forward   msm_points_ntt, the library's root, no shift
  inverse   the inverse transform (its pass over n^-1 included)
  inv coset the inverse on a coset (the pass is over n^-1 shift^-j)
and as yardsticks from entry points that existed before, in the same process:
  pmul      msm_points_mul over n / 2 rows: what one multiplying stage does, without the butterfly behind the walk
  copy      a device copy of n rows (msm_points_lincomb with the scalar 1), which is what the bit reversal moves
  add       msm_points_lincomb A[i] + A[i + n/2] over n / 2 rows: stage 1's stand-in (one addition and one inversion per lane,
            where a stage-1 butterfly does two additions and one inversion)
One process, inputs resident before the timing, every form warmed up, forms alternating inside each repeat; each figure is the
median of the repeats with the [min, max] spread.  Derived columns:
  stage / pmul   (forward - copy - add) / (log2n - 2) over pmul: one multiplying stage against msm_points_mul over n / 2 rows
  fwd / (L-1) pmul   the whole forward transform against log2n - 1 such calls: what the skipped twiddles buy

    python3 tools/bench_points_ntt.py [--reps 5] [--curves bls377,pallas,bn254] [--logn 14,16,20] [--out profiles/points_ntt_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHIFT = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed 253-bit scalar, reduced per curve
FORMS = ("forward", "inverse", "inv coset", "pmul", "copy", "add")


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def fmt(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def curves():
    from montgomery_amd import _lib, api

    return {"bls377": (_lib.CURVE_BLS12_377_G1, api.BLS12_377_PARAMS.order), "pallas": (_lib.CURVE_PALLAS, api.PALLAS_PARAMS.order),
            "bn254": (_lib.CURVE_BN254_G1, api.BN254_PARAMS.order), "bls381": (_lib.CURVE_BLS12_381_G1, api.BLS12_381_PARAMS.order),
            "vesta": (_lib.CURVE_VESTA, api.VESTA_PARAMS.order)}


def measure(cname, logn, reps):
    """{form: [ms, ...]} and the library's report of the forward transform's plan"""
    from montgomery_amd.api import MsmContext

    cid, q = curves()[cname]
    n = 1 << logn
    ctx = MsmContext(cid)
    ctx.generate_points(n, seed=7)
    src, dst = 0, ctx.pointset_create()
    ctx.pointset_select(src)
    dev, _ = ctx.generate_scalars(n, seed=9)
    shift = SHIFT % q

    def plan():
        out = (ctypes.c_int32 * 7)()
        ctx._lib.msm_test_last_points_ntt(ctx._h, out, 7)
        return list(out)

    calls = {
        "forward": lambda: ctx.points_ntt(src=src, log2n=logn, dst=dst),
        "inverse": lambda: ctx.points_ntt(src=src, log2n=logn, inverse=True, dst=dst),
        "inv coset": lambda: ctx.points_ntt(src=src, log2n=logn, inverse=True, shift=shift, dst=dst),
        "pmul": lambda: ctx.points_mul(dev, src=src, count=n // 2, dst=dst),
        "copy": lambda: ctx.points_lincomb(1, src_a=src, count=n, dst=dst),
        "add": lambda: ctx.points_lincomb(1, 1, src_a=src, src_b=src, b_lo=n // 2, count=n // 2, dst=dst),
    }
    info = None
    for k in FORMS:   # warm-up: the workspaces, the destination's rows, the twiddles
        calls[k]()
        if k == "forward":
            info = plan()
    ms = {k: [] for k in FORMS}
    for _ in range(reps):
        for k in FORMS:
            ms[k].append(timed(calls[k]))
    ctx.close()
    return ms, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curves", default="bls377,pallas,bn254")
    ap.add_argument("--logn", default="14,16,20")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# msm_points_ntt over n resident points into a second set; ms: median [min, max] of {a.reps} repeats, forms alternating in one process")
    emit("# columns: curve, log2 n | " + " | ".join(FORMS) + " | stage / pmul | fwd / (L-1) pmul | grid blocks, multiplications")
    for cname in a.curves.split(","):
        for logn in [int(x) for x in a.logn.split(",")]:
            ms, info = measure(cname, logn, a.reps)
            med = {k: statistics.median(v) for k, v in ms.items()}
            stage = (med["forward"] - med["copy"] - med["add"]) / (logn - 2)
            emit(f"{cname:6s} 2^{logn} | " + " | ".join(fmt(ms[k]) for k in FORMS) +
                 f" | {stage / med['pmul']:5.3f}x | {med['forward'] / ((logn - 1) * med['pmul']):5.3f}x | {info[2]}, {info[6]}")


if __name__ == "__main__":
    main()
