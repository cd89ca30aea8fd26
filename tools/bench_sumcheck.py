#!/usr/bin/env python3
"""The resident sumcheck operators timed (profiles/sumcheck_time.txt): msm_scalars_sumcheck_round (PROD m = 2, PROD m = 4, R1CS),
msm_scalars_bind (one table, top variable, in place) and msm_scalars_eq over tables of n = 2^log2n scalars of 32 bytes, each
beside a yardstick from the same run:
    round PROD m = 2        msm_scalars_inner over the same two vectors (the same bytes read, 1 multiplication per element
                            against 1.5)
    round PROD m = 4, R1CS  the two msm_scalars_mul calls that read the same four vectors
    bind                    the in-place fold msm_scalars_lincomb(dst = a = v, x = 1 - r, b = v + 32 h, y = r) it replaces (the same
                            bytes, two multiplications per output against one)
    eq                      msm_scalars_mul (one multiplication and one store per element, but two loads) and msm_scalars_powers
                            (ceil(log2 n) / 2 multiplications per element) at the same n

Per curve and n: five vectors of generated scalars resident before the timing, every form warmed up, forms alternating inside
each repeat; each figure is the wall time of the call (launch, kernels, synchronisation) as the median of the repeats with the
[min, max] spread.  No ratio is fixed in advance: whatever comes out is what the file says.
    python3 tools/bench_sumcheck.py [--reps 7] [--curves bls377] [--logn 16,20,24,26] [--out profiles/sumcheck_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from montgomery_amd import _lib, api  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

CURVES = {"bls377": (_lib.CURVE_BLS12_377_G1, api.BLS12_377_PARAMS.order), "pallas": (_lib.CURVE_PALLAS, api.PALLAS_PARAMS.order),
          "bn254": (_lib.CURVE_BN254_G1, api.BN254_PARAMS.order), "ed377": (_lib.CURVE_ED_ON_BLS12_377, api.ED_ON_BLS12_377_PARAMS.order),
          "bls381": (_lib.CURVE_BLS12_381_G1, api.BLS12_381_PARAMS.order), "grumpkin": (_lib.CURVE_GRUMPKIN, api.GRUMPKIN_PARAMS.order),
          "vesta": (_lib.CURVE_VESTA, api.VESTA_PARAMS.order)}
U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed challenge, reduced per curve


def med(xs):
    return statistics.median(xs)


def fmt(xs):
    return f"{med(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="bls377")
    ap.add_argument("--logn", default="16,20,24,26")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    _lib.load()
    emit(f"# the resident sumcheck over tables of n = 2^log2n 32-byte scalars; wall ms of a call: median [min, max] of {a.reps} repeats, "
         "forms alternating; ratio = operator / yardstick of the same run")
    emit("# rows: operator | its time | yardstick | its time | ratio")
    for cname in a.curves.split(","):
        cid, q = CURVES[cname]
        r = U % q
        for logn in [int(x) for x in a.logn.split(",")]:
            n, h = 1 << logn, 1 << (logn - 1)
            ctx = MsmContext(cid)
            va, vb, vc, ve, vd = (ctx.device_alloc(32 * n) for _ in range(5))
            for seed, v in enumerate((va, vb, vc, ve)):
                ctx.generate_scalars(n, seed=21 + seed, into=v)
            point = [(U * (j + 3)) % q for j in range(logn)]
            top = logn - 1
            forms = {
                "round2": lambda: ctx.scalars_sumcheck_round([va, vb], logn, top),
                "inner": lambda: ctx.scalars_inner(va, vb, n),
                "round4": lambda: ctx.scalars_sumcheck_round([va, vb, vc, ve], logn, top),
                "r1cs": lambda: ctx.scalars_sumcheck_round([va, vb, vc, ve], logn, top, "r1cs"),
                "mul_ab": lambda: ctx.scalars_mul(vd, va, vb, n),
                "mul_ce": lambda: ctx.scalars_mul(vd, vc, ve, n),
                "bind": lambda: ctx.scalars_bind(ve, ve, logn, top, r),
                "fold": lambda: ctx.scalars_lincomb(ve, (1 - r) % q, ve, r, ve + 32 * h, h),
                "eq": lambda: ctx.scalars_eq(vd, point),
                "powers": lambda: ctx.scalars_powers(vd, r, n),
            }
            for f in forms.values():
                f()
            ms = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            two_muls = [x + y for x, y in zip(ms["mul_ab"], ms["mul_ce"])]

            def row(name, xs, yard, ys):
                emit(f"{cname:6s} 2^{logn} | {name:28s} | {fmt(xs)} | {yard:34s} | {fmt(ys)} | {med(xs) / max(med(ys), 1e-9):5.2f}x")

            row("round PROD m=2", ms["round2"], "inner(a, b)", ms["inner"])
            row("round PROD m=4", ms["round4"], "mul(a, b) + mul(c, e)", two_muls)
            row("round R1CS", ms["r1cs"], "mul(a, b) + mul(c, e)", two_muls)
            row("bind m=1, top, in place", ms["bind"], "lincomb fold (1-r) lo + r hi", ms["fold"])
            row("eq", ms["eq"], "mul(a, b)", ms["mul_ab"])
            row("eq", ms["eq"], "powers", ms["powers"])
            ctx.close()


if __name__ == "__main__":
    main()
