#!/usr/bin/env python3
"""msm_points_lincomb timed (profiles/points_lincomb_time.txt): the fold (1, u), the fold (u^-1, u) and the scaling (u, none).

Per curve and n: every form writes into a second point set from a resident source of n points -- the folds produce n / 2 rows
from its two halves, the scaling n rows -- so the source stays as it is and every repeat does the same work.  Beside them two
baselines from entry points that existed before: msm_validate_points(SUBGROUP) over as many points as the form produces rows (a
q-bit double-and-add per point without the endomorphism: the same kind of work; on the cofactor-1 curves it only checks the
curve equation and is printed for completeness) and one msm_run over the same number of points (what a fold sits between).
One process, inputs made and uploaded before the timing, every form warmed up, forms alternating inside each repeat; each figure
is the median of the repeats with the [min, max] spread.  Expectation, not a gate: on a curve with the endomorphism a one-scalar
fold has about half the doublings and a third of the additions of the subgroup check, and should be well under it.
    python3 tools/bench_points_lincomb.py [--reps 7] [--curves bls377,pallas,bn254,ed377] [--logn 16,20,24]
                                          [--out profiles/points_lincomb_time.txt]
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
U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed 253-bit challenge, reduced per curve


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="bls377,pallas,bn254,ed377")
    ap.add_argument("--logn", default="16,20,24")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# msm_points_lincomb from a resident set of n points into a second set; ms: median [min, max] of {a.reps} repeats, forms alternating")
    emit("# columns: curve, log2 n | fold (1, u): n/2 rows | fold (u^-1, u): n/2 rows | scale (u): n rows | validate SUBGROUP n/2 points | "
         "validate SUBGROUP n points | msm_run n/2 points | msm_run n points | fold (1, u) / validate(n/2)")
    for cname in a.curves.split(","):
        cid, q = CURVES[cname]
        u = U % q
        ui = pow(u, -1, q)
        for logn in [int(x) for x in a.logn.split(",")]:
            n = 1 << logn
            h = n // 2
            ctx = MsmContext(cid)
            ctx.generate_points(n, seed=7)
            src = 0
            dst = ctx.pointset_create()
            ctx.pointset_select(src)
            dev, _ = ctx.generate_scalars(n, seed=9)
            forms = {
                "fold1": lambda: ctx.points_lincomb(1, u, src_a=src, a_lo=0, src_b=src, b_lo=h, count=h, dst=dst),
                "foldinv": lambda: ctx.points_lincomb(ui, u, src_a=src, a_lo=0, src_b=src, b_lo=h, count=h, dst=dst),
                "scale": lambda: ctx.points_lincomb(u, src_a=src, a_lo=0, count=n, dst=dst),
                "val_h": lambda: ctx.validate_points(0, h, "subgroup"),
                "val_n": lambda: ctx.validate_points(0, n, "subgroup"),
                "msm_h": lambda: ctx.run_device(dev, h, no_tables=True),
                "msm_n": lambda: ctx.run_device(dev, n, no_tables=True),
            }
            for f in forms.values():   # warm-up: workspaces, the destination's rows
                f()
            ms = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    ms[k].append(timed(f)[0])
            ratio = statistics.median(ms["fold1"]) / max(statistics.median(ms["val_h"]), 1e-9)
            emit(f"{cname:6s} 2^{logn} | " + " | ".join(fmt(ms[k]) for k in forms) + f" | {ratio:5.2f}x")
            ctx.close()


if __name__ == "__main__":
    main()
