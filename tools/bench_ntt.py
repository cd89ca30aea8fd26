#!/usr/bin/env python3
"""msm_scalars_ntt timed (profiles/scalars_ntt_time.txt): the forward transform, the inverse and the coset forward over B vectors
of n = 2^log2n resident scalars, beside msm_scalars_powers and a device-to-device copy of the same B n elements in the same run.

The yardstick is existing code: T_powers(n) + P T_copy(n), P the passes of the plan -- powers does log2(n) / 2 multiplications an
element on average, as the butterflies of a radix-2 transform do, and every pass moves the vector once in and once out, as the
copy does.  The last column is forward / yardstick.

Per curve and size: the vectors resident before the timing, every form warmed up (the twiddle cache is warm, as in a prover that
transforms column after column), forms alternating inside each repeat; each figure is the wall time of the call (launches, kernels,
synchronisation), the median of the repeats with the [min, max] spread.  --tile-logs times the forward transform at other stage
counts per pass as well (msm_test_set_ntt_tile_log), the measurement behind the default.
    python3 tools/bench_ntt.py [--reps 7] [--curves bls377,bn254] [--sizes 16x1,16x16,20x1,24x1,26x1] [--tile-logs 7,9,10]
                               [--out profiles/scalars_ntt_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from montgomery_amd import _lib, api  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

CURVES = {"bls377": (_lib.CURVE_BLS12_377_G1, api.BLS12_377_PARAMS.order), "pallas": (_lib.CURVE_PALLAS, api.PALLAS_PARAMS.order),
          "bn254": (_lib.CURVE_BN254_G1, api.BN254_PARAMS.order), "bls381": (_lib.CURVE_BLS12_381_G1, api.BLS12_381_PARAMS.order),
          "vesta": (_lib.CURVE_VESTA, api.VESTA_PARAMS.order)}
U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed coset shift / evaluation point, reduced per curve
HIP_MEMCPY_D2D = 3


def med(xs):
    return statistics.median(xs)


def fmt(xs):
    return f"{med(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="bls377,bn254")
    ap.add_argument("--sizes", default="16x1,16x16,20x1,24x1,26x1", help="log2n x B, comma separated")
    ap.add_argument("--tile-logs", default="", help="further stage counts per pass to time the forward transform at")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so.7")   # by its SONAME: the runtime the library has mapped; the baseline copy goes through it directly
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    extra = [int(x) for x in a.tile_logs.split(",") if x]
    emit(f"# msm_scalars_ntt over B vectors of n resident 32-byte scalars; wall ms of a call: median [min, max] of {a.reps} repeats, "
         "forms alternating, twiddle cache warm")
    emit("# columns: curve, log2 n x B, passes (stages) | forward | inverse | coset forward | msm_scalars_powers over B n | "
         "device-to-device copy of B n x 32 bytes | yardstick = powers + passes x copy | forward / yardstick"
         + ("".join(f" | forward at tile_log {t}" for t in extra)))
    for cname in a.curves.split(","):
        cid, q = CURVES[cname]
        shift = U % q
        for size in a.sizes.split(","):
            logn, B = (int(x) for x in size.split("x"))
            total = B << logn
            ctx = MsmContext(cid)
            va, vd = (ctx.device_alloc(32 * total) for _ in range(2))
            ctx.generate_scalars(total, seed=11, into=va)
            plan = (ctypes.c_int32 * 32)()

            def copy():
                assert hip.hipMemcpy(vd, va, 32 * total, HIP_MEMCPY_D2D) == 0
                assert hip.hipDeviceSynchronize() == 0

            forms = {
                "forward": lambda: ctx.scalars_ntt(vd, va, logn, batch=B),
                "inverse": lambda: ctx.scalars_ntt(vd, va, logn, inverse=True, batch=B),
                "coset": lambda: ctx.scalars_ntt(vd, va, logn, shift=shift, batch=B),
                "powers": lambda: ctx.scalars_powers(vd, shift, total),
                "copy": copy,
            }
            for f in forms.values():
                f()
            forms["forward"]()
            passes = lib.msm_test_last_ntt_plan(ctx._h, plan, 32)
            stages = "+".join(str(s) for s in plan[:passes])
            ms = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            yard = med(ms["powers"]) + passes * med(ms["copy"])
            tail = ""
            for t in extra:
                assert lib.msm_test_set_ntt_tile_log(ctx._h, t) == 0
                forms["forward"]()
                xs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    forms["forward"]()
                    xs.append((time.perf_counter() - t0) * 1e3)
                tail += f" | {fmt(xs)}"
            emit(f"{cname:6s} 2^{logn} x {B:<2d} {passes} ({stages}) | " + " | ".join(fmt(ms[k]) for k in forms)
                 + f" | {yard:9.3f} | {med(ms['forward']) / yard:5.2f}x" + tail)
            ctx.close()


if __name__ == "__main__":
    main()
