#!/usr/bin/env python3
"""msm_scalars_scan, msm_scalars_inverse and msm_scalars_div_linear timed (profiles/scalars_scan_time.txt) over n resident scalars,
beside yardsticks from existing code in the same run: a device-to-device copy of the vector, msm_scalars_mul, msm_scalars_powers,
and msm_device_download + msm_device_upload of one vector (what the step costs a prover that takes it to the host instead).

What each form is judged against (the last columns are the ratios; below 1 meets it, the sum scan up to 1.5 from 2^24 on):
    sum scan      mul              it moves the 96 bytes an element that mul moves, in a few small launches more
    product scan  powers           about half of powers' multiplications at 2^26
    div_linear    powers + mul     the least any route through existing calls would need for the remainder alone
    inverse       download+upload  otherwise the host is the better place for it

Per curve and size: the vectors resident before the timing, every form warmed up, forms alternating inside each repeat; each figure
is the wall time of the call (launches, kernels, synchronisation), the median of the repeats with the [min, max] spread.
--tile-logs times the sum scan at other tile sizes as well (msm_test_set_scan_tile_log).
    python3 tools/bench_scans.py [--reps 7] [--curves bls377,bn254] [--sizes 16,20,24,26] [--tile-logs 8,9] [--out profiles/scalars_scan_time.txt]
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
U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed evaluation point, reduced per curve
HIP_MEMCPY_D2D = 3


def med(xs):
    return statistics.median(xs)


def fmt(xs):
    return f"{med(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="bls377,bn254")
    ap.add_argument("--sizes", default="16,20,24,26", help="log2 n, comma separated")
    ap.add_argument("--tile-logs", default="", help="further tile sizes to time the sum scan at")
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
    emit(f"# scans over n resident 32-byte scalars; wall ms of a call: median [min, max] of {a.reps} repeats, forms alternating")
    emit("# columns: curve, log2 n, tiles per level | sum scan | product scan | inverse | div_linear | device-to-device copy | "
         "msm_scalars_mul | msm_scalars_powers | download + upload of the vector | sum / mul | product / powers | "
         "div_linear / (powers + mul) | inverse / (download + upload)" + ("".join(f" | sum scan at tile_log {t}" for t in extra)))
    for cname in a.curves.split(","):
        cid, q = CURVES[cname]
        z = U % q
        for size in a.sizes.split(","):
            logn = int(size)
            n = 1 << logn
            ctx = MsmContext(cid)
            va, vb, vd = (ctx.device_alloc(32 * n) for _ in range(3))
            ctx.generate_scalars(n, seed=11, into=va)
            ctx.generate_scalars(n, seed=12, into=vb)
            host = (ctypes.c_uint8 * (32 * n))()
            plan = (ctypes.c_int32 * 8)()
            vp = ctypes.c_void_p

            def copy():
                assert hip.hipMemcpy(vd, va, 32 * n, HIP_MEMCPY_D2D) == 0
                assert hip.hipDeviceSynchronize() == 0

            def round_trip():
                assert lib.msm_device_download(ctx._h, host, vp(va), 32 * n) == 0
                assert lib.msm_device_upload(ctx._h, vp(vd), host, 32 * n) == 0

            forms = {
                "sum": lambda: ctx.scalars_scan(vd, va, n, "sum"),
                "product": lambda: ctx.scalars_scan(vd, va, n, "product", exclusive=True),
                "inverse": lambda: ctx.scalars_inverse(vd, va, n),
                "div": lambda: ctx.scalars_div_linear(vd, va, n, z),
                "copy": copy,
                "mul": lambda: ctx.scalars_mul(vd, va, vb, n),
                "powers": lambda: ctx.scalars_powers(vd, z, n),
                "round_trip": round_trip,
            }
            for f in forms.values():
                f()
            forms["sum"]()
            levels = lib.msm_test_last_scan_plan(ctx._h, plan, 8)
            tiles = "+".join(str(t) for t in plan[:levels])
            ms = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            m = {k: med(v) for k, v in ms.items()}
            tail = ""
            for t in extra:
                assert lib.msm_test_set_scan_tile_log(ctx._h, t) == 0
                forms["sum"]()
                xs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    forms["sum"]()
                    xs.append((time.perf_counter() - t0) * 1e3)
                tail += f" | {fmt(xs)}"
            emit(f"{cname:6s} 2^{logn} ({tiles}) | " + " | ".join(fmt(ms[k]) for k in forms)
                 + f" | {m['sum'] / m['mul']:5.2f}x | {m['product'] / m['powers']:5.2f}x | {m['div'] / (m['powers'] + m['mul']):5.2f}x"
                 + f" | {m['inverse'] / m['round_trip']:5.2f}x" + tail)
            ctx.close()


if __name__ == "__main__":
    main()
