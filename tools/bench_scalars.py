#!/usr/bin/env python3
"""The resident scalar-vector operations timed (profiles/scalars_vec_time.txt): msm_scalars_lincomb (two terms), msm_scalars_mul,
msm_scalars_inner and msm_scalars_powers over n scalars of 32 bytes, beside a device-to-device copy of one such vector (n x 32
bytes read and as many written) in the same run as the baseline.

Per curve and n: three vectors of generated scalars resident before the timing, every form warmed up, forms alternating inside
each repeat; each figure is the wall time of the call (launch, kernel, synchronisation) as the median of the repeats with the
[min, max] spread, and the memory traffic the form needs -- lincomb and mul 96 bytes per element, inner and the copy 64, powers
32 -- divided by that time.  No ratio is fixed in advance: whatever comes out is what the file says.
    python3 tools/bench_scalars.py [--reps 9] [--curves bls377,bls381,bn254,ed377] [--logn 16,20,24,26]
                                   [--out profiles/scalars_vec_time.txt]
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
          "bn254": (_lib.CURVE_BN254_G1, api.BN254_PARAMS.order), "ed377": (_lib.CURVE_ED_ON_BLS12_377, api.ED_ON_BLS12_377_PARAMS.order),
          "bls381": (_lib.CURVE_BLS12_381_G1, api.BLS12_381_PARAMS.order), "grumpkin": (_lib.CURVE_GRUMPKIN, api.GRUMPKIN_PARAMS.order),
          "vesta": (_lib.CURVE_VESTA, api.VESTA_PARAMS.order)}
U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed challenge, reduced per curve
BYTES_PER_ELEMENT = {"lincomb": 96, "mul": 96, "inner": 64, "powers": 32, "copy": 64}
HIP_MEMCPY_D2D = 3


def fmt(xs, traffic):
    med = statistics.median(xs)
    return f"{med:9.3f} [{min(xs):.3f}, {max(xs):.3f}] {traffic / med / 1e6:7.1f} GB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--curves", default="bls377,bls381,bn254,ed377")
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
    hip = ctypes.CDLL("libamdhip64.so.7")   # by its SONAME: the runtime the library has mapped; the baseline copy goes through it directly
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    emit(f"# msm_scalars_* over n resident 32-byte scalars; wall ms of a call: median [min, max] of {a.reps} repeats, forms alternating; "
         "GB/s = the form's memory traffic / the median")
    emit("# columns: curve, log2 n | lincomb x a + y b (96 B/element) | mul (96) | inner (64) | powers (32) | "
         "device-to-device copy of n x 32 bytes (64) | lincomb / copy")
    for cname in a.curves.split(","):
        cid, q = CURVES[cname]
        u = U % q
        ui = pow(u, -1, q)
        for logn in [int(x) for x in a.logn.split(",")]:
            n = 1 << logn
            ctx = MsmContext(cid)
            va, vb, vd = (ctx.device_alloc(32 * n) for _ in range(3))
            ctx.generate_scalars(n, seed=11, into=va)
            ctx.generate_scalars(n, seed=12, into=vb)

            def copy():
                assert hip.hipMemcpy(vd, va, 32 * n, HIP_MEMCPY_D2D) == 0
                assert hip.hipDeviceSynchronize() == 0

            forms = {
                "lincomb": lambda: ctx.scalars_lincomb(vd, u, va, ui, vb, n),
                "mul": lambda: ctx.scalars_mul(vd, va, vb, n),
                "inner": lambda: ctx.scalars_inner(va, vb, n),
                "powers": lambda: ctx.scalars_powers(vd, u, n),
                "copy": copy,
            }
            for f in forms.values():
                f()
            ms = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            ratio = statistics.median(ms["lincomb"]) / max(statistics.median(ms["copy"]), 1e-9)
            emit(f"{cname:6s} 2^{logn} | " + " | ".join(fmt(ms[k], BYTES_PER_ELEMENT[k] * n) for k in forms) + f" | {ratio:5.2f}x")
            ctx.close()


if __name__ == "__main__":
    main()
