#!/usr/bin/env python3
"""Point ingest timing (msm_set_points_ex / msm_validate_points): uncompressed msm_set_points against compressed loads at each
validation level, and the subgroup check alone, with the field multiplications per point the kernels do (from the constants).

usage: python tools/points_ingest_time.py [--curves bls377,bls381] [--logn 20,24,26] [--reps 3] [--out FILE]
The inputs are 2^20 generated points (msm_generate_points), read back in both formats and tiled up to 2^logn: every point is
valid, so every run takes the path of an accepted load.  Times are wall clock around one C call (host bytes: the upload is
included), best of --reps, after one warm-up call.  The table goes to stdout (and to --out); profiles/points_ingest_time.txt
holds it."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from montgomery_amd import _lib  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

FIELDS = {   # p, q, b of y^2 = x^3 + b
    "bls377": (0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001,
               0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001, _lib.CURVE_BLS12_377_G1),
    "bls381": (0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
               0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001, _lib.CURVE_BLS12_381_G1),
}


def mults_per_point(p, q):
    """(decompression, subgroup check) field multiplications + squarings per point, as the kernels of points_ingest.h do them."""
    S, t = 0, p - 1
    while t % 2 == 0:
        S, t = S + 1, t // 2
    e = (p + 1) // 4 if S == 1 else (t - 1) // 2
    sqrt = e.bit_length() + bin(e).count("1")                 # fe_pow_sqrt_e (one square and one product per set bit)
    if S > 1:
        sqrt += 2 + sum(k - 1 for k in range(1, S)) + 3 * (S - 1)   # Tonelli-Shanks: x, b; the squarings; x z, z^2, b z per step
    dec = 1 + 2 + sqrt + 1 + 1 + 1                           # to Montgomery, x^3, sqrt, check, sign (to plain), beta x
    sub = 3 + q.bit_length() * 10 + bin(q).count("1") * 11   # curve equation, proj_double 10M, proj_add_mixed 11M
    return dec, sub


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bls377,bls381")
    ap.add_argument("--logn", default="20,24,26")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    base_n = 1 << 20
    lines = ["points_ingest_time: wall ms of one call, best of %d (host input: upload included)" % args.reps,
             "%-7s %5s %10s %10s %10s %10s %10s %8s %8s" % ("curve", "logn", "set_pts", "cmp_none", "cmp_curve", "cmp_subgr",
                                                          "val_subgr", "M_dec", "M_sub")]
    for curve in args.curves.split(","):
        p, q, cid = FIELDS[curve]
        dec_m, sub_m = mults_per_point(p, q)
        ctx = MsmContext(cid)
        lib = ctx._lib
        ctx.generate_points(base_n, seed=11)
        raw1, cmp1 = ctx.get_points(0, base_n), ctx.get_points(0, base_n, compressed=True)
        for logn in [int(x) for x in args.logn.split(",")]:
            n = 1 << logn
            reps = n // base_n
            raw, cmp_ = (C.c_uint8 * (len(raw1) * reps))(), (C.c_uint8 * (len(cmp1) * reps))()
            for r in range(reps):   # (tiled in place: no second host copy of 6.4 GB)
                C.memmove(C.addressof(raw) + r * len(raw1), raw1, len(raw1))
                C.memmove(C.addressof(cmp_) + r * len(cmp1), cmp1, len(cmp1))
            bad = C.c_uint64()

            def call(rc):
                if rc != _lib.MSM_OK:
                    raise RuntimeError(lib.msm_last_error(ctx._h).decode())

            t_set = best(lambda: call(lib.msm_set_points(ctx._h, raw, n, 0, 0)), args.reps)
            t = {}
            for name, lvl in (("none", _lib.VALIDATE_NONE), ("curve", _lib.VALIDATE_CURVE), ("subgroup", _lib.VALIDATE_SUBGROUP)):
                t[name] = best(lambda: call(lib.msm_set_points_ex(ctx._h, cmp_, n, 0, _lib.POINTS_COMPRESSED, lvl, C.byref(bad))),
                               args.reps)
            t_val = best(lambda: call(lib.msm_validate_points(ctx._h, 0, n, _lib.VALIDATE_SUBGROUP, C.byref(bad))), args.reps)
            lines.append("%-7s %5d %10.1f %10.1f %10.1f %10.1f %10.1f %8d %8d" % (
                curve, logn, 1e3 * t_set, 1e3 * t["none"], 1e3 * t["curve"], 1e3 * t["subgroup"], 1e3 * t_val, dec_m, sub_m))
            print(lines[-1], flush=True)
            del raw, cmp_
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
