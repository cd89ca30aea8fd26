#!/usr/bin/env python3
"""msm_run_narrow against msm_run over the same values widened to 32 bytes (profiles/narrow_scalar_time.txt).

Per curve, n and bits: the narrow call at the window pick_window_narrow gives, and the wide call on the plain path (no_tables)
and on window tables (msm_precompute; where they fit).  One process, device-resident scalars, every form warmed up, forms
alternating inside each repeat; each figure is the median of the repeats with the [min, max] spread.  Columns: ms, c / K,
the share of the narrow call's phase_ms in digits + sort, the ratio best wide / narrow, and beside it the ratio of digit entries
(Weierstrass: 2 N K_wide against N K_narrow; Edwards: N K_wide against N K_narrow).  --csweep also times the narrow call
under each candidate window (for every K the smallest c that reaches it).
    python3 tools/narrow_time.py [--reps 7] [--csweep [--cs 5,9,13,17]] [--curves bls377,ed377] [--logn 14,18,20,22,24,26] [--bits 1,8,16,32,64,128]
                                 [--out profiles/narrow_scalar_time.txt]
    python3 tools/narrow_time.py --once 22 64      one narrow 2^22 call of 64-bit scalars after a warm-up (for rocprofv3 --kernel-trace)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from montgomery_amd import _lib  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

CURVES = {"bls377": _lib.CURVE_BLS12_377_G1, "ed377": _lib.CURVE_ED_ON_BLS12_377, "bls381": _lib.CURVE_BLS12_381_G1,
          "pallas": _lib.CURVE_PALLAS}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def values(n, bits, seed):
    """n unsigned values below 2^bits as (n x width bytes, width, the same values as n x 32 bytes)."""
    rng = np.random.default_rng(seed)
    words = (bits + 63) // 64
    lim = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, words), dtype=np.uint64)
    top = bits - 64 * (words - 1)
    if top < 64:
        lim[:, -1] &= np.uint64((1 << top) - 1)
    wide = np.zeros((n, 4), dtype=np.uint64)
    wide[:, :words] = lim
    width = 1 if bits <= 8 else 2 if bits <= 16 else 4 if bits <= 32 else 8 if bits <= 64 else 16
    narrow = np.ascontiguousarray(wide.view(np.uint8).reshape(n, 32)[:, :width]).tobytes()
    return narrow, width, wide.tobytes()


def candidates(bits, n):
    """for every K = 1 .. 12 the smallest window that reaches it (windows below 9 bits only for scalars of up to 8 bits; above
    16 bits only from 2^21 points), and 17 bits for scalars of up to 32 bits: every window pick_window_narrow may return"""
    c_max, c_min = (22 if n >= (1 << 21) else 16), (2 if bits <= 8 else 9)
    cs = {-(-(bits + 1) // K) for K in range(1, 13) if c_min <= -(-(bits + 1) // K) <= c_max}
    if bits <= 32:
        cs.add(17)
    return sorted(cs)


def upload(ctx, raw):
    p = ctx.device_alloc(len(raw) + 16)
    ctx.device_upload(p, raw)
    return p


def once(logn, bits):
    ctx = MsmContext(CURVES["bls377"])
    n = 1 << logn
    ctx.generate_points(n, seed=7)
    narrow, width, _ = values(n, bits, 5)
    p = upload(ctx, narrow)
    ctx.run_narrow_device(p, n, width, bits)
    ms, (_, info) = timed(lambda: ctx.run_narrow_device(p, n, width, bits))
    print(f"narrow 2^{logn}, {bits} bits: {ms:.3f} ms wall, c = {info['c']}, K = {info['K']}, phase_ms = {info['phase_ms']}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--csweep", action="store_true")
    ap.add_argument("--curves", default="bls377,ed377")
    ap.add_argument("--logn", default="14,18,20,22,24,26")
    ap.add_argument("--bits", default="1,8,16,32,64,128")
    ap.add_argument("--cs", default="", help="explicit windows for --csweep instead of the candidates, e.g. 5,9,13,17")
    ap.add_argument("--out")
    ap.add_argument("--once", nargs=2, type=int, metavar=("LOGN", "BITS"))
    a = ap.parse_args()
    if a.once:
        once(*a.once)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# msm_run_narrow vs msm_run over the same values as 32-byte scalars, device scalars; ms: median [min, max] of {a.reps} "
         "repeats, forms alternating")
    emit("# columns: curve, log2 n, bits | narrow ms, c/K, digits+sort share of its phase_ms | wide plain ms, c/K | wide on tables ms | "
         "best wide / narrow | entry ratio | narrow median within the best wide form's max?")
    for cname in a.curves.split(","):
        te = cname == "ed377"
        for logn in [int(x) for x in a.logn.split(",")]:
            n = 1 << logn
            ctx = MsmContext(CURVES[cname])
            ctx.generate_points(n, seed=7)
            ctx.precompute()
            have_tables = ctx.tables_info()[1] > 0
            for bits in [int(x) for x in a.bits.split(",")]:
                narrow, width, wide = values(n, bits, 1000 + bits)
                pn, pw = upload(ctx, narrow), upload(ctx, wide)
                del narrow, wide
                forms = {
                    "narrow": lambda: ctx.run_narrow_device(pn, n, width, bits),
                    "plain": lambda: ctx.run_device(pw, n, no_tables=True),
                }
                if have_tables:
                    forms["tables"] = lambda: ctx.run_device(pw, n)
                cs = candidates(bits, n) if a.csweep else []
                if a.csweep and a.cs:   # (windows that would need more than 64 windows are left out)
                    cs = [c for c in (int(x) for x in a.cs.split(",")) if -(-(bits + 1) // c) <= 64]
                for c in cs:
                    forms[f"c{c}"] = (lambda c=c: ctx.run_narrow_device(pn, n, width, bits, c=c))
                res = {k: f() for k, f in forms.items()}   # warm-up: workspaces; and the results must agree
                assert all(r[0] == res["plain"][0] for r in res.values()), (cname, logn, bits)
                ms = {k: [] for k in forms}
                for _ in range(a.reps):
                    for k, f in forms.items():
                        ms[k].append(timed(f)[0])
                ni, wi = res["narrow"][1], res["plain"][1]
                ph = ni["phase_ms"]
                share = (ph["digits"] + ph["sort"]) / max(ph["total"], 1e-9)
                wide_forms = [k for k in ("plain", "tables") if k in ms]
                best = min(wide_forms, key=lambda k: statistics.median(ms[k]))
                ratio = statistics.median(ms[best]) / statistics.median(ms["narrow"])
                entries = (1 if te else 2) * wi["K"] / ni["K"]
                ok = statistics.median(ms["narrow"]) <= max(ms[best])
                emit(f"{cname:6s} 2^{logn} b={bits:3d} | {fmt(ms['narrow'])} c={ni['c']:2d}/K={ni['K']:2d} {100 * share:4.0f}% | "
                     f"{fmt(ms['plain'])} c={wi['c']:2d}/K={wi['K']:2d} | {fmt(ms['tables']) if 'tables' in ms else '       -':s} | "
                     f"{ratio:5.2f}x | {entries:5.2f}x | {'ok' if ok else 'SLOWER than ' + best}")
                if cs:
                    emit("        c sweep, narrow ms: " + "  ".join(f"c{c} {statistics.median(ms[f'c{c}']):.3f}" for c in cs))
                ctx.device_free(pn)
                ctx.device_free(pw)
            ctx.close()


if __name__ == "__main__":
    main()
