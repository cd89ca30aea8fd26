#!/usr/bin/env python3
"""msm_run_indexed against what a caller had to do before it existed (profiles/indexed_msm_time.txt).

Per curve, resident count n and m = n/2, n/8, n/64 entries with uniformly random DISTINCT indices and uniform scalars, all
inputs device-resident:
    indexed          msm_run_indexed over the m entries, indices in random order
    indexed sorted   the same entries in ascending index order (what sparse_from_dense hands over)
    dense            msm_run over the dense equivalent: n scalars, zeros elsewhere -- the baseline
    floor            msm_run over the first m resident points with the same m scalars: a dense MSM of m points
One process; every form is warmed up once (the first call of a shape allocates its workspace), then the forms alternate inside
each repeat.  Each figure is the host clock around the call -- every call ends in a device synchronise -- as the median of the
repeats with the [min, max] spread; c / K is the plan that ran, T marks a run on window tables.  The indexed results are checked
against the dense one (bit-identical) before anything is timed.
    python3 tools/bench_indexed.py [--reps 7] [--curves bls377,pallas] [--logn 24,26] [--out profiles/indexed_msm_time.txt]
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
          "pallas": _lib.CURVE_PALLAS, "bn254": _lib.CURVE_BN254_G1, "grumpkin": _lib.CURVE_GRUMPKIN, "vesta": _lib.CURVE_VESTA}
SHARES = (2, 8, 64)   # m = n / share


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def upload(ctx, arr):
    """a contiguous numpy array into a device buffer of its own, without a second host copy"""
    p = ctx.device_alloc(arr.nbytes + 16)
    ctx.device_upload(p, np.ctypeslib.as_ctypes(arr.reshape(-1).view(np.uint8)))
    return p


def plan_str(info):
    return f"{info['c']}/{info['K']}{'T' if info['tables'] else ''}"


def grid_point(ctx, n, m, reps, seed, emit):
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)[:m].astype(np.uint32)
    d_sc, sc_raw = ctx.generate_scalars(m, seed=seed, to_host=True, into=ctx.device_alloc(32 * m), raw=True)
    sc = np.frombuffer(sc_raw, dtype=np.uint8).reshape(m, 32)
    dense = np.zeros((n, 32), dtype=np.uint8)
    dense[idx] = sc
    order = np.argsort(idx, kind="stable")
    bufs = {"idx": upload(ctx, idx), "idx_sorted": upload(ctx, np.ascontiguousarray(idx[order])),
            "sc_sorted": upload(ctx, np.ascontiguousarray(sc[order])), "dense": upload(ctx, dense), "sc": d_sc}
    del dense, sc, sc_raw
    forms = {
        "indexed": lambda: ctx.msm_indexed_device(bufs["sc"], bufs["idx"], m),
        "indexed sorted": lambda: ctx.msm_indexed_device(bufs["sc_sorted"], bufs["idx_sorted"], m),
        "dense": lambda: ctx.run_device(bufs["dense"], n),
        "floor": lambda: ctx.run_device(bufs["sc"], m),
    }
    try:
        first = {name: f() for name, f in forms.items()}                  # warm-up, and the check of section 6
        ref = first["dense"][0]
        for name in ("indexed", "indexed sorted"):
            if first[name][0] != ref:
                raise SystemExit(f"{name} differs from the dense equivalent at n = {n}, m = {m}")
        ms = {name: [] for name in forms}
        for _ in range(reps):
            for name, f in forms.items():
                ms[name].append(timed(f)[0])
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name in forms:
            extra = ""
            if name.startswith("indexed"):
                extra = f"   dense / this {med['dense'] / med[name]:5.2f}   this / floor {med[name] / med['floor']:5.2f}"
            emit(f"  m = n/{n // m:<3d} {name:15s} {fmt(ms[name])} ms   c/K {plan_str(first[name][1]):8s}{extra}")
    finally:
        for p in bufs.values():
            ctx.device_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="bls377,pallas")
    ap.add_argument("--logn", default="24,26")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# tools/bench_indexed.py --reps {a.reps} --curves {a.curves} --logn {a.logn}")
    emit("# wall ms per call, median [min, max]; device-resident inputs, distinct uniformly random indices, uniform scalars")
    for name in a.curves.split(","):
        for logn in (int(x) for x in a.logn.split(",")):
            n = 1 << logn
            ctx = MsmContext(CURVES[name])
            try:
                ctx.generate_points(n, seed=100 + logn)
                emit(f"{name}  n = 2^{logn} resident points")
                for share in SHARES:
                    grid_point(ctx, n, n // share, a.reps, 1000 * logn + share, emit)
            finally:
                ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
