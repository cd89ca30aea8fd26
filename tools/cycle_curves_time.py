#!/usr/bin/env python3
"""Times of BN254 G1, Grumpkin and Vesta with Pallas beside them in the same run (profiles/cycle_curves_time.txt).

Protocol of bench.py: resident points, fresh device scalars for every run (the narrow step: four value sets uploaded before
the timing, cycled), 15 runs of which the first 5 are discarded, the median of the rest with its [min, max].  Every step (one curve, one kind of measurement) runs in a child process of its own
under its own time limit; the first step that fails ends the run.
    python3 tools/cycle_curves_time.py [--out profiles/cycle_curves_time.txt] [--logn 16,20,24,26] [--sweep] [--curves pallas,vesta,bn254,grumpkin]
    python3 tools/cycle_curves_time.py --step KIND CURVE [ARG]     (one step, what the parent starts)
Kinds: msm LOGN (plain path and window tables where the library builds them), batch (2^14 x 16), narrow (2^22 x 64 bits),
ingest (compressed load of 2^24 points), sweep LOGN (window size against time on the plain path).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE_IDS = {"pallas": 3, "bn254": 4, "grumpkin": 5, "vesta": 6}
RUNS, DISCARD = 15, 5
SWEEP_CS = {20: (13, 16, 18), 23: (16, 18, 19, 21), 24: (16, 18, 19, 21, 22), 25: (16, 19, 21, 22), 26: (16, 21, 22)}


def fmt(xs):
    xs = xs[DISCARD:]
    return f"{statistics.median(xs):9.3f} ms [{min(xs):.3f}, {max(xs):.3f}]"


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def step(kind, curve, arg):
    from montgomery_amd.api import MsmContext

    ctx = MsmContext(CURVE_IDS[curve])
    key = lambda r: r.as_tuple()   # noqa: E731
    if kind in ("msm", "sweep"):
        n = 1 << arg
        ctx.generate_points(n, seed=7)
        dev, _ = ctx.generate_scalars(n, seed=100)
        forms = [("plain", dict(no_tables=True), None)] if kind == "msm" else [(f"c={c}", dict(no_tables=True, c=c), None) for c in SWEEP_CS[arg]]
        for name, kw, _ in forms:
            ts, info = [], None
            for r in range(RUNS):
                ctx.generate_scalars(n, seed=200 + r, into=dev)
                ms, (res, info) = timed(lambda: ctx.run_device(dev, n, **kw))
                ts.append(ms)
            print(f"{curve:9s} {kind:6s} 2^{arg:<2d} {name:7s} {fmt(ts)}  c = {info['c']:2d} K = {info['K']:2d}  accumulate {info['phase_ms']['accumulate']:.3f} ms", flush=True)
        if kind == "msm":
            res, info = ctx.run_device(dev, n)          # the default plan builds window tables where they fit
            if info["tables"]:
                plain = key(ctx.run_device(dev, n, no_tables=True)[0])
                assert key(res) == plain
                ts = []
                for r in range(RUNS):
                    ctx.generate_scalars(n, seed=300 + r, into=dev)
                    ms, (res, info) = timed(lambda: ctx.run_device(dev, n))
                    ts.append(ms)
                print(f"{curve:9s} {kind:6s} 2^{arg:<2d} tables  {fmt(ts)}  c = {info['c']:2d} K = {info['K']:2d}", flush=True)
            else:
                print(f"{curve:9s} {kind:6s} 2^{arg:<2d} tables  none (the default plan stays on the plain path)", flush=True)
    elif kind == "batch":
        n, B = 1 << 14, 16
        ctx.generate_points(n, seed=7)
        devs = [ctx.device_alloc(32 * n) for _ in range(B)]
        ts, ts1 = [], []
        for r in range(RUNS):
            for b, d in enumerate(devs):
                ctx.generate_scalars(n, seed=400 + 16 * r + b, into=d)
            ms, out = timed(lambda: ctx.run_batch_device(devs, n))
            ts.append(ms)
            ms1, single = timed(lambda: [ctx.run_device(d, n)[0] for d in devs])
            ts1.append(ms1)
            assert [key(o[0]) for o in out] == [key(s) for s in single]
        print(f"{curve:9s} batch  2^14 x 16        {fmt(ts)}  one by one {fmt(ts1)}", flush=True)
    elif kind == "narrow":
        import numpy as np

        # the values are made and uploaded before anything is timed (four distinct sets, cycled as bench.py cycles its
        # scalar sets), and one call warms the path up: nothing but msm_run_narrow runs between two timed calls
        n = 1 << 22
        ctx.generate_points(n, seed=7)
        bufs = []
        for k in range(4):
            rng = np.random.default_rng(500 + k)
            vals = rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)
            bufs.append(ctx.device_alloc(8 * n))
            ctx.device_upload(bufs[-1], vals.tobytes())
        ctx.run_narrow_device(bufs[0], n, 8, 64)
        ts, info = [], None
        for r in range(RUNS):
            ms, (res, info) = timed(lambda: ctx.run_narrow_device(bufs[r % 4], n, 8, 64))
            ts.append(ms)
        print(f"{curve:9s} narrow 2^22 x 64 bits   {fmt(ts)}  c = {info['c']:2d} K = {info['K']:2d}", flush=True)
    elif kind == "ingest":
        n = 1 << 24
        ctx.generate_points(n, seed=7)
        raw = ctx.get_points(0, n)
        comp = ctx.get_points(0, n, compressed=True)
        for name, data, kw in (("compressed, subgroup", comp, dict(compressed=True, validate="subgroup")),
                               ("uncompressed, curve", raw, dict(validate="curve")), ("uncompressed, none", raw, dict(validate=None))):
            ts = [timed(lambda: ctx.load_points(data, **kw))[0] for _ in range(5)]
            print(f"{curve:9s} ingest 2^24 {name:22s} {statistics.median(ts[1:]):9.1f} ms [{min(ts[1:]):.1f}, {max(ts[1:]):.1f}] (host buffer, 4 runs after a warm-up)", flush=True)
        assert ctx.get_points(0, 1 << 10) == raw[: 64 << 10]
    else:
        raise SystemExit(f"unknown step {kind}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", nargs="+")
    ap.add_argument("--out", default=None)
    ap.add_argument("--logn", default="16,20,24,26")
    ap.add_argument("--curves", default="pallas,vesta,bn254,grumpkin")
    ap.add_argument("--kinds", default="msm,batch,narrow,ingest")
    ap.add_argument("--sweep", default="", help="sizes of the plan sweep, e.g. 20,23,24,25,26")
    a = ap.parse_args()
    if a.step:
        step(a.step[0], a.step[1], int(a.step[2]) if len(a.step) > 2 else 0)
        return
    curves, kinds = a.curves.split(","), a.kinds.split(",")
    steps = []
    for lg in [int(x) for x in a.logn.split(",")] if "msm" in kinds else []:
        steps += [("msm", c, lg, 120 + (1 << max(0, lg - 20)) * 6) for c in curves]
    for k, limit in (("batch", 180), ("narrow", 240), ("ingest", 600)):
        if k in kinds:
            steps += [(k, c, 0, limit) for c in curves]
    for lg in [int(x) for x in a.sweep.split(",") if x]:
        steps += [("sweep", c, lg, 240 + (1 << max(0, lg - 20)) * 12) for c in curves]
    lines = [f"# tools/cycle_curves_time.py: {RUNS} runs, the first {DISCARD} discarded, median [min, max]; resident points, fresh device scalars per run"]
    print(lines[0], flush=True)
    for kind, curve, arg, limit in steps:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, curve, str(arg)], capture_output=True,
                                 text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{curve} {kind} {arg}: time limit of {limit} s -- run ended")
            print(lines[-1], flush=True)
            break
        got = [l for l in out.stdout.splitlines() if l.strip()]
        lines += got
        print("\n".join(got), flush=True)
        if out.returncode != 0:
            lines.append(f"{curve} {kind} {arg}: exit status {out.returncode} -- run ended\n{out.stderr[-2000:]}")
            print(lines[-1], flush=True)
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if len(lines) and "run ended" not in lines[-1] else 1)


if __name__ == "__main__":
    main()
