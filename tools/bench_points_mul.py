#!/usr/bin/env python3
"""msm_points_mul / msm_points_mul_base timed (profiles/points_mul_time.txt).

Per curve and n, from a resident set of n points and n resident scalars into a second point set:
  var         msm_points_mul: row i under scalar i
  base        msm_points_mul_base with the table of the base cached
  base+build  the same with another base every call, the table path forced: every call builds the table
  bcast       msm_points_mul_base through the variable-base kernel over a broadcast row (the path of short uncached calls)
and as yardsticks from entry points that existed before, in the same process:
  lincomb     msm_points_lincomb scaling the same set by ONE scalar
  msm         msm_run over the same rows and scalars
One process per library, inputs resident before the timing, every form warmed up, forms alternating inside each repeat; each
figure is the median of the repeats with the [min, max] spread.

--libs name=path,...  times candidate builds of the library (make ab_pmul NAME=... EXTRA=-D...) the same way, each in a process of
its own with MSM_HIP_LIB set, `-` = the in-tree build; only var / base / base+build / bcast are printed for them.
--sweep  adds the two paths of an uncached base at 2^10 .. 2^18 rows on the first curve: where they meet is the row count from
which msm_points_mul_base builds its table.

    python3 tools/bench_points_mul.py [--reps 5] [--curves bls377,pallas,bn254,ed377] [--logn 14,16,20,24] [--sweep]
                                      [--libs=-,w3=ab_builds/libmsm_pmul_w3.so,...] [--out profiles/points_mul_time.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3   # a fixed 253-bit scalar, reduced per curve
FORMS = ("var", "base", "base+build", "bcast", "lincomb", "msm")


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def fmt(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def curves():
    from montgomery_amd import _lib, api

    return {"bls377": (_lib.CURVE_BLS12_377_G1, api.BLS12_377_PARAMS.order), "pallas": (_lib.CURVE_PALLAS, api.PALLAS_PARAMS.order),
            "bn254": (_lib.CURVE_BN254_G1, api.BN254_PARAMS.order), "ed377": (_lib.CURVE_ED_ON_BLS12_377, api.ED_ON_BLS12_377_PARAMS.order),
            "bls381": (_lib.CURVE_BLS12_381_G1, api.BLS12_381_PARAMS.order), "grumpkin": (_lib.CURVE_GRUMPKIN, api.GRUMPKIN_PARAMS.order),
            "vesta": (_lib.CURVE_VESTA, api.VESTA_PARAMS.order)}


def measure(cname, logn, reps, forms):
    """{form: [ms, ...]} and the library's report of the last variable-base and table calls"""
    from montgomery_amd.api import MsmContext

    cid, q = curves()[cname]
    n = 1 << logn
    ctx = MsmContext(cid)
    ctx.generate_points(n, seed=7)
    src, dst = 0, ctx.pointset_create()
    ctx.pointset_select(src)
    dev, _ = ctx.generate_scalars(n, seed=9)
    bases = [ctx.get_points(i, 1) for i in (1, 2)]
    flip = [0]

    def path(p):
        ctx._check(ctx._lib.msm_test_set_points_mul_base_path(ctx._h, p))

    def report():
        out = (ctypes.c_int32 * 4)()
        ctx._lib.msm_test_last_points_mul(ctx._h, out, 4)
        return list(out)

    def base_build():
        flip[0] ^= 1
        path(1)
        ctx.points_mul_base(dev, bases[flip[0]], count=n, dst=dst)

    def base_cached():
        path(1)
        ctx.points_mul_base(dev, None, count=n, dst=dst)

    def bcast():
        path(2)
        ctx.points_mul_base(dev, bases[0], count=n, dst=dst)

    calls = {
        "var": lambda: ctx.points_mul(dev, src=src, count=n, dst=dst),
        "base": base_cached,
        "base+build": base_build,
        "bcast": bcast,
        "lincomb": lambda: ctx.points_lincomb(U % q, src_a=src, a_lo=0, count=n, dst=dst),
        "msm": lambda: ctx.run_device(dev, n, no_tables=True),
    }
    info = {}
    for k in forms:   # warm-up: workspaces, the destination's rows, the generator's table
        calls[k]()
        if k in ("var", "base"):
            info[k] = report()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k in forms:
            if k == "base":   # (base+build leaves another base's table behind)
                base_cached()
            ms[k].append(timed(calls[k]))
    ctx.close()
    return ms, info


def child(a):
    out = {}
    for logn in [int(x) for x in a.logn.split(",")]:
        ms, info = measure(a.curves.split(",")[0], logn, a.reps, FORMS[:4])
        out[logn] = {"ms": ms, "info": info}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curves", default="bls377,pallas,bn254,ed377")
    ap.add_argument("--logn", default="14,16,20,24")
    ap.add_argument("--libs", default="")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current line by line: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    logns = [int(x) for x in a.logn.split(",")]
    emit(f"# msm_points_mul / msm_points_mul_base from n resident points and n resident scalars into a second set; ms: median [min, max] of "
         f"{a.reps} repeats (3 at 2^24), forms alternating")
    emit("# columns: curve, log2 n | " + " | ".join(FORMS) + " | var / lincomb | base / var | grid blocks, w | table rows, w_b")
    for cname in a.curves.split(","):
        for logn in logns:
            ms, info = measure(cname, logn, 3 if logn >= 24 else a.reps, FORMS)
            med = {k: statistics.median(v) for k, v in ms.items()}
            emit(f"{cname:6s} 2^{logn} | " + " | ".join(fmt(ms[k]) for k in FORMS) +
                 f" | {med['var'] / med['lincomb']:5.2f}x | {med['base'] / med['var']:5.2f}x | {info['var'][0]}, {info['var'][1]} | "
                 f"{info['base'][3]}, {info['base'][1]}")
    if a.sweep:
        cname = a.curves.split(",")[0]
        emit(f"# an uncached base on {cname}: the table path with its build against the broadcast row; columns: log2 n | base+build | bcast")
        for logn in range(10, 19):
            ms, _ = measure(cname, logn, a.reps, ("base+build", "bcast"))
            emit(f"{cname:6s} 2^{logn} | " + " | ".join(fmt(ms[k]) for k in ("base+build", "bcast")))
    if a.libs:
        cname = a.curves.split(",")[0]
        ab_logn = ",".join(str(x) for x in logns if x <= 20)
        emit(f"# candidate builds on {cname}, one process each; columns: build, log2 n | var | base | base+build | bcast | grid blocks, w | table rows, w_b")
        for spec in a.libs.split(","):
            name, _, lib = spec.partition("=")
            env = dict(os.environ)
            if name != "-":
                env["MSM_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--curves", cname, "--logn", ab_logn, "--reps", str(a.reps)],
                                 env=env, capture_output=True, text=True)
            res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode or not res:
                emit(f"{name:8s} failed: {out.stderr.strip()[-300:]}")
                continue
            for logn, r in sorted(json.loads(res[0][7:]).items(), key=lambda kv: int(kv[0])):
                emit(f"{name if name != '-' else 'in-tree':8s} 2^{logn} | " + " | ".join(fmt(r["ms"][k]) for k in FORMS[:4]) +
                     f" | {r['info']['var'][0]}, {r['info']['var'][1]} | {r['info']['base'][3]}, {r['info']['base'][1]}")


if __name__ == "__main__":
    main()
