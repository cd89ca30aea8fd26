"""Same schedules, same results: a fixed list of small calls -- uncut, cut into window groups and into ranges of the points, the
narrow, indexed and batched forms, one window of msm_window_sums, and the two-group paths at 2^21 / 2^22 -- one line per call with
its plan, its statistics and its affine result, from two builds of libmsm_hip.so side by side (lines that start with "#" are
shown and not compared).
usage: python tools/group_schedule_parity.py OTHER.so [OUT.txt]     (the in-tree build against OTHER.so, e.g. a build of the
parent commit made with `make ab`; exit status 1 if any line differs)
       python tools/group_schedule_parity.py --child               (the lines of the build MSM_HIP_LIB names)"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def child():
    import numpy as np
    from montgomery_amd.api import MsmContext
    from test_gpu_cut_calls import _limits

    def line(label, res, info, extra=""):
        at = "inf" if res.isZero else f"{res.x:x} {res.y:x}"
        print(f"{label}: c={info['c']} K={info['K']} tables={int(info['tables'])} rounds={info['rounds']} n_pairs={info['n_pairs']} "
              f"n_pairs_algo={info['n_pairs_algo']} max_bucket={info['max_bucket']} {extra}-> {at}", flush=True)

    for name, cid in (("bls377", 0), ("ed377", 1)):
        te = cid == 1
        ctx = MsmContext(cid)
        for n in ((1 << 14), (1 << 15) + 11, (1 << 16) + 37):
            ctx.generate_points(n, seed=41)
            dev, host = ctx.generate_scalars(n, seed=43, to_host=True)
            line(f"{name} n={n} default", *ctx.run_device(dev, n))
            line(f"{name} n={n} default again", *ctx.run_device(dev, n))
            c, K = ctx.plan(n, c=10, no_tables=True)
            line(f"{name} n={n} c=10 uncut", *ctx.run_device(dev, n, c=10, no_tables=True))
            for cut, limit in _limits(te, n, c, K).items():
                ctx.set_workspace_limit(limit)
                line(f"{name} n={n} c=10 {cut}", *ctx.run_device(dev, n, c=10, no_tables=True))
                line(f"{name} n={n} c=10 {cut} host", *ctx.run(host, c=10, no_tables=True))
                line(f"{name} n={n} default {cut}", *ctx.run_device(dev, n))
                ctx.set_workspace_limit(0)
        n = 1 << 14
        ctx.generate_points(n, seed=45)
        dev, host = ctx.generate_scalars(n, seed=47, to_host=True)
        rng = np.random.default_rng(49)
        line(f"{name} narrow", *ctx.run_narrow(rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int32)))
        idx = rng.integers(0, n, size=2 * n + 3, dtype=np.uint32)
        sc = rng.integers(0, 256, size=(idx.size, 32), dtype=np.uint8)
        sc[:, 31] &= 3
        line(f"{name} indexed", *ctx.msm_indexed(sc.tobytes(), idx))
        line(f"{name} indexed narrow", *ctx.msm_indexed_narrow(rng.integers(0, 1 << 16, size=idx.size, dtype=np.uint16), idx))
        for b, (res, info) in enumerate(ctx.run_batch([host] + [sc[b * n:(b + 1) * n].tobytes() for b in range(2)])):
            line(f"{name} batch[{b}]", res, info)
        # one window: its sum as the affine point (the projective X, Y, Z a call hands out are not compared: "#" lines)
        sums, info = ctx.window_sums(dev, n, 2, 3, on_device=True)
        line(f"{name} window_sums [2, 3)", ctx.combine(sums, 1, info["c"]), info)
        again, _ = ctx.window_sums(dev, n, 2, 3, on_device=True)
        print(f"# {name} window_sums [2, 3) sha256 of X || Y || Z, two calls: {hashlib.sha256(sums).hexdigest()[:16]} "
              f"{hashlib.sha256(again).hexdigest()[:16]}", flush=True)
        ctx.close()
    ctx = MsmContext(0)
    for lg, kw in ((21, {}), (22, {"no_tables": True})):
        n = 1 << lg
        ctx.generate_points(n, seed=51)
        dev, _ = ctx.generate_scalars(n, seed=53)
        for rep in range(2):     # (the first default-plan call builds the window tables, the second runs on them)
            line(f"bls377 n=2^{lg} {kw or 'default'} call {rep}", *ctx.run_device(dev, n, **kw))
    ctx.close()


def lines_of(lib):
    env = dict(os.environ)
    env.pop("MSM_HIP_LIB", None)
    if lib:
        env["MSM_HIP_LIB"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
    if out.returncode:
        sys.exit(f"{lib or 'in-tree build'}: exit status {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return out.stdout.splitlines()


def main():
    if sys.argv[1:] == ["--child"]:
        return child()
    other = sys.argv[1]
    a, b = lines_of(other), lines_of(None)
    rows = [f"# {os.path.basename(other)} (first line of each pair) against the in-tree build (second line)"]
    differ = len(a) != len(b)
    for x, y in zip(a, b):
        if x.startswith("#") and y.startswith("#"):      # shown, not compared
            rows += [x, y]
            continue
        differ |= x != y
        rows += [x, y, "  same" if x == y else "  DIFFERENT"]
    rows.append(f"# {len(a)} / {len(b)} lines: " + ("DIFFERENT" if differ else "every line identical"))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text)
    sys.exit(1 if differ else 0)


main()
