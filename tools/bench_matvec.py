#!/usr/bin/env python3
"""msm_scalars_matvec timed (profiles/matvec_time.txt), and the sweep that sets the two thresholds of its plan.

Workloads over n = 2^log2n rows and columns, 32-byte scalars:
    (a) r1cs        row lengths 1 .. 4, plus one row in 2^10 of length 2^10; columns uniform, and column 0 hit by every row
    (b) r1cs^T      the transposed pattern of (a): the column of every row is a row of n entries, the rest Poisson around 3.5
    (c) permutation a random permutation in the all-ones form: the gather y[i] = x[perm[i]], no multiplication
    (d) identity    col = row with coefficients: one multiplication per row and a gather that costs nothing
Yardsticks from the same run: msm_scalars_inner over nnz(a) elements (the same multiplications, streamed operands),
msm_scalars_mul over n, a device-to-device copy of x (torch, if it is there), and -- up to 2^20 rows -- the host path the operator
replaces for (a): download x, the product in Python integers, upload y.

Beside each time stands the gather estimate: nnz divided by the scattered-line rate of tools/ubench_gather, about
30e9 lines/s while the gathered range is within 0.5 GB and 13e9 beyond it.

The patterns are made with numpy on the host and uploaded; the coefficients are generated on the device (their values do not
matter to the time) and the matrices are created from device arrays, so that 2^24 rows need no 2 GB of host coefficients.
Per size every form is warmed up, forms alternate inside each repeat, each figure is the wall time of the call (launches and
synchronisation) as the median of the repeats with the [min, max] spread.  Nothing is gated: whatever comes out is what the file says.

The sweep (--sweep LOG2N) creates (a) and (b) at every pair of thresholds through msm_test_set_matvec_geometry and times them.
    python3 tools/bench_matvec.py [--reps 7] [--logn 16,20,24] [--sweep 20] [--out profiles/matvec_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from montgomery_amd import _lib, api  # noqa: E402
from montgomery_amd.api import MsmContext  # noqa: E402

Q = api.BLS12_377_PARAMS.order
SHORT_MAX = (4, 8, 16, 32, 64, 1024)
PART_LEN = (256, 1024, 4096, 8192, 16384, 65536)


def med(xs):
    return statistics.median(xs)


def fmt(xs):
    return f"{med(xs):9.3f} [{min(xs):.3f}, {max(xs):.3f}]"


def gather_ms(nnz, x_bytes):
    return nnz / (30e9 if x_bytes <= 0.5e9 else 13e9) * 1e3


def pattern_r1cs(n, rng):
    lens = rng.integers(1, 5, n, dtype=np.int64)
    if n >= 1024:
        lens[::1024] = 1024
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    col = rng.integers(0, n, int(row_ptr[-1]), dtype=np.uint32)
    col[row_ptr[:-1]] = 0
    return row_ptr.astype(np.uint32), col, lens


def pattern_transposed(n, col, lens):
    order = np.argsort(col, kind="stable")
    t_col = np.repeat(np.arange(n, dtype=np.uint32), lens)[order]
    t_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=t_ptr[1:])
    return t_ptr.astype(np.uint32), t_col


class Bench:
    def __init__(self):
        self.ctx = MsmContext(_lib.CURVE_BLS12_377_G1)

    def upload_u32(self, a):
        raw = np.ascontiguousarray(a, dtype="<u4").tobytes()
        p = self.ctx.device_alloc(max(len(raw), 32))
        self.ctx.device_upload(p, raw)
        return p

    def matrix(self, n, row_ptr, col, d_val, geometry=(0, 0)):
        """from device arrays; d_val: device coefficients (at least nnz of them) or None"""
        ctx = self.ctx
        d_rp, d_col = self.upload_u32(row_ptr), self.upload_u32(col)
        assert ctx._lib.msm_test_set_matvec_geometry(ctx._h, *geometry) == 0
        mid = ctx.matrix_create(n, n, d_rp, d_col, d_val, nnz=len(col), on_device=True)
        assert ctx._lib.msm_test_set_matvec_geometry(ctx._h, 0, 0) == 0
        ctx.device_free(d_rp)
        ctx.device_free(d_col)
        return mid

    def last(self):
        out = (ctypes.c_int32 * 5)()
        self.ctx._lib.msm_test_last_matvec(self.ctx._h, out, 5)
        return list(out)


def time_forms(forms, reps):
    for f in forms.values():
        f()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def host_path(ctx, x, y, n, row_ptr, col, val_raw):
    """download x, the product of (a) in Python integers, upload y: one run, ms"""
    t0 = time.perf_counter()
    raw = ctx.device_download(x, 32 * n)
    xs = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]
    vs = [int.from_bytes(val_raw[32 * j:32 * j + 32], "little") for j in range(len(col))]
    rp, cl = row_ptr.tolist(), col.tolist()
    out = bytearray(32 * n)
    for r in range(n):
        s = 0
        for j in range(rp[r], rp[r + 1]):
            s += vs[j] * xs[cl[j]]
        out[32 * r:32 * r + 32] = (s % Q).to_bytes(32, "little")
    ctx.device_upload(y, bytes(out))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", default="16,20,24")
    ap.add_argument("--sweep", default="20", help="log2 rows of the threshold sweep, comma separated; empty: no sweep")
    ap.add_argument("--host-max", type=int, default=20, help="largest log2n at which the host path is timed")
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
    try:
        import torch
    except Exception:   # (no torch, or one that cannot start: the copy yardstick is left out)
        torch = None
    B = Bench()
    ctx = B.ctx
    emit(f"# msm_scalars_matvec on BLS12-377 over n x n matrices, 32-byte scalars; wall ms of a call: median [min, max] of {a.reps} "
         "repeats, forms alternating; gather = nnz / the scattered-line rate (30e9/s within 0.5 GB of x, 13e9/s beyond)")
    emit("# rows: workload | nnz | long rows, parts, launches | its time | gather estimate | yardstick | its time | ratio")
    for logn in [int(v) for v in a.logn.split(",") if v]:
        n = 1 << logn
        rng = np.random.default_rng(1000 + logn)
        rp_a, col_a, lens = pattern_r1cs(n, rng)
        nnz = len(col_a)
        rp_b, col_b = pattern_transposed(n, col_a, lens)
        d_val, d_w = ctx.device_alloc(32 * nnz), ctx.device_alloc(32 * nnz)
        ctx.generate_scalars(nnz, seed=31, into=d_val)
        ctx.generate_scalars(nnz, seed=32, into=d_w)
        x, y = ctx.device_alloc(32 * n), ctx.device_alloc(32 * n)
        ctx.generate_scalars(n, seed=33, into=x)
        mats = {
            "a r1cs": (B.matrix(n, rp_a, col_a, d_val), nnz),
            "b r1cs^T": (B.matrix(n, rp_b, col_b, d_val), nnz),
            "c permutation (ones)": (B.matrix(n, np.arange(n + 1), rng.permutation(n), None), n),
            "d identity": (B.matrix(n, np.arange(n + 1), np.arange(n), d_val), n),
        }
        forms = {k: (lambda m=m: ctx.scalars_matvec(m, y, x)) for k, (m, _) in mats.items()}
        forms["inner"] = lambda: ctx.scalars_inner(d_val, d_w, nnz)
        forms["mul"] = lambda: ctx.scalars_mul(y, x, d_val, n)
        if torch is not None:
            tx = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
            ty = torch.empty_like(tx)

            def copy():
                ty.copy_(tx)
                torch.cuda.synchronize()
            forms["copy"] = copy
        shapes = {}
        for k, (m, _) in mats.items():
            ctx.scalars_matvec(m, y, x)
            shapes[k] = B.last()[2:]
        ms = time_forms(forms, a.reps)

        def row(name, z, yard, ys):
            xs = ms[name]
            emit(f"2^{logn} | {name:22s} | {z:9d} | {str(shapes[name]):22s} | {fmt(xs)} | {gather_ms(z, 32 * n):7.3f} | {yard:24s} | "
                 f"{fmt(ys)} | {med(xs) / max(med(ys), 1e-9):6.2f}x")

        row("a r1cs", nnz, "inner over nnz", ms["inner"])
        row("b r1cs^T", nnz, "inner over nnz", ms["inner"])
        row("b r1cs^T", nnz, "a r1cs", ms["a r1cs"])
        row("c permutation (ones)", n, "copy of x" if "copy" in ms else "mul over n", ms.get("copy", ms["mul"]))
        row("c permutation (ones)", n, "mul over n", ms["mul"])
        row("d identity", n, "mul over n", ms["mul"])
        if logn <= a.host_max:
            val_raw = ctx.device_download(d_val, 32 * nnz)
            t = host_path(ctx, x, y, n, rp_a, col_a, val_raw)
            emit(f"2^{logn} | a r1cs                 | {nnz:9d} | host path: download x, Python product, upload y (one run) | {t:12.1f} ms | "
                 f"{t / max(med(ms['a r1cs']), 1e-9):9.0f}x the operator")
        for m, _ in mats.values():
            ctx.matrix_destroy(m)
        for p in (d_val, d_w, x, y):
            ctx.device_free(p)
    for logn in [int(v) for v in a.sweep.split(",") if v]:
        n = 1 << logn
        rng = np.random.default_rng(1000 + logn)
        rp_a, col_a, lens = pattern_r1cs(n, rng)
        nnz = len(col_a)
        rp_b, col_b = pattern_transposed(n, col_a, lens)
        d_val = ctx.device_alloc(32 * nnz)
        ctx.generate_scalars(nnz, seed=31, into=d_val)
        x, y = ctx.device_alloc(32 * n), ctx.device_alloc(32 * n)
        ctx.generate_scalars(n, seed=33, into=x)
        emit(f"# sweep at 2^{logn} rows, nnz = {nnz}: median ms of 5 of (a) r1cs / (b) r1cs^T per (short_max, part_len); "
             "(parts of a, parts of b)")
        emit("# short_max \\ part_len " + " ".join(f"{p:>24d}" for p in PART_LEN))
        for s in SHORT_MAX:
            cells = []
            for p in PART_LEN:
                ma, mb = B.matrix(n, rp_a, col_a, d_val, (s, p)), B.matrix(n, rp_b, col_b, d_val, (s, p))
                ms = time_forms({"a": lambda: ctx.scalars_matvec(ma, y, x), "b": lambda: ctx.scalars_matvec(mb, y, x)}, 5)
                ctx.scalars_matvec(ma, y, x)
                pa = B.last()[3]
                ctx.scalars_matvec(mb, y, x)
                pb = B.last()[3]
                cells.append(f"{med(ms['a']):7.3f}/{med(ms['b']):7.3f} ({pa},{pb})")
                ctx.matrix_destroy(ma)
                ctx.matrix_destroy(mb)
            emit(f"{s:>20d}   " + " ".join(f"{c:>24s}" for c in cells))
        for p in (d_val, x, y):
            ctx.device_free(p)
    ctx.close()


if __name__ == "__main__":
    main()
