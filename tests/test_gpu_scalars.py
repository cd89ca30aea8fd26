"""The resident scalar-vector operations on the GPU: msm_scalars_lincomb, _mul, _inner, _powers and msm_device_download.  `-m gpu`.

Expected values are Python integers mod cv.q; every comparison is bit-exact.  Sizes are the smallest that give a ragged wave
(63, 65), a ragged block (257) and more than one block (321), beside 1, 64 and 256.  Vectors sit at an odd 32-byte offset inside
their allocation and carry non-canonical elements (q, q + 1, 2^256 - 1) and zeros among the random ones."""
import ctypes
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
import operator_fixture as F  # noqa: E402
from host_lib import host_library  # noqa: E402
from operator_fixture import SENTINEL, TOP, OperatorFixture as Fix, to_bytes  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (1, 63, 64, 65, 256, 257, 321)
NMAX = SHAPES[-1]


def _ints(tag, n, bound):
    return O.prng_ints(f"scalars/{tag}", n, bound)


mixed = functools.partial(F.mixed, "scalars")


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module")
def inner_grid():
    """(grid cap in blocks, lanes per block) of k_sv_inner, from the constants of scalar_vec.h"""
    L = host_library("scalars_host")
    return L.sv_inner_max_blocks(), L.sv_block()


# ---------------------------------------------------------------------------------------------- 1: shapes

def test_every_op_at_every_shape(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    A, B = mixed(f.cv, "shape/a", NMAX), mixed(f.cv, "shape/b", NMAX)
    a, b = f.vector(A), f.vector(B, pad=5)
    x, y, s = _ints(f"{f.name}/shape/xys", 3, q)
    for n in SHAPES:
        for op in ("lincomb", "one", "mul", "powers"):
            d = f.vector(n)
            if op == "lincomb":
                ctx.scalars_lincomb(d, x, a, y, b, n)
                exp = [(x * u + y * v) % q for u, v in zip(A[:n], B[:n])]
            elif op == "one":
                ctx.scalars_lincomb(d, x, a, n=n)
                exp = [x * u % q for u in A[:n]]
            elif op == "mul":
                ctx.scalars_mul(d, a, b, n)
                exp = [u * v % q for u, v in zip(A[:n], B[:n])]
            else:
                ctx.scalars_powers(d, x, n, s)
                exp = [s * pow(x, i, q) % q for i in range(n)]
            assert f.read(d, n) == exp, (f.name, op, n)
            assert ctx.device_download(d - 32, 32) == SENTINEL and ctx.device_download(d + 32 * n, 32) == SENTINEL, (op, n)
        assert ctx.scalars_inner(a, b, n) == sum(u * v for u, v in zip(A[:n], B[:n])) % q, (f.name, n)
    # the shortcut-looking scalars are ordinary input
    d = f.vector(NMAX)
    for xx, yy in ((0, 0), (1, 0), (0, 1), (1, 1), (q - 1, 1), (1, q - 1)):
        ctx.scalars_lincomb(d, xx, a, yy, b, NMAX)
        assert f.read(d, NMAX) == [(xx * u + yy * v) % q for u, v in zip(A, B)], (f.name, xx, yy)
    for ss, xx in ((1, 0), (1, 1), (0, x), (q - 1, q - 1)):
        ctx.scalars_powers(d, xx, 65, ss)
        assert f.read(d, 65) == [ss * pow(xx, i, q) % q for i in range(65)], (f.name, ss, xx)
    assert f.read(a, NMAX) == A and f.read(b, NMAX) == B          # the sources are as they were


# ---------------------------------------------------------------------------------------------- 2: inner beyond one pass

@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_inner_walks_the_capped_grid_three_times_and_a_ragged_fourth(name, inner_grid):
    """k_sv_inner runs at most INNER_MAX_BLOCKS = 1024 blocks of BLOCK = 256 lanes: 2^18 lanes, each of which takes the elements
    i = lane, lane + 2^18, ...  n = 3 * 2^18 + 77 = 786 509 (< 2^20) gives every lane three elements and the first 77 lanes --
    a wave and a ragged second one of block 0 -- a fourth.  The vectors repeat 4093 and 4099 values (two primes, so the pairs do
    not repeat within n) that hold the non-canonical elements too."""
    from montgomery_amd.api import MsmContext

    blocks, lanes = inner_grid
    assert (blocks, lanes) == (1024, 256)
    n = 3 * blocks * lanes + 77
    assert n <= 1 << 20
    cv = D.CURVE_TABLE[name]
    q, pa, pb = cv.q, 4093, 4099
    A, B = mixed(cv, "big/a", pa), mixed(cv, "big/b", pb)
    ra, rb = to_bytes(A), to_bytes(B)
    ctx = MsmContext(cv.cid)
    try:
        a, b = ctx.device_alloc(32 * n), ctx.device_alloc(32 * n)
        ctx.device_upload(a, (ra * (n // pa + 1))[:32 * n])
        ctx.device_upload(b, (rb * (n // pb + 1))[:32 * n])
        exp = sum(A[i % pa] * B[i % pb] for i in range(n)) % q
        assert ctx.scalars_inner(a, b, n) == exp
        # one element less: lane 76 loses its fourth element
        assert ctx.scalars_inner(a, b, n - 1) == (exp - A[(n - 1) % pa] * B[(n - 1) % pb]) % q
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 3: aliasing

def test_dst_may_be_a_source_and_the_fold_runs_in_place(f7):
    f, q, ctx, n = f7, f7.q, f7.ctx, NMAX
    A, B = mixed(f.cv, "alias/a", n), mixed(f.cv, "alias/b", n)
    x, y = _ints(f"{f.name}/alias/xy", 2, q)
    exp = [(x * u + y * v) % q for u, v in zip(A, B)]
    a, b = f.vector(A), f.vector(B)
    ctx.scalars_lincomb(a, x, a, y, b, n)                        # dst = a
    assert f.read(a, n) == exp and f.read(b, n) == B
    a = f.vector(A)
    ctx.scalars_lincomb(b, x, a, y, b, n)                        # dst = b
    assert f.read(b, n) == exp and f.read(a, n) == A
    b, d = f.vector(B), f.vector(n)
    ctx.scalars_lincomb(d, x, a, y, b, n)                        # disjoint
    assert f.read(d, n) == exp and f.read(a, n) == A and f.read(b, n) == B
    ctx.scalars_lincomb(d, x, a, y, a, n)                        # the sources may be one vector
    assert f.read(d, n) == [(x + y) * u % q for u in A]
    ctx.scalars_mul(a, a, b, n)                                  # dst = a, and dst = a = b
    assert f.read(a, n) == [u * v % q for u, v in zip(A, B)]
    ctx.scalars_mul(b, b, b, n)
    assert f.read(b, n) == [v * v % q for v in B]
    # the in-place fold of 2 n elements: the lower half is written, the upper half keeps its bytes (non-canonical ones included)
    V = mixed(f.cv, "alias/v", 2 * n)
    v = f.vector(V)
    assert ctx.fold_scalars(v, 2 * n, x, y) == n
    assert f.read(v, n) == [(x * V[i] + y * V[n + i]) % q for i in range(n)]
    assert f.read(v + 32 * n, n) == V[n:]
    assert ctx.device_download(v - 32, 32) == SENTINEL and ctx.device_download(v + 64 * n, 32) == SENTINEL


# ---------------------------------------------------------------------------------------------- 4: agreement with the MSM

def test_msm_over_a_folded_vector(f7):
    f, cv, q, ctx, n = f7, f7.cv, f7.q, f7.ctx, 2 * NMAX
    logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1501, want_scalars=True))
    V = mixed(cv, "msm/v", n)
    v = f.vector(V)
    lo, hi = _ints(f"{f.name}/msm/lohi", 2, q)
    h = ctx.fold_scalars(v, n, lo, hi)
    folded = [(lo * V[i] + hi * V[h + i]) % q for i in range(h)]
    got, _ = ctx.run_device(v, h)                               # over the points [0, h)
    assert f.point(got) == cv.scale_g(sum(s * k for s, k in zip(folded, logs)) % q)
    got, _ = ctx.run_device(v, h, point_lo=h)                   # and over the upper half of the points
    assert f.point(got) == cv.scale_g(sum(s * k for s, k in zip(folded, logs[h:])) % q)
    # the untouched upper half of the vector, non-canonical elements and all: msm_run takes them as their residues
    got, _ = ctx.run_device(v + 32 * h, h)
    assert f.point(got) == cv.scale_g(sum(s * k for s, k in zip(V[h:], logs)) % q)


# ---------------------------------------------------------------------------------------------- 5: refusals

def test_every_refusal_leaves_the_context_usable(f7):
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_SCALAR, MsmError

    f, q, ctx, n = f7, f7.q, f7.ctx, 65
    lib, h = ctx._lib, ctx._h
    A, B = mixed(f.cv, "bad/a", 2 * n), mixed(f.cv, "bad/b", 2 * n)
    a, b, d = f.vector(A), f.vector(B), f.vector(2 * n)
    x, y = _ints(f"{f.name}/bad/xy", 2, q)
    good = [(x * u + y * v) % q for u, v in zip(A[:n], B[:n])]

    def still_good():
        assert f.read(a, 2 * n) == A and f.read(b, 2 * n) == B          # nothing was written
        ctx.scalars_lincomb(d, x, a, y, b, n)                           # and a call succeeds
        assert f.read(d, n) == good
        assert ctx.scalars_inner(a, b, n) == sum(u * v for u, v in zip(A[:n], B[:n])) % q

    def refused(code, fn, *args, **kw):
        with pytest.raises(MsmError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn.__name__, args)
        still_good()

    # a pointer off 16 bytes, in every position
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, d + 8, x, a, y, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, d, x, a + 8, y, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, d, x, a, y, b + 4, n)
    refused(MSM_ERR_ARG, ctx.scalars_mul, d, a + 8, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_mul, d + 8, a, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_inner, a, b + 8, n)
    refused(MSM_ERR_ARG, ctx.scalars_powers, d + 8, x, n)
    # a partial overlap of dst with a, and with b: one element up, one element down, the last element
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, a + 32, x, a, y, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, a, x, a + 32, y, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, b + 32 * (n - 1), x, a, y, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, b, x, a, y, b + 32, n)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, a + 16, x, a, n=n)
    refused(MSM_ERR_ARG, ctx.scalars_mul, a + 32, a, b, n)
    refused(MSM_ERR_ARG, ctx.scalars_mul, b + 32, a, b, n)
    # host scalars at and above q
    refused(MSM_ERR_SCALAR, ctx.scalars_lincomb, d, q, a, y, b, n)
    refused(MSM_ERR_SCALAR, ctx.scalars_lincomb, d, x, a, q + 1, b, n)
    refused(MSM_ERR_SCALAR, ctx.scalars_lincomb, d, TOP, a, n=n)
    refused(MSM_ERR_SCALAR, ctx.scalars_powers, d, x, n, q)
    refused(MSM_ERR_SCALAR, ctx.scalars_powers, d, q, n, 1)
    refused(MSM_ERR_ARG, ctx.scalars_lincomb, d, x, a, y, b, 1 << 30)
    # null pointers, at the C ABI
    vp = ctypes.c_void_p
    xb = (ctypes.c_uint8 * 32).from_buffer_copy(x.to_bytes(32, "little"))
    out = (ctypes.c_uint8 * 32)()
    for rc in (lib.msm_scalars_lincomb(h, None, xb, vp(a), xb, vp(b), n), lib.msm_scalars_lincomb(h, vp(d), xb, None, xb, vp(b), n),
               lib.msm_scalars_lincomb(h, vp(d), None, vp(a), xb, vp(b), n), lib.msm_scalars_lincomb(h, vp(d), xb, vp(a), None, vp(b), n),
               lib.msm_scalars_mul(h, vp(d), vp(a), None, n), lib.msm_scalars_mul(h, None, vp(a), vp(b), n),
               lib.msm_scalars_inner(h, None, vp(b), n, out), lib.msm_scalars_inner(h, vp(a), vp(b), n, None),
               lib.msm_scalars_powers(h, None, xb, xb, n), lib.msm_scalars_powers(h, vp(d), None, xb, n),
               lib.msm_device_download(h, out, None, 32), lib.msm_device_download(h, None, vp(a), 32)):
        assert rc == MSM_ERR_ARG
        still_good()


def test_device_list_contexts_are_refused():
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    multi = MsmContext(D.CURVE_TABLE["bls377"].cid, devices=[0, 0])
    try:
        p = multi.device_alloc(64)
        multi.device_upload(p, bytes(64))
        for call in (lambda: multi.scalars_lincomb(p, 1, p, n=2), lambda: multi.scalars_mul(p, p, p, 2),
                     lambda: multi.scalars_inner(p, p, 2), lambda: multi.scalars_powers(p, 3, 2)):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == MSM_ERR_ARG
        assert multi.device_download(p, 64) == bytes(64)
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 6: n == 0, 7: round trip

def test_empty_vectors_and_the_round_trip(f7):
    f, q, ctx = f7, f7.q, f7.ctx
    lib, h = ctx._lib, ctx._h
    A = mixed(f.cv, "zero/a", 5)
    a = f.vector(A)
    ctx.scalars_lincomb(a, 3, a, 4, a, 0)
    ctx.scalars_lincomb(a, 3, a, n=0)
    ctx.scalars_mul(a, a, a, 0)
    ctx.scalars_powers(a, 3, 0)
    assert ctx.scalars_inner(a, a, 0) == 0
    assert ctx.fold_scalars(a, 0, 1, 1) == 0
    one = (ctypes.c_uint8 * 32)(1)
    out = (ctypes.c_uint8 * 32)(*([7] * 32))
    assert lib.msm_scalars_lincomb(h, None, one, None, one, None, 0) == 0      # null vectors are fine where nothing is read
    assert lib.msm_scalars_mul(h, None, None, None, 0) == 0
    assert lib.msm_scalars_powers(h, None, one, one, 0) == 0
    assert lib.msm_scalars_inner(h, None, None, 0, out) == 0 and bytes(out) == bytes(32)
    assert f.read(a, 5) == A
    # download returns what upload wrote: whole buffers, odd lengths, from an offset
    data = bytes((i * 37 + 11) & 0xFF for i in range(32 * 321 + 13))
    p = ctx.device_alloc(len(data))
    f.bufs.append(p)
    ctx.device_upload(p, data)
    assert ctx.device_download(p, len(data)) == data
    assert ctx.device_download(p + 45, 1001) == data[45:1046]
    assert ctx.device_download(p, 0) == b""


# ---------------------------------------------------------------------------------------------- 8: an inner-product argument

def test_inner_product_argument_end_to_end(f7):
    """Ten rounds over n = 1 024 generators G_i = g_i G with known logs, a random vector a and b = powers(z) made on the device.
    Each round takes L = <a_lo, G_hi>, R = <a_hi, G_lo>, cL = <a_lo, b_hi>, cR = <a_hi, b_lo>, then folds a' = u a_lo + u^-1 a_hi,
    b' = u^-1 b_lo + u b_hi, G' = u^-1 G_lo + u G_hi, and checks <a', G'> = P + u^2 L + u^-2 R and <a', b'> = v + u^2 cL + u^-2 cR.
    Points are compared through their logs (cv.scale_g); the host follows the vectors in integers for that check only."""
    f, cv, q, ctx, n = f7, f7.cv, f7.q, f7.ctx, 1024
    work = ctx.pointset_create()
    try:
        g = O.scalars_from_bytes(ctx.generate_points(n, seed=1502, want_scalars=True))
        a_sh = _ints(f"{f.name}/ipa/a", n, q)
        z = _ints(f"{f.name}/ipa/z", 1, q)[0]
        a, b = f.vector(a_sh), f.vector(n)
        ctx.scalars_powers(b, z, n)
        b_sh = [pow(z, i, q) for i in range(n)]
        assert f.read(b, n) == b_sh

        def dot(u, v):
            return sum(s * t for s, t in zip(u, v)) % q

        P_log, v = dot(a_sh, g), ctx.scalars_inner(a, b, n)
        assert v == dot(a_sh, b_sh)
        got, _ = ctx.run_device(a, n)
        assert f.point(got) == cv.scale_g(P_log)
        us = [w or 2 for w in _ints(f"{f.name}/ipa/u", 10, q)]
        m = n
        for u in us:
            h = m // 2
            ui = pow(u, -1, q)
            L, _ = ctx.run_device(a, h, point_lo=h)
            R, _ = ctx.run_device(a + 32 * h, h)
            cL, cR = ctx.scalars_inner(a, b + 32 * h, h), ctx.scalars_inner(a + 32 * h, b, h)
            assert ctx.fold_scalars(a, m, u, ui) == h and ctx.fold_scalars(b, m, ui, u) == h
            assert ctx.fold_points(ui, u) == h
            # the check, in integers mod q
            L_log, R_log = dot(a_sh[:h], g[h:m]), dot(a_sh[h:m], g[:h])
            assert f.point(L) == cv.scale_g(L_log) and f.point(R) == cv.scale_g(R_log), (f.name, m)
            assert cL == dot(a_sh[:h], b_sh[h:m]) and cR == dot(a_sh[h:m], b_sh[:h]), (f.name, m)
            a_sh = [(u * a_sh[i] + ui * a_sh[h + i]) % q for i in range(h)]
            b_sh = [(ui * b_sh[i] + u * b_sh[h + i]) % q for i in range(h)]
            g = [(ui * g[i] + u * g[h + i]) % q for i in range(h)]
            P_log = (P_log + u * u * L_log + ui * ui * R_log) % q
            v = (v + u * u * cL + ui * ui * cR) % q
            got, _ = ctx.run_device(a, h)                       # <a', G'> over the folded vector and the folded set
            assert f.point(got) == cv.scale_g(P_log), (f.name, m)
            assert ctx.scalars_inner(a, b, h) == v, (f.name, m)
            m = h
        assert m == 1 and ctx.pointset_size() == 1
        assert f.read(a, 1) == a_sh and f.read(b, 1) == b_sh and v == a_sh[0] * b_sh[0] % q
        assert P_log == a_sh[0] * g[0] % q
    finally:
        ctx.pointset_select(0)
        ctx.pointset_destroy(work)
