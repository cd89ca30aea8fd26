"""msm_scalars_scan, msm_scalars_inverse and msm_scalars_div_linear on the GPU, bit for bit against Python integers mod q.  `-m gpu`.

Every vector sits at an odd 32-byte offset inside its allocation with sentinel elements before and after, which are checked after
every call; inputs carry q, q + 1, 2^256 - 1 and 0 among the random residues.  Sizes come from the library's own tile constants
(tests/csrc/scans_host.hip), and every scan asserts the levels it ran (msm_test_last_scan_plan).  The arithmetic is exact: no
tolerances."""
import ctypes
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import degenerate_inputs as D  # noqa: E402
import operator_fixture as F  # noqa: E402
from host_lib import host_library  # noqa: E402
from operator_fixture import SENTINEL, TOP, OperatorFixture, to_bytes  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

THREE = ("bls377", "ed377", "pallas")
SMALL = (1, 63, 64, 65, 255, 256, 257, 511, 513)


def _ints(tag, n, bound):
    return O.prng_ints(f"scans/{tag}", n, bound)


def _start(n):
    """where the special elements begin: a vector of up to three has one too"""
    return 3 if n > 3 else 0


def mixed(cv, tag, n):
    return F.mixed("scans", cv, tag, n, start=_start(n))


def unit_mixed(cv, tag, n):
    """n elements with residues other than 0, q + 1 and 2^256 - 1 among them: a product scan that stays away from 0"""
    q = cv.q
    vals = [v + 1 for v in _ints(f"{cv.name}/{tag}", n, q - 1)]
    return F.with_specials(vals, (q + 1, TOP if TOP % q else 1), _start(n))


def tiled(base, n):
    return [base[i % len(base)] for i in range(n)]


def plan(n, tile_log):
    levels = []
    while n:
        n = -(-n >> tile_log)
        levels.append(n)
        if n == 1:
            break
    return levels


def scan_ref(vals, q, op, exclusive, init):
    """(dst, total) of msm_scalars_scan"""
    acc = (0 if op == "sum" else 1) if init is None else init
    out = []
    for v in vals:
        if exclusive:
            out.append(acc)
        acc = (acc + v) % q if op == "sum" else acc * v % q
        if not exclusive:
            out.append(acc)
    return out, acc


def div_ref(vals, q, z):
    """(dst, remainder) of msm_scalars_div_linear: synthetic division from the top coefficient down"""
    out, acc = [0] * len(vals), 0
    for j in range(len(vals) - 1, -1, -1):
        out[j] = acc
        acc = (acc * z + vals[j]) % q
    return out, acc


class Fix(OperatorFixture):
    def __init__(self, name):
        super().__init__(name)
        self.tile_log = None

    def last_plan(self):
        return self.last("msm_test_last_scan_plan", 8)

    def set_tile_log(self, t, default):
        """t = 0: the default; the plan of later calls is checked against the tile in force"""
        self.set("msm_test_set_scan_tile_log", t)
        self.tile_log = t or default


@pytest.fixture(scope="module", params=D.NAMES)
def f7(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module", params=THREE)
def f3(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module", params=["bls377", "pallas"])
def f2(request):
    f = Fix(request.param)
    yield f
    f.close()


@pytest.fixture(scope="module")
def consts():
    L = host_library("scans_host")
    return {"default": L.scans_default_tile_log(), "min": L.scans_min_tile_log(), "block": L.scans_block(), "inv_e": L.scans_inverse_e()}


def big_shapes(consts):
    """(tile_log or 0 for the default, n): three levels at the smallest tile, and the default tile's edges"""
    t, T = consts["min"], 1 << consts["min"]
    D_ = 1 << consts["default"]
    return [(t, T * T - 1), (t, T * T), (t, T * T + 1), (0, D_ - 1), (0, D_), (0, D_ + 1), (0, 3 * D_ + 77)]


def check_scan(f, a, vals, op, exclusive, init, dst=None):
    n = len(vals)
    d = f.vector(n) if dst is None else dst
    total = f.ctx.scalars_scan(d, a, n, op, exclusive, init)
    exp, exp_total = scan_ref(vals, f.q, op, exclusive, init)
    assert f.last_plan() == plan(n, f.tile_log), (f.name, n)
    assert total == exp_total, (f.name, n, op, exclusive, init)
    assert f.read(d, n) == exp, (f.name, n, op, exclusive, init)
    assert f.fenced(d, n) and f.fenced(a, n), (f.name, n, op)
    if dst is None:
        f.free(d)


# ---------------------------------------------------------------------------------------------- 1: scans

def test_scan_small_shapes_on_every_curve(f7, consts):
    f, q = f7, f7.q
    f.set_tile_log(consts["min"], consts["default"])
    rnd = _ints(f"{f.name}/init", 1, q)[0]
    for n in SMALL:
        for op in ("sum", "product"):
            vals = mixed(f.cv, f"small/{n}", n) if op == "sum" else unit_mixed(f.cv, f"small/{n}", n)
            a, d = f.vector(vals), f.vector(n)
            for exclusive in (False, True):
                for init in (None, 1, q - 1, rnd):
                    check_scan(f, a, vals, op, exclusive, init, dst=d)
            assert f.read(a, n) == vals                      # the source is left alone
            check_scan(f, a, vals, op, True, rnd, dst=a)     # in place
            f.free(a, d)
    # a product over the mixed pattern: it meets q at element 3 and stays 0 from there
    vals = mixed(f.cv, "small/zeroing", 65)
    a = f.vector(vals)
    check_scan(f, a, vals, "product", False, None)
    f.free(a)


def test_scan_tile_edges_and_three_levels(f3, consts):
    f, q = f3, f3.q
    rnd = _ints(f"{f.name}/init/big", 1, q)[0]
    for tile_log, n in big_shapes(consts):
        f.set_tile_log(tile_log, consts["default"])
        for op, base in (("sum", mixed(f.cv, "big", 4093)), ("product", unit_mixed(f.cv, "big", 4093))):
            vals = tiled(base, n)
            a = f.vector(vals)
            check_scan(f, a, vals, op, False, None)
            check_scan(f, a, vals, op, True, rnd)
            check_scan(f, a, vals, op, False, rnd, dst=a)
            f.free(a)
    T = 1 << consts["min"]
    f.set_tile_log(consts["min"], consts["default"])
    assert plan(T * T + 1, consts["min"]) == [T + 1, 2, 1]   # what the three-level cases asserted through check_scan


def test_product_scan_with_one_zero_residue(f3, consts):
    """one element of residue 0 at the last place of a tile, the first place of a tile and either side of a level-2 boundary:
    everything from it on is 0, everything before it unchanged"""
    f, q = f3, f3.q
    t = consts["min"]
    T = 1 << t
    n = T * T + 5
    f.set_tile_log(t, consts["default"])
    base = tiled(unit_mixed(f.cv, "zero", 4093), n)
    clean, _ = scan_ref(base, q, "product", False, None)
    d = f.vector(n)
    for pos in (T - 1, T, T * T - 1, T * T):
        for zero in (0, q):
            vals = list(base)
            vals[pos] = zero
            a = f.vector(vals)
            total = f.ctx.scalars_scan(d, a, n, "product")
            assert f.last_plan() == [T + 1, 2, 1]
            got = f.read(d, n)
            assert got[:pos] == clean[:pos], (f.name, pos, zero)
            assert got[pos:] == [0] * (n - pos) and total == 0, (f.name, pos, zero)
            assert f.fenced(d, n)
            f.free(a)
    f.free(d)


def test_results_do_not_depend_on_the_tile(f3, consts):
    f, q = f3, f3.q
    T = 1 << consts["min"]
    z = _ints(f"{f.name}/tile/z", 1, q)[0]
    for n in (3 * (1 << consts["default"]) + 77, T * T + 1):
        sums, prods = tiled(mixed(f.cv, "tile", 4093), n), tiled(unit_mixed(f.cv, "tile", 4093), n)
        a, b, d = f.vector(sums), f.vector(prods), f.vector(n)
        seen = []
        for tile_log in range(consts["min"], consts["default"] + 1):
            f.set_tile_log(tile_log if tile_log != consts["default"] else 0, consts["default"])
            out = []
            for call in (lambda: f.ctx.scalars_scan(d, a, n, "sum", True), lambda: f.ctx.scalars_scan(d, b, n, "product"),
                         lambda: f.ctx.scalars_div_linear(d, a, n, z)):
                out.append((call(), f.raw(d, n)))
                assert f.last_plan() == plan(n, f.tile_log)
            seen.append(out)
        assert all(s == seen[0] for s in seen[1:]), (f.name, n)
        assert seen[0][2] == (div_ref(sums, q, z)[1], to_bytes(div_ref(sums, q, z)[0]))
        f.free(a, b, d)


# ---------------------------------------------------------------------------------------------- 2: the inverse

def check_inverse(f, vals, in_place=False):
    q, n = f.q, len(vals)
    a = f.vector(vals)
    d = a if in_place else f.vector(n)
    zeros = f.ctx.scalars_inverse(d, a, n)
    assert f.read(d, n) == [pow(v % q, q - 2, q) for v in vals], (f.name, n)
    assert zeros == sum(1 for v in vals if v % q == 0), (f.name, n)
    assert f.fenced(d, n) and f.fenced(a, n)
    if not in_place:
        assert f.read(a, n) == vals
        f.free(d)
    f.free(a)


def test_inverse(f7, consts):
    f, q = f7, f7.q
    per_block = consts["inv_e"] * consts["block"]
    for n in (1, 63, 257, 513, per_block - 1, per_block, per_block + 1, 3 * per_block + 77):
        vals = mixed(f.cv, f"inv/{n}", n)
        if n > 20:
            vals[11], vals[n - 2] = 2 * q, (TOP // q) * q
        check_inverse(f, vals)
        check_inverse(f, vals, in_place=True)
    for n in (1, 65, per_block + 1):
        check_inverse(f, [0] * n)
        check_inverse(f, [q] * n, in_place=True)
        check_inverse(f, [1] * n)


# ---------------------------------------------------------------------------------------------- 3: division by X - z

def check_div(f, vals, z, in_place):
    q, n, ctx = f.q, len(vals), f.ctx
    a = f.vector(vals)
    d = a if in_place else f.vector(n)
    # the remainder by the existing entry points first: <a, powers(z)>
    pw = f.vector(n)
    ctx.scalars_powers(pw, z, n)
    by_inner = ctx.scalars_inner(a, pw, n)
    rem = ctx.scalars_div_linear(d, a, n, z)
    exp, exp_rem = div_ref(vals, q, z)
    assert f.last_plan() == plan(n, f.tile_log), (f.name, n)
    assert rem == exp_rem == by_inner, (f.name, n, z)
    assert f.read(d, n) == exp, (f.name, n, z, in_place)
    assert f.fenced(d, n) and f.fenced(a, n)
    if not in_place:
        assert f.read(a, n) == vals
        f.free(d)
    f.free(a, pw)


def test_div_linear_small_shapes_on_every_curve(f7, consts):
    f, q = f7, f7.q
    f.set_tile_log(consts["min"], consts["default"])
    rnd = _ints(f"{f.name}/z", 1, q)[0]
    for n in SMALL:
        vals = mixed(f.cv, f"div/{n}", n)
        for i, z in enumerate((0, 1, q - 1, rnd)):
            check_div(f, vals, z, in_place=bool((i + n) % 2))
        check_div(f, vals, rnd, in_place=True)
        check_div(f, vals, rnd, in_place=False)


def test_div_linear_tile_edges_and_three_levels(f3, consts):
    f, q = f3, f3.q
    rnd = _ints(f"{f.name}/z/big", 1, q)[0]
    base = mixed(f.cv, "div/big", 4093)
    for tile_log, n in big_shapes(consts):
        f.set_tile_log(tile_log, consts["default"])
        vals = tiled(base, n)
        check_div(f, vals, rnd, in_place=False)
        check_div(f, vals, q - 1, in_place=True)
    f.set_tile_log(0, consts["default"])
    for z in (0, 1):
        check_div(f, tiled(base, 3 * (1 << consts["default"]) + 77), z, in_place=False)


def test_kzg_witness_commitment(f2, consts):
    """coefficients -> div_linear -> msm_run over the device quotient where it lies, at 321 generated points: the point is
    (sum q_j g_j) G by the known discrete logs"""
    f, cv, q, ctx = f2, f2.cv, f2.q, f2.ctx
    n = 321
    f.set_tile_log(consts["min"], consts["default"])
    logs = O.scalars_from_bytes(ctx.generate_points(n, seed=1701, want_scalars=True))
    vals = mixed(cv, "kzg", n)
    z = _ints(f"{f.name}/kzg/z", 1, q)[0]
    a = f.vector(vals)
    rem = ctx.scalars_div_linear(a, a, n, z)
    quo, exp_rem = div_ref(vals, q, z)
    assert rem == exp_rem and f.read(a, n) == quo and f.last_plan() == [2, 1]
    # (X - z) q(X) + a(z) = a(X) at a point of its own
    x = _ints(f"{f.name}/kzg/x", 1, q)[0]
    assert ((x - z) * sum(c * pow(x, j, q) for j, c in enumerate(quo)) + rem) % q == sum(c * pow(x, j, q) for j, c in enumerate(vals)) % q
    got, _ = ctx.run_device(a, n)
    assert f.point(got) == cv.scale_g(sum(c * g for c, g in zip(quo, logs)) % q)
    f.free(a)


def test_empty_and_single_element_calls(f7, consts):
    f, q, ctx = f7, f7.q, f7.ctx
    f.set_tile_log(0, consts["default"])
    d = f.vector(2)
    assert ctx.scalars_scan(d, d, 0, "sum") == 0 and f.last_plan() == []
    assert ctx.scalars_scan(d, d, 0, "product") == 1
    assert ctx.scalars_scan(d, d, 0, "product", init=q - 1) == q - 1
    assert ctx.scalars_scan(0, 0, 0, "sum", init=5) == 5          # null vectors with n == 0
    assert ctx.scalars_inverse(d, d, 0) == 0
    assert ctx.scalars_div_linear(d, d, 0, 7) == 0 and f.last_plan() == []
    assert f.raw(d, 2) == SENTINEL * 2
    a = f.vector([q + 5])
    assert ctx.scalars_div_linear(d, a, 1, 3) == 5 and f.last_plan() == [1]
    assert f.raw(d, 2) == bytes(32) + SENTINEL
    f.free(a, d)


# ---------------------------------------------------------------------------------------------- 4: refusals

def test_every_refusal_leaves_dst_and_the_context_alone(f7, consts):
    from montgomery_amd import _lib
    from montgomery_amd._lib import MSM_ERR_ARG, MSM_ERR_SCALAR, MsmError

    f, q, ctx = f7, f7.q, f7.ctx
    f.set_tile_log(0, consts["default"])
    n = 40
    vals = mixed(f.cv, "refuse", n)
    a, d = f.vector(vals + vals), f.vector(n)
    out = (ctypes.c_uint8 * 32)()

    def still_good():
        assert f.raw(d, n) == SENTINEL * n and f.read(a, 2 * n) == vals + vals and f.fenced(d, n)
        t = f.vector(n)
        assert ctx.scalars_scan(t, a, n, "sum") == sum(vals) % q
        f.free(t)

    def refused(code, call, *args, **kw):
        with pytest.raises(MsmError) as e:
            call(*args, **kw)
        assert e.value.code == code, (call.__name__, args, kw)
        if call is not inverse:
            assert f.last_plan() == []                        # a refused scan or division reports no plan
        still_good()

    def inverse(dst, src, m):
        return ctx.scalars_inverse(dst, src, m)

    calls = (lambda dst, src, m: ctx.scalars_scan(dst, src, m, "sum"), lambda dst, src, m: ctx.scalars_scan(dst, src, m, "product", True),
             inverse, lambda dst, src, m: ctx.scalars_div_linear(dst, src, m, 3))
    for call in calls:
        refused(MSM_ERR_ARG, call, a + 32, a, n)              # partial overlap, either way round
        refused(MSM_ERR_ARG, call, a, a + 32 * (n - 1), n)
        refused(MSM_ERR_ARG, call, d + 8, a, n - 1)           # misaligned dst, misaligned source
        refused(MSM_ERR_ARG, call, d, a + 4, n)
        refused(MSM_ERR_ARG, call, 0, a, n)                   # null pointers with n > 0
        refused(MSM_ERR_ARG, call, d, 0, n)
        refused(MSM_ERR_ARG, call, d, a, 1 << 30)
    refused(MSM_ERR_SCALAR, ctx.scalars_scan, d, a, n, "sum", False, q)
    refused(MSM_ERR_SCALAR, ctx.scalars_scan, d, a, n, "product", True, TOP)
    refused(MSM_ERR_SCALAR, ctx.scalars_scan, d, a, 0, "sum", False, q)           # checked for an empty vector too
    refused(MSM_ERR_SCALAR, ctx.scalars_div_linear, d, a, n, q)
    refused(MSM_ERR_SCALAR, ctx.scalars_div_linear, d, a, n, TOP)
    with pytest.raises(MsmError):
        ctx.scalars_scan(d, a, n, "horner")                   # (the facade's own refusal: the library is not called)
    still_good()
    vp = ctypes.c_void_p
    for op, flags in ((2, 0), (-1, 0), (_lib.SCAN_SUM, 2), (_lib.SCAN_PRODUCT, _lib.SCAN_EXCLUSIVE | 0x80000000)):
        assert ctx._lib.msm_scalars_scan(ctx._h, vp(d), vp(a), n, op, flags, None, out) == MSM_ERR_ARG, (op, flags)
        assert f.last_plan() == []
        still_good()
    assert ctx._lib.msm_scalars_div_linear(ctx._h, vp(d), vp(a), n, None, out) == MSM_ERR_ARG      # null z
    still_good()
    for t in (1, 7, consts["default"] + 1, -1):
        assert ctx._lib.msm_test_set_scan_tile_log(ctx._h, t) == MSM_ERR_ARG
    f.free(a, d)


def test_device_list_contexts_are_refused():
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError
    from montgomery_amd.api import MsmContext

    multi = MsmContext(D.CURVE_TABLE["bls377"].cid, devices=[0, 0])
    try:
        p = multi.device_alloc(256)
        multi.device_upload(p, SENTINEL * 8)
        for call in (lambda: multi.scalars_scan(p + 128, p, 2), lambda: multi.scalars_inverse(p + 128, p, 2),
                     lambda: multi.scalars_div_linear(p + 128, p, 2, 3)):
            with pytest.raises(MsmError) as e:
                call()
            assert e.value.code == MSM_ERR_ARG
        assert multi._lib.msm_test_set_scan_tile_log(multi._h, 8) == MSM_ERR_ARG
        assert multi._lib.msm_test_last_scan_plan(multi._h, None, 0) == -1
        assert multi.device_download(p, 256) == SENTINEL * 8
        multi.device_free(p)
    finally:
        multi.close()
