"""Shared window tables (msm_tables.hip): from the size at which a run on tables is two window groups, the point set holds
T = ceil(K / 2) tables 2^(c j) P and BOTH groups gather from them, each relative to its own first window; the host supplies the
weight 2^(c wpg) between the groups' sums (window_sums_once).  The sizes here are the smallest at which two groups run on tables:
2^21 points on BLS12-377, 2^20 on Ed-on-BLS12-377.  Results are group elements: every run on shared tables must equal the plain
path bit for bit.  Needs an MI355X: `-m gpu`."""
import pytest

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

C = O.BLS12_377
N = 1 << 21


@pytest.fixture(scope="module")
def set_2p21(gpu_ctx, c_oracle):
    """2^21 generated points with known discrete logs, uniform scalars in device memory, and the expected sum -- computed once."""
    a = gpu_ctx.generate_points(N, seed=5021, want_scalars=True, raw=True)
    dev, s = gpu_ctx.generate_scalars(N, seed=6021, to_host=True, raw=True)
    exp = O.aff_scale(c_oracle.dot_mod(a, s, N, C.q), (C.gx, C.gy), C.p)
    return dev, exp


def test_default_plan_holds_four_tables_for_seven_windows(gpu_ctx, set_2p21):
    """c = 18, K = 7: the groups are windows [0, 4) and [4, 7), both through tables 0 .. 3."""
    dev, exp = set_2p21
    res, info = gpu_ctx.run_device(dev, N)
    assert info["tables"] and (info["c"], info["K"]) == gpu_ctx.plan(N) == (18, 7), info
    assert gpu_ctx.tables_info() == (18, 7, 4 * N * 256)
    assert res.as_tuple() == exp
    plain, pinfo = gpu_ctx.run_device(dev, N, no_tables=True)
    assert not pinfo["tables"] and plain.as_tuple() == exp
    ser, sinfo = gpu_ctx.run_device(dev, N, serial=True)
    assert sinfo["tables"] and ser.as_tuple() == exp


def test_headline_plan_shape_three_tables_for_six_windows(gpu_ctx, set_2p21):
    """precompute(c = 21): K = 6, T = 3 -- the plan of 2^26 points, the folded top window in the second group.  Constant scalars
    put all entries of a group into one or two buckets; 0 and 1 leave the upper group's sum the identity, which must survive the
    2^(3 c) weight."""
    dev, exp = set_2p21
    assert gpu_ctx.precompute(N, c=21) == (21, 6, 3 * N * 256)
    got, info = gpu_ctx.run_device(dev, N, c=21)
    want, winfo = gpu_ctx.run_device(dev, N, c=21, no_tables=True)
    assert info["tables"] and not winfo["tables"] and (info["c"], info["K"]) == (winfo["c"], winfo["K"]) == (21, 6)
    assert got.as_tuple() == want.as_tuple() == exp
    for val in (C.q - 1, 1, (1 << 252) - 1, 0):
        const = val.to_bytes(32, "little") * N
        a, ia = gpu_ctx.run(const, c=21)
        b, ib = gpu_ctx.run(const, c=21, no_tables=True)
        assert ia["tables"] and not ib["tables"] and a.as_tuple() == b.as_tuple(), hex(val)


def test_merged_window_shards_wider_than_the_tables(gpu_ctx, set_2p21):
    """msm_window_sums(merged_sums) over a window range of a set that holds T = 4 tables: the six windows [1, 7) are more than
    the set has tables, the three windows [2, 5) start at neither group's first window of a full run.  Both ranges are cut into
    two groups that read the tables from table 0, and the merged sum, relative to the range's first window, comes back in its
    first slot."""
    from montgomery_amd import _lib
    from montgomery_amd.distributed import combine_host

    dev, _ = set_2p21
    c, K = 18, 7
    assert gpu_ctx.precompute(N, c=c) == (c, K, 4 * N * 256)
    ref = b"".join(gpu_ctx.window_sums(dev, N, k, k + 1, c=c, on_device=True)[0] for k in range(K))
    want = combine_host(ref, K, c, _lib.CURVE_BLS12_377_G1)
    ident = lambda part, j: part[144 * j + 96 : 144 * j + 144] == bytes(48)       # Z = 0
    for lo, hi in ((1, 7), (2, 5)):
        pw, iw = gpu_ctx.window_sums(dev, N, lo, hi, c=c, on_device=True, merged=True)
        assert iw["tables"] and not ident(pw, 0) and all(ident(pw, j) for j in range(1, hi - lo)), (lo, hi)
        mixed = ref[: 144 * lo] + pw + ref[144 * hi:]
        assert combine_host(mixed, K, c, _lib.CURVE_BLS12_377_G1) == want, (lo, hi)
    gpu_ctx.set_points(O.points_to_bytes([(C.gx, C.gy)], 48))   # give the rows and tables back


def test_edwards_shares_eight_tables_among_fifteen_windows():
    """Ed-on-BLS12-377 at 2^20 points: c = 17, K = 15, groups of 8 + 7 windows over T = 8 tables.  The row size comes from a
    one-group set of the same context."""
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    ctx = MsmContext(_lib.CURVE_ED_ON_BLS12_377)
    try:
        m = 1 << 14
        ctx.generate_points(m, seed=81)
        dev, _ = ctx.generate_scalars(m, seed=82)
        _, i1 = ctx.run_device(dev, m)
        c1, K1, b1 = ctx.tables_info()
        assert i1["tables"] and K1 >= 2 and b1 % (K1 * m) == 0
        row = b1 // (K1 * m)
        n = 1 << 20
        ctx.generate_points(n, seed=83)
        dev, _ = ctx.generate_scalars(n, seed=84)
        got, it = ctx.run_device(dev, n)
        plain, ip = ctx.run_device(dev, n, no_tables=True)
        assert it["tables"] and not ip["tables"] and (got.x, got.y) == (plain.x, plain.y)
        assert ctx.tables_info() == (17, 15, 8 * n * row)
    finally:
        ctx.close()
