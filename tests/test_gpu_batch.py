"""msm_run_batch: B MSMs over one resident point set in one call, element by element equal to msm_run.  `-m gpu`."""
import ctypes

import pytest

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ("bls377", "ed377", "bls381", "pallas")


def _ctx(name):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    cid = {"bls377": _lib.CURVE_BLS12_377_G1, "ed377": _lib.CURVE_ED_ON_BLS12_377, "bls381": _lib.CURVE_BLS12_381_G1,
           "pallas": _lib.CURVE_PALLAS}[name]
    return MsmContext(cid)


def _order(name):
    return {"bls377": O.BLS12_377.q, "ed377": O.ED_ON_BLS12_377.q, "bls381": O.BLS12_381.q, "pallas": O.PALLAS.q}[name]


@pytest.fixture(scope="module", params=CURVES)
def cv(request):
    ctx = _ctx(request.param)
    ctx.generate_points(1 << 14, seed=900)
    yield request.param, ctx
    ctx.close()


def _scalars(name, B, n, tag):
    return [O.scalars_to_bytes(O.prng_ints(f"batch/{name}/{tag}/{b}", n, _order(name))) for b in range(B)]


def _check_each(ctx, scalars, got, **kw):
    for s, (res, info) in zip(scalars, got):
        exp, _ = ctx.run(s, **kw)
        assert res == exp


@pytest.mark.parametrize("B", [1, 2, 7, 16])
@pytest.mark.parametrize("n", [1, 100, 1 << 10, 1 << 14])
def test_batch_equals_msm_run(cv, B, n):
    name, ctx = cv
    sc = _scalars(name, B, n, f"{B}/{n}")
    got = ctx.run_batch(sc)
    assert len(got) == B
    _check_each(ctx, sc, got)
    infos = [i for _, i in got]
    assert all(i == infos[0] for i in infos), "the statistics of the whole call go into every element"


@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_batch_device_scalars(cv, n):
    name, ctx = cv
    B = 7
    sc = _scalars(name, B, n, f"dev/{n}")
    ptrs = []
    for s in sc:
        p = ctx.device_alloc(len(s))
        ctx.device_upload(p, s)
        ptrs.append(p)
    try:
        got = ctx.run_batch_device(ptrs, n)
        _check_each(ctx, sc, got)
        assert [r for r, _ in got] == [r for r, _ in ctx.run_batch(sc)]
    finally:
        for p in ptrs:
            ctx.device_free(p)


def test_batch_against_oracle(cv):
    """At a few hundred points the elements also match the CPU oracle."""
    name, ctx = cv
    n, B = 300, 3
    sc = _scalars(name, B, n, "oracle")
    got = ctx.run_batch(sc)
    cb = ctx.coord_bytes
    pts = O.points_from_bytes(ctx.get_points(0, n), cb)
    for s, (res, info) in zip(sc, got):
        ints = O.scalars_from_bytes(s)
        if name == "ed377":
            assert (res.x, res.y) == O.msm_basic_te(ints, pts, c=info["c"])
        else:
            C = {"bls377": O.BLS12_377, "bls381": O.BLS12_381, "pallas": O.PALLAS}[name]
            assert res.as_tuple() == O.msm_batched_affine(ints, pts, C=C, c=info["c"])


def test_batch_edge_elements(cv):
    """An all-zero element, two identical elements, one scalar repeated (heavy buckets), scalars >= q."""
    name, ctx = cv
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    n, q = 1 << 12, _order(name)
    base = _scalars(name, 1, n, "edge")[0]
    zero = bytes(32 * n)
    rep = O.scalars_to_bytes([0x1234567890ABCDEF % q] * n)
    big = O.scalars_to_bytes([(q + 5 + i) % (1 << 256) for i in range(n)])
    sc = [zero, base, base, rep, big]
    got = ctx.run_batch(sc)
    _check_each(ctx, sc, got)
    ident = ctx.run(zero)[0]
    assert got[0][0] == ident
    assert got[1][0] == got[2][0]
    with pytest.raises(MsmError) as e:
        ctx.run_batch(sc, strict=True)
    assert e.value.code == _lib.MSM_ERR_SCALAR
    assert [r for r, _ in ctx.run_batch(sc[:4], strict=True)] == [r for r, _ in got[:4]]


def test_batch_options(cv):
    """n == 0, a point_lo range, an explicit window, no_glv."""
    name, ctx = cv
    sc = _scalars(name, 4, 1000, "opts")
    empty = ctx.run_batch([b""] * 3)
    assert [r for r, _ in empty] == [ctx.run(b"")[0]] * 3
    got = ctx.run_batch_device([0, 0], 0)
    assert len(got) == 2
    for s, (r, _) in zip(sc, ctx.run_batch(sc, point_lo=777)):
        p = ctx.device_alloc(len(s))
        ctx.device_upload(p, s)
        assert r == ctx.run_device(p, 1000, point_lo=777)[0]
        ctx.device_free(p)
    for c in (6, 11, 16):
        got = ctx.run_batch(sc, c=c)
        assert all(i["c"] == c for _, i in got)
        _check_each(ctx, sc, got)
    if name != "ed377":
        got = ctx.run_batch(sc, no_glv=True)
        _check_each(ctx, sc, got, no_glv=True)


def test_batch_bad_arguments():
    from montgomery_amd import _lib
    from montgomery_amd._lib import MsmOpts, MsmResult

    ctx = _ctx("bls377")
    ctx.generate_points(64, seed=3)
    lib = _lib.load()
    s = (ctypes.c_uint8 * (32 * 64))()
    arr = (ctypes.c_void_p * 2)(ctypes.cast(s, ctypes.c_void_p), None)
    res = (MsmResult * 2)()
    for bad in ({"k_hi": 2}, {"bucket_shards": 2}, {"merged_sums": 1}, {"by_window": 1}):
        o = MsmOpts(**bad)
        arr1 = (ctypes.c_void_p * 1)(ctypes.cast(s, ctypes.c_void_p))
        assert lib.msm_run_batch(ctx._h, arr1, 1, 64, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG
    o = MsmOpts()
    assert lib.msm_run_batch(ctx._h, arr, 2, 64, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG   # a null element
    assert lib.msm_run_batch(ctx._h, arr, 0, 64, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG   # B == 0
    assert lib.msm_run_batch(ctx._h, arr, 1, 64, 0, ctypes.byref(o), None) == _lib.MSM_ERR_ARG  # no out
    assert lib.msm_run_batch(ctx._h, arr, 1, 65, 0, ctypes.byref(o), res) == _lib.MSM_ERR_NO_POINTS
    ctx.close()


def test_batch_of_several_groups():
    """Ed-on-BLS12-377, 2^12 x 40: more elements than one window group holds."""
    ctx = _ctx("ed377")
    n = 1 << 12
    ctx.generate_points(n, seed=41)
    sc = _scalars("ed377", 40, n, "groups")
    got = ctx.run_batch(sc)
    _check_each(ctx, sc, got)
    ctx.close()


def test_batch_fallback_region():
    """2^20 x 3 on BLS12-377: the radix-split region, where the call runs element by element."""
    ctx = _ctx("bls377")
    n = 1 << 20
    ctx.generate_points(n, seed=42)
    ptrs = [ctx.device_alloc(32 * n) for _ in range(3)]
    for b, p in enumerate(ptrs):
        ctx.generate_scalars(n, seed=50 + b, into=p)
    got = ctx.run_batch_device(ptrs, n)
    assert got[0][1]["c"] == ctx.run_device(ptrs[0], n)[1]["c"]
    for p, (r, _) in zip(ptrs, got):
        assert r == ctx.run_device(p, n)[0]
    ctx.close()


def test_batch_known_discrete_logs():
    """2^18 x 8 against sum_i s_i a_i G for points P_i = a_i G."""
    from oracle import c_oracle

    C = O.BLS12_377
    ctx = _ctx("bls377")
    n = 1 << 18
    logs = ctx.generate_points(n, seed=43, want_scalars=True)
    host = [ctx.generate_scalars(n, seed=60 + b, to_host=True)[1] for b in range(8)]
    got = ctx.run_batch(host)
    for h, (r, _) in zip(host, got):
        k = c_oracle.dot_mod(logs, h, n, C.q)
        assert r.as_tuple() == O.aff_scale(k, (C.gx, C.gy), C.p)
    ctx.close()


def test_batch_beside_window_tables():
    """On a point set with window tables the batch equals msm_run and leaves the tables as they are."""
    ctx = _ctx("bls377")
    n = 1 << 14
    ctx.generate_points(n, seed=44)
    ctx.precompute()
    before = ctx.tables_info()
    assert before[1] > 0
    sc = _scalars("bls377", 5, n, "tables")
    got = ctx.run_batch(sc)
    assert ctx.tables_info() == before
    for s, (r, _) in zip(sc, got):
        exp, info = ctx.run(s)
        assert info["tables"] and r == exp
    assert ctx.tables_info() == before
    ctx.close()


def test_batch_is_fused():
    """2^14 x 16: the elements share the tree rounds -- fewer rounds than 16 single calls."""
    ctx = _ctx("bls377")
    n = 1 << 14
    ctx.generate_points(n, seed=45)
    sc = _scalars("bls377", 16, n, "fused")
    _, single = ctx.run(sc[0], no_tables=True)
    got = ctx.run_batch(sc)
    assert got[0][1]["rounds"] < 16 * single["rounds"]
    assert not got[0][1]["tables"]
    ctx.close()
