"""Every device buffer goes back with its owner: the count of live buffers (msm_test_live_buffers) around whole contexts, around
single owners inside one, and around a call that is refused half way.  `-m gpu`.

The counter is the process's, and the session's other contexts may be alive and idle: every reading is a difference against a
baseline taken at the start of the test, and the tests use contexts of their own."""
import pytest

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

BLS377, ED377 = 0, 1
N_POINTS = 4096 + 77


def live():
    from montgomery_amd.api import MsmContext

    return MsmContext.test_live_buffers()


def scalars_of(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def populate(ctx):
    """One of everything a context can own; returns the ids of what the caller gives back by hand."""
    n = N_POINTS
    # set 0: tables of the whole set, which need a bigger row buffer than the rows alone
    ctx.generate_points(n, seed=11)
    c, K, table_bytes = ctx.precompute()
    assert K >= 2 and table_bytes > n * 2 * ctx.coord_bytes and ctx.tables_range() == (0, n)
    # a second set: tables of a range of its points, in a buffer of their own
    ranged = ctx.pointset_create()
    ctx.generate_points(n, seed=12)
    ctx.precompute(4096, point_lo=64)
    assert ctx.tables_info()[1] >= 2 and ctx.tables_range() == (64, 4096)
    ctx.pointset_select(0)
    # one MSM from host scalars, one from device scalars: workspaces, the scalar buffer, staging
    dev, host = ctx.generate_scalars(n, seed=13, to_host=True)
    from_host, _ = ctx.run(host)
    from_dev, _ = ctx.run_device(dev, n)
    assert (from_host.x, from_host.y, from_host.isZero) == (from_dev.x, from_dev.y, from_dev.isZero)
    # the operators over resident vectors, each with the buffers it keeps in the context
    a, b = ctx.device_alloc(32 * n), ctx.device_alloc(32 * n)
    log2n = min(10, ctx.scalars_ntt_max_log2n())   # (the scalar field of Ed-on-BLS12-377 has no root of order 2^10)
    ctx.scalars_ntt(a, dev, log2n, shift=5)
    ctx.scalars_scan(a, dev, 1025)
    ctx.scalars_inverse(b, dev, 1025)
    ctx.scalars_sumcheck_round([dev, a], 4, 0)
    ctx.scalars_eq(b, [3, 5, 7, 11])
    # per-row multiples and a linear combination, each into a fresh set
    mul = ctx.pointset_create()
    ctx.points_mul(dev, src=0, count=64, dst=mul)
    base = ctx.pointset_create()
    ctx.points_mul_base(dev, None, count=64, dst=base)
    comb = ctx.pointset_create()
    ctx.points_lincomb(3, 5, src_a=0, src_b=ranged, count=n, dst=comb)
    ctx.pointset_select(0)
    # two matrices; a row of 40 entries lies above the default short_max of 32: the plan of the long rows and their partials exist
    long_row = ctx.matrix_create(3, 64, [0, 2, 42, 43], [0, 1] + list(range(40)) + [7], list(range(1, 44)))
    ones = ctx.matrix_create(2, 64, [0, 1, 3], [5, 0, 63], None)
    ctx.scalars_matvec(long_row, a, dev)
    ctx.scalars_matvec(ones, b, dev)
    return {"matrix": long_row, "alloc": a, "set": base}


@pytest.mark.parametrize("curve", [BLS377, ED377], ids=["bls377", "ed377"])
def test_everything_a_context_owns_comes_back(curve):
    from montgomery_amd.api import MsmContext

    base = live()
    ctx = MsmContext(curve)
    try:
        held = populate(ctx)
        # one matrix: exactly its bytes go back
        before = live()
        matrix_bytes = ctx.matrix_info(held["matrix"])["bytes"]
        ctx.matrix_destroy(held["matrix"])
        after = live()
        assert matrix_bytes > 0 and before[1] - after[1] == matrix_bytes and after[0] < before[0]
        # one allocation, one point set
        ctx.device_free(held["alloc"])
        assert live()[0] == after[0] - 1
        ctx.pointset_destroy(held["set"])
        assert live()[0] == after[0] - 2
        assert live()[0] > base[0] and live()[1] > base[1]
    finally:
        ctx.close()   # with everything else still live
    assert live() == base


def test_create_close_cycles_return_to_the_baseline():
    from montgomery_amd.api import MsmContext

    base = live()
    for cycle in range(3):
        ctx = MsmContext()
        try:
            assert live()[0] > base[0]
            ctx.generate_points(256, seed=21 + cycle)
            dev, _ = ctx.generate_scalars(256, seed=22)
            ctx.run_device(dev, 256)
        finally:
            ctx.close()
        assert live() == base, cycle


def test_a_call_refused_half_way_gives_back_what_it_took():
    """msm_test_batch_add_mode allocates its wire points, its rows and then its planes, 2 * steps * 256 * 96 bytes for one pair:
    with planes of four times the device's memory the third allocation is refused before anything runs, and the first two must
    not stay behind.  One call, made once."""
    import torch

    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext, MsmError

    p = O.BLS12_377.p
    (P, Q), _ = O.random_points_bls377("gpu/lifecycle", 2)
    enc = lambda A: A[0].to_bytes(48, "little") + A[1].to_bytes(48, "little")
    total = torch.cuda.mem_get_info()[1]
    steps = -(-4 * total // (2 * 256 * 96))
    assert 2 * steps * 256 * 96 >= 4 * total and steps < 1 << 32
    ctx = MsmContext()
    try:
        base = live()
        with pytest.raises(MsmError) as refused:
            ctx.test_batch_add_mode(enc(P), enc(Q), 1, steps)
        assert refused.value.code == _lib.MSM_ERR_HIP
        assert live() == base
        assert ctx.test_batch_add_mode(enc(P), enc(Q), 1, 1) == enc(O.aff_add(P, Q, p))
        assert live() == base
    finally:
        ctx.close()


def test_a_device_list_context_comes_back():
    import torch

    from montgomery_amd.api import MsmContext

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    base = live()
    ctx = MsmContext(devices=[0, 1])
    try:
        ctx.generate_points(4096, seed=31)
        dev, host = ctx.generate_scalars(4096, seed=32, to_host=True)
        ctx.run(host)
        assert live()[0] > base[0]
    finally:
        ctx.close()
    assert live() == base
