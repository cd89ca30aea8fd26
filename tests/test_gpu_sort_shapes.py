"""The sort's heavy-bin parts and path switches under crafted digits (tests/crafted_digits.py; sort_kernels.h, "Parts of heavy
bins"; msm_sort.hip).  Uniform, repeated and prover-like scalars leave most of that code untouched: a multi-part bin with
densely populated buckets, bins of exactly part_len, part_len + 1 and k * part_len records, several multi-part bins in one
window, heavy first and last bins, a heavy short top window, the hand-over of the pair list between parts, the radix split
either side of its one-level fallback and with one busy coarse bin.  Every case checks

  1. the affine result, bit for bit, against (sum s_i a_i) G for generated points P_i = a_i G,
  2. info["n_pairs_algo"] against the crafted histogram, exactly,
  3. info["max_bucket"]: the crafted maximum in the slot form and on the other sort paths; in the pair form k_part_scan
     reports 2 * sum of ceil(n_part / 2) over the parts of a bucket's bin, so true_max <= max_bucket <= the largest of
     size + parts of the bucket's bin,
  4. info["c"], info["K"], info["tables"].

The shapes are the smallest that reach each path, derived from msm_sort.hip (crafted_digits.Geometry restates it, and every
test asserts the path it means to take, and that the library reports the same: msm_test_last_sort_paths).  The pair form needs more than 2^23 table rows AND logG >= 2: at 2^23 + 4096 points
the mean bucket of a 21-bit plan is 16 (logG = 1, slot form), so the pair-form cases run seven 18-bit windows there.
run_batch is fused into the one-level sort only (msm_batch.hip refuses any other path), so it has no case here.
Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import crafted_digits as D
from degenerate_inputs import CURVE_TABLE

pytestmark = pytest.mark.gpu

_resident = {}      # what this module last generated on the shared context: (n, seed) -> the a_i


def ids(cases):
    return [cs.id for cs in cases]


def points(ctx, n, seed=1700):
    """n generated points on ctx, generated once per (n, seed) run of tests: the a_i as a ctypes array."""
    key = (id(ctx), n, seed)
    if key not in _resident or ctx.n_points != n:
        _resident.clear()
        _resident[key] = ctx.generate_points(n, seed=seed, want_scalars=True, raw=True)
    return _resident[key]


def as_c(s_np):
    """The n x 32 byte array as a ctypes array over the same memory (no copy of a 256 MB buffer)."""
    return (C.c_uint8 * s_np.size).from_buffer(s_np.reshape(-1))


def expected_point(c_oracle, cv, a, s_np, n):
    return cv.scale_g(c_oracle.dot_mod(a, as_c(s_np), n, cv.q))


def bucket_bounds(cr, keep=None):
    """(pair additions, smallest and largest max_bucket the call may report) from the crafted digits and the sort's cuts."""
    pl = cr.plan
    hists, largest, pairs = cr.stats(keep)
    groups = pl.window_groups(cr.n, cr.tables)
    upper = largest
    for gi, (lo, hi) in enumerate(groups):
        geo = D.Geometry(pl, cr.n, lo, hi, cr.tables)
        if geo.path != "pairs":
            continue
        for kk, h in enumerate([hists[gi]] if cr.tables else hists[lo:hi]):
            fb = geo.fb[kk]
            if fb == 0:
                continue
            sizes = h[1:].astype(np.int64)
            sizes = np.concatenate([sizes, np.zeros(-len(sizes) % (1 << fb), dtype=np.int64)]).reshape(-1, 1 << fb)
            rec = sizes.sum(axis=1)
            parts = np.where(rec > geo.part_len, -(-rec // geo.part_len), 0)
            upper = max(upper, int((sizes.max(axis=1) + parts).max()))
    return pairs, largest, upper


def check_info(cr, info, c, tables=False, keep=None):
    pairs, lo, hi = bucket_bounds(cr, keep)
    print(cr.name, {k: info[k] for k in ("c", "K", "tables", "n_pairs_algo", "max_bucket")}, "expected", pairs, lo, hi)
    assert (info["c"], info["K"], info["tables"]) == (c, cr.plan.K, tables), info
    assert info["n_pairs_algo"] == pairs, (info, pairs)
    assert lo <= info["max_bucket"] <= hi, (info, lo, hi)


def paths(cr):
    return [D.Geometry(cr.plan, cr.n, lo, hi, cr.tables).path for lo, hi in cr.plan.window_groups(cr.n, cr.tables)]


def took(ctx, cr):
    """The prediction against the library's own report of the call just made (msm_test_last_sort_paths)."""
    got = ctx.test_last_sort_paths()
    assert got == paths(cr), (cr.name, got, paths(cr))


# ---------------------------------------------------------------------------------------------- bin split, slot form

@pytest.mark.parametrize("cs", D.SLOT_CASES, ids=ids(D.SLOT_CASES))
def test_bin_split_slot_form(gpu_ctx, c_oracle, cs):
    """k_bin_count, k_part_scan (entries) and k_bin_slots: BLS12-377, explicit window, plain path, 2^18 and 2^18 + 77 points."""
    cr = cs.make()
    assert paths(cr) == ["slots"]
    a = points(gpu_ctx, cs.n)
    s = cr.scalars()
    res, info = gpu_ctx.run(s.tobytes(), c=cs.c, no_tables=True)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], a, s, cs.n), (cs.id, info)
    check_info(cr, info, cs.c)


# ---------------------------------------------------------------------------------------------- bin split, pair form

@pytest.fixture(scope="module")
def big(gpu_ctx):
    """The points of the pair-form cases and one device scalar buffer for all of them."""
    n = max(D.PAIR_N, D.TABLES_N)
    dev = gpu_ctx.device_alloc(32 * n)
    yield dev
    gpu_ctx.device_free(dev)


@pytest.mark.parametrize("cs", D.PAIR_CASES, ids=ids(D.PAIR_CASES))
def test_bin_split_pair_form(gpu_ctx, c_oracle, big, cs):
    """k_part_scan (elements, part_pair_off) and k_bin_pairs: more than 2^23 rows, both window groups in the pair form."""
    cr = cs.make()
    assert paths(cr) == ["pairs", "pairs"]
    a = points(gpu_ctx, cs.n)
    s = cr.scalars()
    gpu_ctx.device_upload(big, as_c(s))
    res, info = gpu_ctx.run_device(big, cs.n, c=cs.c, no_tables=True)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], a, s, cs.n), (cs.id, info)
    check_info(cr, info, cs.c)


@pytest.mark.parametrize("cs", D.TABLES_CASES, ids=ids(D.TABLES_CASES))
def test_bin_split_on_window_tables(gpu_ctx, c_oracle, big, cs):
    """The default plan on window tables at the smallest n whose first group's merged window exceeds 2^23 rows (four shared
    tables): that group takes the pair form, the second (three windows) the slot form; a bin is heavy across the merged window."""
    cr = cs.make()
    assert paths(cr) == ["pairs", "slots"]
    a = points(gpu_ctx, cs.n)
    assert gpu_ctx.plan(cs.n) == (cs.c, cr.plan.K)
    s = cr.scalars()
    gpu_ctx.device_upload(big, as_c(s))
    gpu_ctx.precompute(cs.n)
    res, info = gpu_ctx.run_device(big, cs.n)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], a, s, cs.n), (cs.id, info)
    check_info(cr, info, cs.c, tables=True)


# ---------------------------------------------------------------------------------------------- radix split

@pytest.mark.parametrize("cs", D.RADIX_CASES, ids=ids(D.RADIX_CASES))
def test_radix_split_and_its_fallbacks(gpu_ctx, c_oracle, cs):
    """c = 16 at 2^20 points: the largest bucket either side of the `heavy` fallback to the one-level scatter (2^17 entries),
    one coarse bin with half of a window's entries over all of its 128 buckets (one k_radix_fine block, busy cursors), and a
    full coarse bin either side of one_level_entry_limit."""
    cr = cs.make()
    assert paths(cr) == (["one_level"] if cs.n < D.RADIX_N else ["radix"])
    a = points(gpu_ctx, cs.n)
    s = cr.scalars()
    res, info = gpu_ctx.run(s.tobytes(), c=cs.c, no_tables=True)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], a, s, cs.n), (cs.id, info)
    check_info(cr, info, cs.c)
    if cs.dist == "radix_edge":
        # the host rule: heavy = max_bucket >= 2^16 && max_bucket * Hn >= 16 * two_n, Hn = 2^8 coarse bins, two_n = 2^21
        assert (info["max_bucket"] * 256 >= 16 * 2 * cs.n) == (cs.kw["m_largest"] == 1 << 17)


# ---------------------------------------------------------------------------------------------- other entry points

@pytest.fixture(scope="module")
def ed_ctx():
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    ctx = MsmContext(_lib.CURVE_ED_ON_BLS12_377)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("cs", D.ED_CASES, ids=ids(D.ED_CASES))
def test_edwards_digits_pack_directly(ed_ctx, c_oracle, cs):
    """Ed-on-BLS12-377 (k_te_digits, one entry per point, twelve 21-bit windows in one group): no endomorphism, the crafted
    digits are the scalar's."""
    cr = cs.make()
    assert paths(cr) == ["slots"]
    a = points(ed_ctx, cs.n, seed=1701)
    s = cr.scalars()
    res, info = ed_ctx.run(s.tobytes(), c=cs.c, no_tables=True)
    took(ed_ctx, cr)
    assert (res.x, res.y) == expected_point(c_oracle, CURVE_TABLE["ed377"], a, s, cs.n), (cs.id, info)
    check_info(cr, info, cs.c)


def test_narrow_scalars(gpu_ctx, c_oracle):
    """msm_run_narrow over 16-byte scalars (k_digits_narrow<16>: digits and slice histograms of its own)."""
    cs = D.NARROW_CASE
    cr = cs.make()
    assert paths(cr) == ["slots"]
    a = points(gpu_ctx, cs.n)
    res, info = gpu_ctx.run_narrow(cr.scalars(16).tobytes(), bits=cs.narrow_bits, signed=False, c=cs.c, width=16)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], a, cr.scalars(), cs.n), info
    check_info(cr, info, cs.c)


def test_indexed_over_a_strict_subset(gpu_ctx, c_oracle):
    """msm_run_indexed: 2^18 entries over a permuted subset of 2^18 + 77 resident points."""
    cs = D.INDEXED_CASE
    cr = cs.make()
    N = D.SLOT_N[1]
    a = points(gpu_ctx, N)
    idx = np.random.default_rng(77).permutation(N)[:cs.n].astype(np.uint32)
    s = cr.scalars()
    a_sel = np.ascontiguousarray(np.frombuffer(a, dtype=np.uint8).reshape(N, 32)[idx])
    res, info = gpu_ctx.msm_indexed(s, idx, c=cs.c)
    took(gpu_ctx, cr)
    assert res.as_tuple() == expected_point(c_oracle, CURVE_TABLE["bls377"], as_c(a_sel), s, cs.n), info
    check_info(cr, info, cs.c)


@pytest.mark.parametrize("cs", D.SHARD_CASES, ids=ids(D.SHARD_CASES))
def test_bucket_shards(gpu_ctx, c_oracle, cs):
    """msm_window_sums with bucket_shard = (g, 2): the digit kernel drops the other shard's buckets before the sort -- a heavy bin
    inside shard 0, and four bins of part_len-edge sizes two on either side of the cut.  Added up by msm_combine_groups."""
    from montgomery_amd import _lib
    from montgomery_amd.distributed import combine_groups_host

    cr = cs.make()
    a = points(gpu_ctx, cs.n)
    s = cr.scalars()
    buf = (C.c_uint8 * (32 * cs.n)).from_buffer_copy(s.tobytes())
    parts = b""
    for g in range(2):
        part, info = gpu_ctx.window_sums(buf, cs.n, 0, cr.plan.K, c=cs.c, bucket_shard=(g, 2))
        check_info(cr, info, cs.c, keep=D.shard_ranges(cr.plan, g, 2))
        parts += part
    exp = expected_point(c_oracle, CURVE_TABLE["bls377"], a, s, cs.n)
    assert combine_groups_host(parts, 2, cr.plan.K, cs.c, _lib.CURVE_BLS12_377_G1) == exp


def test_bn254_nine_limb_digits(c_oracle):
    """One cycle curve: the 9-limb instantiation of k_digits in front of the same sort."""
    from montgomery_amd.api import MsmContext

    cs = D.BN254_CASE
    cr = cs.make()
    cv = CURVE_TABLE["bn254"]
    ctx = MsmContext(cv.cid)
    try:
        a = ctx.generate_points(cs.n, seed=1702, want_scalars=True, raw=True)
        s = cr.scalars()
        res, info = ctx.run(s.tobytes(), c=cs.c, no_tables=True)
        took(ctx, cr)
        assert res.as_tuple() == expected_point(c_oracle, cv, a, s, cs.n), info
        check_info(cr, info, cs.c)
    finally:
        ctx.close()
