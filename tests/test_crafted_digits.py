"""tests/crafted_digits.py proved on the CPU, for every input tests/test_gpu_sort_shapes.py runs: every pool scalar is below q,
decomposes into the crafted halves and recodes into the crafted digits under the plan's K (no scalar is left out: the inputs
are chosen so that the round trip holds for the whole pool); the histogram meets the structural claim of the distribution --
bin sizes against part_len, populated buckets, the largest bucket -- and the point order the claims about parts; and
expected_stats agrees with the bucket walk of the oracle's batched-affine MSM on a small instance.  No GPU."""
import numpy as np
import pytest

import crafted_digits as D
from degenerate_inputs import CURVE_TABLE, pool as point_pool
from oracle import msm_oracle as O

CASES = {cs.id: cs for cs in D.ALL_CASES}


def bin_sizes(cr, hist, window):
    """records per bin of (the merged window of) `window` from its bucket histogram"""
    fb = cr.fb[window]
    h = hist[1:].astype(np.int64)
    h = np.concatenate([h, np.zeros(-len(h) % (1 << fb), dtype=np.int64)])
    return h.reshape(-1, 1 << fb).sum(axis=1)


def hist_of(cr, hists, window):
    if not cr.tables:
        return hists[window]
    return hists[[i for i, (lo, hi) in enumerate(cr.merged()) if lo <= window < hi][0]]


def test_plan_arithmetic_is_make_plans():
    """K, the fold and the cuts of the sort for the plans the GPU tests name (include/msm_hip.h: K = ceil((b + 1) / c), b = 126
    after GLV on BLS12-377 and BN254, 251 on the Edwards curve; msm_sort.hip for the cuts)."""
    for curve, c, K, fold in (("bls377", 16, 8, False), ("bls377", 18, 7, True), ("bls377", 20, 7, False), ("bls377", 21, 6, True),
                              ("bls377", 24, 6, False), ("bn254", 21, 6, True), ("ed377", 21, 12, False)):
        pl = D.Plan(curve, c)
        assert (pl.K, pl.fold) == (K, fold), (curve, c)
    assert D.Plan("bls377", 21, D.NARROW_BITS).K == 6 and not D.Plan("bls377", 21, D.NARROW_BITS).fold
    g = D.Geometry(D.Plan("bls377", 21), 1 << 18, 0, 6)
    assert (g.path, g.ab, g.fb, g.part_len, g.V) == ("slots", [10] * 6, [10] * 5 + [11], 1 << 16, 6 << 10)
    assert D.Geometry(D.Plan("bls377", 18), 1 << 18, 0, 7).fb == [7] * 6 + [8]
    g = D.Geometry(D.Plan("bls377", 24), 1 << 18, 0, 6)
    assert (g.ab, g.fb, g.hb) == ([11] * 5 + [7], [12] * 5 + [0], 2048)
    assert D.Geometry(D.Plan("bls377", 20), 1 << 18, 0, 7).fb[6] == 0
    p18 = D.Plan("bls377", 18)
    assert p18.window_groups(D.PAIR_N) == [(0, 4), (4, 7)]
    assert [D.Geometry(p18, D.PAIR_N, lo, hi).path for lo, hi in p18.window_groups(D.PAIR_N)] == ["pairs", "pairs"]
    assert D.Geometry(D.Plan("bls377", 21), D.PAIR_N, 0, 3).path == "slots"     # (mean bucket 16: logG = 1)
    assert D.Geometry(D.Plan("bls377", 21), 1 << 24, 0, 3).path == "pairs"
    assert [D.Geometry(p18, D.TABLES_N, lo, hi, True).path for lo, hi in p18.window_groups(D.TABLES_N, True)] == ["pairs", "slots"]
    assert D.Geometry(p18, D.TABLES_N - 4096, 0, 4, True).path == "slots"       # 4 x 2^21 rows: not MORE than 2^23
    p16 = D.Plan("bls377", 16)
    assert D.Geometry(p16, D.RADIX_N, 0, 8).path == "radix" and D.Geometry(p16, D.RADIX_N - 1, 0, 8).path == "one_level"
    assert D.Geometry(D.Plan("ed377", 21), 1 << 19, 0, 12).path == "slots"


def test_scalar_from_digits_and_glv_scalar():
    assert D.scalar_from_digits([5, -3, 2], 4) == 5 - 3 * 16 + 2 * 256
    assert D.scalar_from_digits([8, 0, 1], 4) == 8 + 256
    with pytest.raises(AssertionError):
        D.scalar_from_digits([-8], 4)          # 2^(c-1) only as a positive digit
    B = O.BLS12_377
    assert D.glv_scalar(3, 5, "bls377") == (3 + 5 * B.lam) % B.q
    with pytest.raises(AssertionError):
        D.glv_scalar(1 << 125, 0, "bls377")


@pytest.mark.parametrize("curve", sorted(D.HALF_BITS))
def test_half_bound_round_trips(curve):
    """HALF_BITS: random halves of exactly that many bits, and of a few smaller lengths, all come back from O.glv_decompose."""
    cv = CURVE_TABLE[curve]
    bits = D.HALF_BITS[curve]
    for nb in (bits, bits - 1, bits - 5, 64, 1):
        top = 1 << (nb - 1)
        ks = [top | v for v in O.prng_ints(f"crafted/{curve}/{nb}", 400, top)]
        for k1, k2 in zip(ks[:200], ks[200:]):
            assert O.glv_decompose(D.glv_scalar(k1, k2, curve), cv.glv) == (k1, k2, False, False)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_pool_round_trips_and_structure(cid, c_oracle):
    cs = CASES[cid]
    cr = cs.make()
    pl = cr.plan
    cv = pl.cv
    c, K = pl.c, pl.K
    # ---- the whole pool: below q, GLV gives the halves back, the halves recode into the crafted digits
    scalars, halves, digits = cr.pool_scalars(), cr.halves(), cr.digits.tolist()
    assert len(set(scalars)) == len(scalars) == len(cr.counts)
    for j, s in enumerate(scalars):
        assert 0 <= s < cv.q
        if pl.halves == 2:
            assert O.glv_decompose(s, cv.glv) == (halves[j][0], halves[j][1], False, False), j
        else:
            assert s == halves[j][0] and s < (1 << pl.value_bits)
        for hf in range(pl.halves):
            assert halves[j][hf] < (1 << pl.value_bits)
            # (a zero digit is no entry and has no sign: the oracle reports the carry it passes on)
            assert [(l, neg and l != 0) for l, neg in O.signed_digits(halves[j][hf], c, K)] == [(abs(e), e < 0) for e in digits[j][hf]], (j, hf)
    if cs.curve == "bls377" and pl.halves == 2:
        for j in range(0, len(scalars), max(1, len(scalars) // 64)):
            assert c_oracle.glv_decompose(scalars[j]) == (halves[j][0], halves[j][1], False, False)
    if cs.narrow_bits:
        assert all(s < (1 << cs.narrow_bits) for s in scalars) and cs.narrow_bits <= 128
    assert cr.counts.sum() == cr.n == len(cr.order) and (np.bincount(cr.order, minlength=len(cr.counts)) == cr.counts).all()
    # ---- the histogram against the claims
    hists, largest, pairs = cr.stats()
    assert sum(int(h[1:].sum()) for h in hists) == int((np.broadcast_to(cr.counts[:, None, None], cr.digits.shape) * (cr.digits != 0)).sum())
    assert pairs == sum(int(h[1:].sum()) - int((h[1:] > 0).sum()) for h in hists)
    for (w, b), records in cr.bins.items():
        sizes = bin_sizes(cr, hist_of(cr, hists, w), w)
        assert sizes[b] == records, (w, b)
        fb = cr.fb[w]
        in_bin = hist_of(cr, hists, w)[1 + (b << fb):1 + ((b + 1) << fb)]
        assert int((in_bin > 0).sum()) == cr.buckets[(w, b)]
    geo_path = {lo: D.Geometry(pl, cr.n, lo, hi, cr.tables).path for lo, hi in pl.window_groups(cr.n, cr.tables)}
    bin_split = all(p in ("slots", "pairs") for p in geo_path.values())
    if bin_split and cs.dist != "short_top":
        # the planted bins above part_len are cut into parts (there may be more: the other digits of a class of few entries
        # are deep buckets of their own -- the giant's, or those of the four entries of `runs`)
        for w0 in ([lo for lo, _ in cr.merged()] if cr.tables else range(K)):
            sizes = bin_sizes(cr, hist_of(cr, hists, w0), w0)
            heavy = set(np.nonzero(sizes > cr.part_len[w0])[0].tolist())
            planted = {b for (w, b), r in cr.bins.items() if w == w0 and r > cr.part_len[w0]}
            assert heavy >= planted, (w0, heavy, planted)
    (w, b), records = next(iter(cr.bins.items()))
    part_len, NB = cr.part_len[w] or (1 << 16), 1 << cr.fb[w]
    if cs.dist == "full_bin":
        assert records == 3 * part_len + 1 and cr.buckets[(w, b)] == NB and 0 < b < len(bin_sizes(cr, hists[0], w)) - 1
        d = np.concatenate([cr.digits[:, :, k].ravel() for k in cr.windows_of(w)])
        mine = (d != 0) & (((np.abs(d) - 1) >> cr.fb[w]) == b)
        assert len(np.unique(d[mine])) == 2 * NB                           # both signs in every bucket
    elif cs.dist == "exact_edges":
        assert sorted(r for (ww, _), r in cr.bins.items() if ww == w) == sorted([part_len, part_len + 1, 2 * part_len, 2 * part_len - 1])
        assert len(cr.bins) == 4 and len({ww for ww, _ in cr.bins}) == 1
    elif cs.dist == "ends":
        fbt = cr.fb[K - 1]
        assert set(cr.bins) == {(0, 0), (K - 1, (pl.top_max - 1) >> fbt)}
        assert all(r > cr.part_len[ww] for (ww, _), r in cr.bins.items())
        assert hists[K - 1][pl.top_max] > 0 and len(hists[K - 1]) == pl.top_max + 1 or hists[K - 1][pl.top_max + 1:].sum() == 0
        assert hists[0][1] > 0 and (c not in (18, 21) or pl.top_max == 1 << (c - 1))
    elif cs.dist == "neighbours":
        for w0 in ([lo for lo, _ in cr.merged()] if cr.tables else range(K)):
            bs = sorted(bb for (ww, bb), r in cr.bins.items() if ww == w0 and r > cr.part_len[w0])
            assert len(bs) == 3 and bs[1] == bs[0] + 1, (w0, bs)
    elif cs.dist in ("alternating", "runs"):
        assert cr.buckets[(w, b)] == 4 and records > 3 * part_len
        rec = cr.bin_records(w, b)
        assert len(rec) == records
        parts = [rec[i:i + part_len] for i in range(0, records, part_len)]
        assert len(parts) == 4
        if cs.dist == "alternating":
            for part in parts:
                _, cnt = np.unique(part, return_counts=True)
                assert (cnt % 2 == 1).all(), cnt
            assert all(len(np.unique(part)) == 4 for part in parts[:3])
        else:
            assert (np.diff(np.searchsorted(np.unique(rec), rec)) >= 0).all()       # sorted by bucket
            for a, z in zip(parts, parts[1:]):
                assert a[-1] == z[0] and len(np.intersect1d(a, z)) == 1             # one bucket straddles the boundary
    elif cs.dist == "giant_and_singletons":
        in_bin = np.sort(hist_of(cr, hists, w)[1 + (b << cr.fb[w]):1 + ((b + 1) << cr.fb[w])])
        assert in_bin[-1] == 2 * part_len + 1 and set(in_bin[:-1].tolist()) == {1, 2, 3} and records > part_len
    elif cs.dist == "short_top":
        assert cr.fb[K - 1] == 0 and len(cr.bins) == 2 and sum(cr.bins.values()) == pl.per_point * cr.n
        assert int((hists[K - 1][1:] > 0).sum()) == 2
    elif cs.dist == "radix_edge":
        assert largest == cs.kw["m_largest"] == records
        assert sorted(h[1:].max() for h in hists)[-1] == largest and all(np.sort(h[1:])[-3] < largest // 8 for h in hists)
    elif cs.dist == "radix_fat_bin":
        assert records == cr.n == pl.per_point * cr.n // 2 and cr.buckets[(w, b)] == NB == 128
        assert largest <= 1 << 16 and hists[w][1 + (b << 7):1 + ((b + 1) << 7)].min() == cr.n // NB


@pytest.mark.parametrize("curve,c,dist", [("bls377", 12, "full_bin"), ("bls377", 13, "full_bin"), ("bn254", 12, "giant_and_singletons")])
def test_small_msm_and_the_bucket_walk(curve, c, dist):
    """64 pool scalars of a crafted input over 64 points: the oracle's batched-affine MSM under the plan's window equals its
    plain sum, and the buckets it fills -- GLV halves, signed digits, one entry per non-zero digit: msm_batched_affine's slice
    phase restated -- are expected_stats' histogram, largest bucket and pair additions."""
    cv = CURVE_TABLE[curve]
    pl = D.Plan(curve, c)
    cr = D.DISTS[dist](pl, 1 << 18)
    pick = np.concatenate([np.arange(40), np.arange(len(cr.counts) - 24, len(cr.counts))])      # planted entries and fill
    scalars = [cr.pool_scalars()[j] for j in pick]
    points = point_pool(curve)[0]
    assert O.msm_batched_affine(scalars, points, cv.B, c=c) == O.msm_naive_affine(scalars, points, cv.B)
    walk = [dict() for _ in range(pl.K)]
    for s in scalars:
        a0, a1, n0, n1 = O.glv_decompose(s, cv.glv)
        assert not n0 and not n1
        for half in (a0, a1):
            for k, (l, _neg) in enumerate(O.signed_digits(half, c, pl.K)):
                if l:
                    walk[k][l] = walk[k].get(l, 0) + 1
    hists, largest, pairs = D.expected_stats(cr.digits[pick], np.ones(len(pick), dtype=np.int64), c, pl.K)
    for k in range(pl.K):
        assert {int(l): int(hists[k][l]) for l in np.nonzero(hists[k])[0] if l} == walk[k]
    assert largest == max(v for w in walk for v in w.values())
    assert pairs == sum(v - 1 for w in walk for v in w.values())


def test_shard_ranges_cut_at_a_bin_boundary():
    pl = D.Plan("bls377", 21)
    r0, r1 = D.shard_ranges(pl, 0, 2), D.shard_ranges(pl, 1, 2)
    assert r0[0] == (0, 1 << 19) and r1[0] == (1 << 19, 1 << 21) and r0[5] == (0, 1 << 20) and r1[5] == (1 << 20, 1 << 21)
    cr = D.SHARD_CASES[1].make()
    fb = cr.fb[3]
    assert (511 << fb) + (1 << fb) == 1 << 19 and {b for _, b in cr.bins} == {510, 511, 512, 513}      # two bins on either side of the cut
    whole = cr.stats()
    parts = [cr.stats(keep=D.shard_ranges(pl, g, 2)) for g in range(2)]
    assert parts[0][2] + parts[1][2] == whole[2] and max(parts[0][1], parts[1][1]) == whole[1]


# ---------------------------------------------------------------------------------------------- the pair form at small sizes

ALL_W = ("bls377", "bls381", "pallas", "bn254", "grumpkin", "vesta")


def test_geometry_takes_the_row_threshold():
    """The default is msm_sort.hip's 2^23 rows; a lowered threshold leaves c >= 18 and logG >= 2 as the conditions."""
    p18, p21 = D.Plan("bls377", 18), D.Plan("bls377", 21)
    for n in (1 << 21, D.PAIR_N):
        assert D.sort_paths(p18, n) == D.sort_paths(p18, n, chunk_rows=1 << 23)
    assert D.sort_paths(p18, 1 << 21) == ["slots"] and D.sort_paths(p18, 1 << 21, chunk_rows=1 << D.PAIR_ROWS_LOG) == ["pairs"]
    assert D.sort_paths(p18, 1 << 21, chunk_rows=1 << 21) == ["slots"]           # rows must EXCEED the threshold
    assert D.sort_paths(p18, (1 << 21) + 1, chunk_rows=1 << 21) == ["pairs"]
    assert D.sort_paths(D.Plan("bls377", 16), 1 << 21, chunk_rows=1 << D.PAIR_ROWS_LOG) == ["radix"]      # c < 18: never
    assert D.sort_paths(D.Plan("ed377", 21), 1 << 23, chunk_rows=1 << D.PAIR_ROWS_LOG) == ["slots", "slots"]   # nor the Edwards curve
    g = D.Geometry(p21, 1 << 24, 0, 3)
    assert (g.mean, g.logG, g.rows) == (32, 2, 1 << 24)
    g = D.Geometry(p18, 1 << 21, 0, 7)
    assert (g.mean, g.logG, g.part_len, g.V) == (32, 2, 1 << 16, 7 << 10)


@pytest.mark.parametrize("curve", ALL_W)
def test_smallest_pair_form_sizes(curve):
    """PAIR_MIN_PLAIN and PAIR_MIN_TABLES, derived by hand in tests/crafted_digits.py, against Geometry under the lowered
    threshold: at the size every window group takes the pair form, one point less and a group's mean bucket is 31 -- logG = 1,
    the slot form.  K per curve: b = 126 (BLS12-377, BN254, Grumpkin) or 127 bits after the endomorphism split."""
    rows = 1 << D.PAIR_ROWS_LOG
    K18 = {"bls377": 7, "bn254": 7, "grumpkin": 7, "bls381": 8, "pallas": 8, "vesta": 8}[curve]
    K21 = {"bls377": 6, "bn254": 6, "grumpkin": 6, "bls381": 7, "pallas": 7, "vesta": 7}[curve]
    for c, K in ((18, K18), (21, K21), (22, 6)):
        pl = D.Plan(curve, c)
        assert pl.K == K, (curve, c)
        n = D.PAIR_MIN_PLAIN[c]
        assert n == 1 << (c + 3)
        assert set(D.sort_paths(pl, n, False, rows)) == {"pairs"} and set(D.sort_paths(pl, n - 1, False, rows)) == {"slots"}
        assert all(D.Geometry(pl, n, lo, hi, False, rows).mean == 32 for lo, hi in pl.window_groups(n))
        assert all(D.Geometry(pl, n - 1, lo, hi, False, rows).logG == 1 for lo, hi in pl.window_groups(n - 1))
        n = D.PAIR_MIN_TABLES[(c, K)]
        groups = pl.window_groups(n, True)
        small = min(hi - lo for lo, hi in groups)
        assert len(groups) == (1 if n < (1 << 21) else 2) and small == (K if len(groups) == 1 else K // 2)
        assert n == -(-(1 << (c + 3)) // small)
        assert set(D.sort_paths(pl, n, True, rows)) == {"pairs"}, (curve, c)
        assert "slots" in D.sort_paths(pl, n - 1, True, rows), (curve, c)
        assert min(D.Geometry(pl, n - 1, lo, hi, True, rows).mean for lo, hi in pl.window_groups(n - 1, True)) == 31
    # at the default threshold the 18-bit sizes take the slot form; the 21- and 22-bit ones have more than 2^23 rows anyway (the
    # GPU tests reach THEIR slot form by raising the threshold)
    pl = D.Plan(curve, 18)
    assert set(D.sort_paths(pl, 1 << 21)) == {"slots"} and set(D.sort_paths(pl, D.PAIR_MIN_TABLES[(18, K18)], True)) == {"slots"}
    assert set(D.sort_paths(D.Plan(curve, 21), D.PAIR_MIN_TABLES[(21, K21)], True)) == {"pairs"}
    assert set(D.sort_paths(D.Plan(curve, 21), D.PAIR_MIN_TABLES[(21, K21)], True, 1 << 40)) == {"slots"}


def test_the_tables_cases_mix_both_forms():
    """Two window groups of one call in different forms: on window tables the groups of a seven-window plan merge four and
    three windows, and a threshold between 3 n and 4 n rows -- the default one at TABLES_N -- gives the first the pair form and
    the second the slot form.  The plain path cannot: its groups all see n rows."""
    p18 = D.Plan("bls377", 18)
    assert p18.window_groups(D.TABLES_N, True) == [(0, 4), (4, 7)] and 3 * D.TABLES_N <= (1 << 23) < 4 * D.TABLES_N
    assert D.sort_paths(p18, D.TABLES_N, True) == ["pairs", "slots"]
    assert D.sort_paths(p18, D.TABLES_N, True, 1 << D.PAIR_ROWS_LOG) == ["pairs", "pairs"]
    assert len(set(D.sort_paths(p18, D.PAIR_N, False, 1 << 22))) == 1


def _layout_case(curve, tables, narrow_bits=0, layouts=None):
    pl = D.Plan(curve, 18, narrow_bits)
    n = D.PAIR_MIN_TABLES[(18, pl.K)] if tables else D.PAIR_MIN_PLAIN[18]
    if tables == "parts":
        return D.degenerate_pairs_in_parts(pl, n, layouts=layouts)
    return D.degenerate_pairs(pl, n, tables=tables, layouts=layouts)


@pytest.mark.parametrize("curve,tables,narrow_bits", [("bls377", False, 0), ("bn254", False, 0), ("bls377", True, 0), ("bn254", True, 0),
                                                      ("bls377", "parts", 0), ("bn254", "parts", 0), ("bls377", False, D.NARROW_BITS)])
def test_degenerate_layouts_produce_their_pairs(curve, tables, narrow_bits):
    """Every layout, by the bucket walk of the pair form (pair_kinds): EVERY bucket of its lone scalar holds exactly the pairs
    written down by hand for the layout, kind by kind and round by round (LAYOUT_PAIRS) -- and the bucket that "parts" spreads
    over two parts of a multi-part bin those of LAYOUT_PAIRS_TWO_PARTS, with an entry paired with nothing at the end of both
    parts; the lone scalars are below q and come back from the decomposition and the recoding."""
    layouts = dict(D.DEGENERATE_LAYOUTS, **D.TORSION_LAYOUTS) if narrow_bits else None
    dp = _layout_case(curve, tables, narrow_bits, layouts)
    tables = bool(tables)
    cr, pl = dp.cr, dp.cr.plan
    cv = pl.cv
    geo = [D.Geometry(pl, cr.n, lo, hi, tables, 1 << D.PAIR_ROWS_LOG) for lo, hi in pl.window_groups(cr.n, tables)]
    assert {g.path for g in geo} == {"pairs"} and {g.logG for g in geo} == {2}
    for j in range(len(dp.groups)):
        s, hv = cr.pool_scalars()[j], cr.halves()[j]
        assert 0 <= s < cv.q
        if pl.halves == 2:
            assert O.glv_decompose(s, cv.glv) == (hv[0], hv[1], False, False)
        for hf in range(pl.halves):
            assert [(l, neg and l != 0) for l, neg in O.signed_digits(hv[hf], pl.c, pl.K)] == [(abs(e), e < 0) for e in cr.digits[j][hf].tolist()]
    logs = {at: 1000003 * (at + 1) + 7 for _, pos in dp.groups for at in pos}       # stand-ins for the a_i: distinct, non-zero
    kinds = D.pair_kinds(dp, dp.values(logs.__getitem__, cv.q), 2, glv=not narrow_bits)
    for name, pos in dp.groups:
        assert pos == sorted(pos) and len(set(pos)) == len(pos)
    D.check_layout_pairs(dp, kinds)
    # a scalar has a bucket per non-zero digit: 2 K of them with the endomorphism (the planted one counts for two digits), K without
    digits = pl.halves * pl.K
    assert all(digits - 2 <= len(kinds[j]) + (j in getattr(dp, "planted", {})) <= digits for j in kinds)
    if hasattr(dp, "planted"):
        (w, b), records = max(cr.bins.items(), key=lambda kv: kv[1])
        assert len(dp.planted) == len(dp.groups) and 2 * cr.part_len[0] < records <= 3 * cr.part_len[0]


def test_combine_is_the_kernels_case_table():
    q = 101
    assert D.combine(D.ABSENT, D.ABSENT, q) == ("zero", (0, 0)) and D.combine((0, 0), D.ABSENT, q)[0] == "zero"
    assert D.combine((5, 0), D.ABSENT, q) == ("copy_a_absent", (5, 0)) and D.combine((5, 0), (0, 0), q) == ("copy_a_identity", (5, 0))
    assert D.combine((0, 0), (7, 0), q) == ("copy_b", (7, 0))
    assert D.combine((5, 0), (5, 0), q) == ("double", (10, 0)) and D.combine((5, 0), (96, 0), q) == ("cancel", (0, 0))
    assert D.combine((0, 1), (0, 1), q) == ("cancel", (0, 0))                   # T + T: y = 0
    assert D.combine((5, 1), (5, 1), q) == ("double", (10, 0))                  # (P + T) doubled: 2 T = O
    assert D.combine((5, 1), (96, 1), q) == ("cancel", (0, 0)) and D.combine((5, 1), (96, 0), q) == ("generic", (0, 1))
