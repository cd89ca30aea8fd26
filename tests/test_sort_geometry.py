"""The geometry of a window group's sort on the CPU: msmi::sort_geometry (montgomery_amd/csrc/msm_plan.hip) through the shim
tests/csrc/schedule_host.hip -- the sort path, the cut of every window's bucket index into coarse and fine bits, the slices, the
parts of heavy bins, the padding granule and the slot bound that sort_window_group (msm_sort.hip) allocates and launches by.
No GPU: the geometry is plain arithmetic over the plan, the shape of the group and the context's CU count.

Named cases: geometries derived by hand from the rules, not from running the code.  The arithmetic, for a group of kc_d windows
over n points (Weierstrass: 2 n entries per window, Edwards: n; on window tables the group is ONE window of all its entries):
  mean   = entries per window / buckets the digits fill (2^L_log; half of them under a folded plan), at least 1
  left   = 32 from mean 512, 16 from mean 128 (from 64 under c >= 18 off the tables), else 8
  logG   = the largest g <= 10 with 2^g * left <= mean, at least 1
  path   = bin split if 2^L_log counters exceed 128 KB (L_log >= 16) or the merged window of a run on tables has 2^22 entries;
           else radix split if L_log > 7 and a window has 2^21 entries (Edwards 2^22); else one level
  eff    = bits a window's digits have: c - 1, a folded top window c, a short top window what is left of the scalar; L_log on tables
  ab, fb = eff, 0 up to 10 bits; else ab = max(10, eff - 12), fb = eff - ab (radix split: L_log - 7, 7)
  hb     = 2^max(ab), nbmax = 2^max(fb), V = kc * hb (radix split: kc * 2^(L_log - 7))
  slices = bin split: min(4 * CUs, n / 4096), at least ceil(n / max_pps) with max_pps = 2^17 entries; pps = ceil(n / slices)
  part_len = max(2^16, 2 * entries / V rounded up to 4096); pair form: bin split, not Edwards, c >= 18, more than
           2^chunk_rows_log table rows, logG >= 2
Grid: tests/crafted_digits.py's Geometry -- the restatement every GPU test of the sort builds its inputs from -- must agree with
the library, and every geometry keeps what the kernels rely on."""
import ctypes as C
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import crafted_digits as D  # noqa: E402

from host_lib import host_library  # noqa: E402

BLS377, ED377 = 0, 1            # MSM_CURVE_BLS12_377_G1, MSM_CURVE_ED_ON_BLS12_377 (include/msm_hip.h)
N_CU = 256
BS_MAX_AB, BS_MAX_FB, BS_SPAN_LOG, BP_TILE = 11, 12, 17, 4096      # sort_kernels.h
FIELDS = ("kc_d kc two_n_d two_n n_entries nb mean logG bin_split radix pairs hb hb_stride nbmax Hn V sortB pps chunk per_block "
          "part_len part_grid parts_extra slots_bound L_log fold K bits").split()
CAP = 40000                     # groups: at most 126 windows x 256 ranges


@pytest.fixture(scope="module")
def lib():
    L = host_library("schedule_host")
    i32p, u64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    L.gs_plan.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, i32p]
    L.gs_schedule.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, i32p, i32p, u64p, u64p, i32p, i32p]
    L.gs_sort_geometry.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u64p, u8p, u8p,
                                   C.c_char_p, C.c_int]
    return L


class Geo:
    """sort_geometry of one call of the shim: its fields by name, ab / fb of the windows behind the digit kernel, path as
    crafted_digits.Geometry names it; refused = (code, text) where the function refuses the group"""

    def __init__(self, L, curve, n, c, k, tables=False, no_glv=False, chunk_rows_log=23, n_cu=N_CU):
        f, ab, fb, msg = (C.c_uint64 * len(FIELDS))(), (C.c_uint8 * 16)(), (C.c_uint8 * 16)(), C.create_string_buffer(256)
        rc = L.gs_sort_geometry(curve, n_cu, n, c, int(no_glv), k[0], k[1], int(tables), chunk_rows_log, f, ab, fb, msg, 256)
        assert rc != 0, (curve, n, c, no_glv)
        self.refused = (int(f[0]), msg.value.decode()) if rc < 0 else None
        if rc < 0:
            return
        for name, v in zip(FIELDS, f):
            setattr(self, name, int(v))
        self.ab, self.fb = list(ab)[:self.kc], list(fb)[:self.kc]
        self.path = "pairs" if self.pairs else "slots" if self.bin_split else "radix" if self.radix else "one_level"


# ---------------------------------------------------------------------------------------------- named cases

def test_first_group_of_a_big_folded_call(lib):
    """BLS12-377, 2^26 points, c = 21, windows [0, 3).  127 = 6 * 21 + 1 folds: K = 6, L_log = 21.  2^27 entries per window, three
    windows; 2^21 buckets do not fit the LDS: bin split.  The lower windows hold 20-bit digits: ab = max(10, 8) = 10, fb = 10,
    hb = nbmax = 1024, V = 3 * 1024.  Slices: min(4 * 256, 2^26 / 4096) = 1024, and 2^26 / 2^16 = 1024 for the span: pps = 2^16,
    chunk = 2^17, so pass A takes min(1024, 2^17 / 2^17 = 1) = 1 slice per block.  part_len = 2 * 3 * 2^27 / 3072 = 2^18.
    mean = 2^27 / 2^20 (folded: half of 2^21) = 128 -> left = 16; 4 * 16 and 8 * 16 = 128 fit the mean, 16 * 16 does not:
    logG = 3.  2^26 rows > 2^23, c >= 18, logG >= 2: pairs.  The parts may add min(entries, V * nbmax = 3 * 2^20) slots; the
    bound is entries + that + (2^3 - 1) * min(3 * 2^21 buckets, entries)."""
    g = Geo(lib, BLS377, 1 << 26, 21, (0, 3))
    assert (g.K, g.fold, g.L_log) == (6, 1, 21)
    assert (g.kc_d, g.kc, g.two_n_d, g.two_n, g.n_entries, g.nb) == (3, 3, 1 << 27, 1 << 27, 3 << 27, 3 << 21)
    assert (g.path, g.ab, g.fb, g.hb, g.hb_stride, g.nbmax, g.V) == ("pairs", [10] * 3, [10] * 3, 1024, 1024, 1024, 3072)
    assert (g.sortB, g.pps, g.chunk, g.per_block) == (1024, 65536, 131072, 1)
    assert (g.part_len, g.part_grid) == (1 << 18, 3072 + 1536 + 1)
    assert (g.mean, g.logG) == (128, 3)
    assert (g.parts_extra, g.slots_bound) == (3 << 20, (3 << 27) + (3 << 20) + 7 * (3 << 21))


def test_second_group_holds_the_folded_top_window(lib):
    """the same call, windows [3, 6): the top window is c + 1 = 22 bits wide and not recoded, its digits have 21 bits:
    ab = max(10, 9) = 10, fb = 11, so a bin has up to 2048 buckets; the stride of the bins stays 1024"""
    g = Geo(lib, BLS377, 1 << 26, 21, (3, 6))
    assert (g.path, g.ab, g.fb, g.hb, g.nbmax, g.V) == ("pairs", [10] * 3, [10, 10, 11], 1024, 2048, 3072)
    assert (g.part_len, g.mean, g.logG) == (1 << 18, 128, 3)
    assert g.parts_extra == min(3 << 27, 3072 * 2048)


def test_radix_boundary(lib):
    """BLS12-377, c = 16: K = 8 windows of 2^15 buckets, which fit the LDS.  2^20 points are 2^21 entries per window: the radix
    split, 8 coarse bits x 7 fine bits, 256 blocks of the last pass per window, V = 8 * 256.  mean = 2^21 / 2^15 = 64 -> left 8
    (c < 18): 2^3 * 8 = 64 fits: logG = 3.  Slices: two per CU over 8 windows = ceil(512 / 8) = 64 of 2^15 entries.
    One point less: 2^21 - 2 entries, one level; mean 63: logG = 2."""
    g = Geo(lib, BLS377, D.RADIX_N, 16, (0, 8))
    assert (g.K, g.L_log, g.path, g.ab, g.fb, g.Hn, g.V, g.hb) == (8, 15, "radix", [8] * 8, [7] * 8, 256, 2048, 1)
    assert (g.mean, g.logG, g.sortB, g.chunk, g.part_len, g.parts_extra) == (64, 3, 64, 1 << 15, 0, 0)
    assert g.slots_bound == (8 << 21) + 7 * (8 << 15)
    g = Geo(lib, BLS377, D.RADIX_N - 1, 16, (0, 8))
    assert (g.path, g.Hn, g.V, g.mean, g.logG, g.sortB, g.chunk) == ("one_level", 1, 8, 63, 2, 64, 1 << 15)
    assert g.ab == [0] * 8 and g.fb == [0] * 8


def test_edwards_takes_the_slot_form(lib):
    """Ed-on-BLS12-377, 2^19 points, c = 21: K = 252 / 21 = 12, no fold, 2^20 buckets: bin split; never pairs on this curve.
    Every window, the top one too (21 bits left), has 20-bit digits: (10, 10).  mean = 2^19 / 2^20 -> 1: logG = 1.  Slices:
    min(1024, 2^19 / 4096) = 128 of 4096 points = 4096 entries; pass A takes min(128, 2^17 / 4096 = 32, ceil(2^16 / 4096) = 16)
    = 16 per block.  part_len: 2 * 12 * 2^19 / 12288 = 1024 -> the floor 2^16."""
    g = Geo(lib, ED377, 1 << 19, 21, (0, 12))
    assert (g.K, g.fold, g.L_log, g.two_n_d) == (12, 0, 20, 1 << 19)
    assert (g.path, g.ab, g.fb, g.V) == ("slots", [10] * 12, [10] * 12, 12 << 10)
    assert (g.mean, g.logG, g.sortB, g.pps, g.chunk, g.per_block, g.part_len, g.parts_extra) == (1, 1, 128, 4096, 4096, 16, 1 << 16, 0)


def test_pair_form_on_window_tables_counts_the_rows_of_all_tables(lib):
    """BLS12-377, c = 18 (127 = 7 * 18 + 1 folds: 2^18 buckets) on window tables, four windows: ONE merged window of 4 * 2 n entries
    whose digits have all 18 bits: ab = 10, fb = 8, V = 1024.  4 * 2^21 rows are not MORE than 2^23: slots; 4 * (2^21 + 4096) are:
    pairs (mean = 2^24 / 2^17 = 128 -> left 16 -> logG = 3).  The group behind it has three tables: slots."""
    g = Geo(lib, BLS377, D.TABLES_N - 4096, 18, (0, 4), tables=True)
    assert (g.kc_d, g.kc, g.two_n, g.nb, g.path, g.ab, g.fb, g.V, g.mean, g.logG) == (4, 1, 1 << 24, 1 << 18, "slots", [10], [8], 1024, 128, 3)
    g = Geo(lib, BLS377, D.TABLES_N, 18, (0, 4), tables=True)
    assert (g.path, g.two_n, g.mean, g.logG) == ("pairs", (1 << 24) + (1 << 15), 128, 3)
    assert Geo(lib, BLS377, D.TABLES_N, 18, (4, 7), tables=True).path == "slots"
    # a lowered threshold (msm_test_set_chunk_rows_log) moves the switch, and with it the slots the parts may add; nothing else
    hi, lo = (Geo(lib, BLS377, D.TABLES_N - 4096, 18, (0, 4), tables=True, chunk_rows_log=r) for r in (23, 22))
    assert (hi.path, lo.path, hi.parts_extra, lo.parts_extra) == ("slots", "pairs", 0, 1024 << 8)
    same = [f for f in FIELDS if f not in ("pairs", "parts_extra", "slots_bound")]
    assert [getattr(hi, f) for f in same] == [getattr(lo, f) for f in same]


def test_short_top_window_is_sorted_outright(lib):
    """BLS12-377, c = 24: K = 6, the top window holds 127 - 120 = 7 bits: up to 10 bits pass A sorts the window outright,
    ab = 7, fb = 0; the others have 23-bit digits: ab = max(10, 11) = 11, fb = 12, hb = 2048.  c = 20: K = 7, 127 - 120 = 7 too."""
    g = Geo(lib, BLS377, 1 << 18, 24, (0, 6))
    assert (g.K, g.fold, g.path, g.ab, g.fb, g.hb, g.nbmax, g.V) == (6, 0, "slots", [11] * 5 + [7], [12] * 5 + [0], 2048, 4096, 6 * 2048)
    g = Geo(lib, BLS377, 1 << 18, 20, (0, 7))
    assert (g.ab[6], g.fb[6], g.hb) == (7, 0, 1024)


def test_cases_the_python_model_is_pinned_on(lib):
    """what tests/test_crafted_digits.py asserts of crafted_digits.Geometry, asserted of the library"""
    g = Geo(lib, BLS377, 1 << 18, 21, (0, 6))
    assert (g.path, g.ab, g.fb, g.part_len, g.V) == ("slots", [10] * 6, [10] * 5 + [11], 1 << 16, 6 << 10)
    assert Geo(lib, BLS377, 1 << 18, 18, (0, 7)).fb == [7] * 6 + [8]
    assert [Geo(lib, BLS377, D.PAIR_N, 18, k).path for k in ((0, 4), (4, 7))] == ["pairs", "pairs"]
    assert Geo(lib, BLS377, D.PAIR_N, 21, (0, 3)).path == "slots"      # (mean bucket 16: logG = 1)
    assert Geo(lib, BLS377, D.PAIR_N, 21, (0, 3)).logG == 1
    assert Geo(lib, BLS377, 1 << 24, 21, (0, 3)).path == "pairs"


def test_refusals_keep_their_code_and_text(lib):
    """more windows than a WinSplit describes, off the one-level sort: MSM_ERR_INTERNAL = 7 (include/msm_hip.h).  The schedule never
    makes such a group (test_no_group_of_the_schedule_is_refused)."""
    assert Geo(lib, ED377, 1 << 20, 17, (0, 15)).refused is None
    # BLS12-377 without the endomorphism, c = 9: K = ceil(254 / 9) = 29 windows of 2^8 buckets; 2^21 entries: the radix split
    assert Geo(lib, BLS377, 1 << 20, 9, (0, 29), no_glv=True).refused == (7, "more than 16 windows in a radix-split group")
    assert Geo(lib, BLS377, (1 << 20) - 1, 9, (0, 29), no_glv=True).path == "one_level"      # (no table of 16 entries there)
    assert Geo(lib, BLS377, 1 << 20, 9, (0, 16), no_glv=True).path == "radix"
    # c = 17: 17 windows (as the virtual windows of a fused batch would be: no single scalar has that many)
    assert Geo(lib, BLS377, 1 << 12, 17, (0, 17), no_glv=True).refused == (7, "more than 16 windows in a group of a window size above 16")


# ---------------------------------------------------------------------------------------------- the grid

class PlanOnly(D.Plan):
    """crafted_digits.Plan filled from the library's plan: the windows no crafted value reaches (which D.Plan refuses) and the
    plans without the endomorphism included.  eff_bits and window_groups are D.Plan's."""

    def __init__(self, te, c, K, L_log, fold, bits):
        self.te, self.c, self.K, self.L_log, self.fold, self.bits = te, c, K, L_log, bool(fold), bits
        self.per_point = 1 if te else 2


def _plans(lib, curve, n):
    plan = (C.c_int32 * 2)()
    return [(c, ng, plan[0]) for ng in ((0,) if curve == ED377 else (0, 1)) for c in range(1, 26) if lib.gs_plan(curve, n, c, ng, plan)]


def _check_invariants(g, te, c, n, tag):
    assert g.sortB * g.pps >= n and g.slots_bound >= g.n_entries, tag
    assert g.hb_stride == g.hb and g.V == g.kc * (g.hb if g.bin_split else g.Hn), tag
    if g.bin_split or g.radix:
        assert g.kc <= 16, tag                                         # a WinSplit is filled
    if g.bin_split:
        eff = [a + f for a, f in zip(g.ab, g.fb)]
        assert max(g.ab) <= BS_MAX_AB and max(g.fb) <= BS_MAX_FB and g.hb == 1 << max(g.ab) and g.nbmax == 1 << max(g.fb), tag
        assert all(1 <= e <= g.L_log for e in eff), tag
        assert g.chunk <= 1 << BS_SPAN_LOG and g.chunk == (1 if te else 2) * g.pps, tag
        assert 1 <= g.per_block <= g.sortB and g.per_block * g.chunk <= max(g.chunk, 1 << BS_SPAN_LOG), tag
        assert g.part_len % BP_TILE == 0 and g.part_len >= 1 << 16 and g.part_grid == g.V + g.V // 2 + 1, tag
    else:
        assert (g.part_len, g.part_grid, g.pairs, g.hb, g.nbmax) == (0, 0, 0, 1, 1), tag
    if g.radix:
        assert g.ab == [g.L_log - 7] * g.kc and g.fb == [7] * g.kc and g.Hn == 1 << (g.L_log - 7) <= 256, tag
    if g.pairs:
        assert g.logG >= 2 and c >= 18 and not te and g.bin_split, tag
    assert g.parts_extra == (min(g.n_entries, g.V * g.nbmax) if g.pairs else 0), tag


@pytest.mark.parametrize("lg", range(10, 30))
@pytest.mark.parametrize("curve", [BLS377, ED377])
def test_python_model_agrees_and_invariants_hold(lib, curve, lg):
    te = curve == ED377
    n = (1 << lg) + (37 if lg % 3 == 0 else 0)
    paths, refused = set(), 0
    for c, no_glv, K in _plans(lib, curve, n):
        for tables in (False, True):
            for rows_log in (23, 12):
                pl = None
                for k in (D.Plan.window_groups(PlanOnly(te, c, K, 0, False, 0), n, tables)):
                    tag = (curve, n, c, no_glv, k, tables, rows_log)
                    g = Geo(lib, curve, n, c, k, tables, no_glv, rows_log)
                    if g.refused:                                      # (the schedule cuts such a group: see the test below)
                        assert k[1] - k[0] > 16 and not tables, tag
                        refused += 1
                        continue
                    if g.two_n > 1 << 31:                              # (a payload names its entry in 31 bits, msm_kernels.h: no
                        continue                                       # such window runs -- the schedule cuts it by points)
                    pl = pl or PlanOnly(te, c, g.K, g.L_log, g.fold, g.bits)
                    assert g.K == K and (g.kc_d, g.kc) == (k[1] - k[0], 1 if tables else k[1] - k[0]), tag
                    m = D.Geometry(pl, n, k[0], k[1], tables, 1 << rows_log)
                    assert (m.path, m.part_len, m.mean, m.logG, m.n_entries) == (g.path, g.part_len, g.mean, g.logG, g.n_entries), tag
                    if g.path != "one_level":                          # (the one-level sort cuts nothing)
                        assert (m.ab, m.fb, m.V) == (g.ab, g.fb, g.V) and m.hb == (g.hb if g.bin_split else g.Hn), tag
                    if g.bin_split:                                    # ab + fb = the window's effective bits
                        assert [a + f for a, f in zip(g.ab, g.fb)] == [pl.eff_bits(k[0] + kk, tables) for kk in range(g.kc)], tag
                    _check_invariants(g, te, c, n, tag)
                    paths.add(g.path)
    # the grid reaches the paths it is there for
    assert "slots" in paths and ("one_level" in paths or lg > 19) and ("radix" in paths or lg < 22), (paths, lg)
    assert ("pairs" in paths) == (not te) or lg < 22, (paths, lg)
    assert refused == 0 or lg >= 20, (refused, lg)                     # (below 2^20 points only narrow windows come 17 to a group)


@pytest.mark.parametrize("lg", range(10, 30))
@pytest.mark.parametrize("curve", [BLS377, ED377])
def test_no_group_of_the_schedule_is_refused(lib, curve, lg):
    """every group group_schedule itself produces -- plain and on tables, roomy and tight budgets, whole and partial window
    ranges -- has a geometry"""
    n = (1 << lg) + (37 if lg % 3 == 0 else 0)
    ka, kb, lo, cnt = (C.c_int32 * CAP)(), (C.c_int32 * CAP)(), (C.c_uint64 * CAP)(), (C.c_uint64 * CAP)()
    piece, flags = (C.c_int32 * CAP)(), (C.c_int32 * 6)()
    seen = 0
    for c, no_glv, K in _plans(lib, curve, n):
        for budget in (250 << 30, 4 << 30):
            for tab_T in (0, K):
                for k in {(0, K), (min(1, K - 1), K)}:
                    cnt_g = lib.gs_schedule(curve, N_CU, budget, n, 0, c, no_glv, k[0], k[1], tab_T, 0, n, 0, 0, CAP, ka, kb, lo, cnt, piece, flags)
                    assert cnt_g > 0, (curve, n, c, no_glv, budget, tab_T, k)
                    for grp in {(ka[i], kb[i], cnt[i]) for i in range(cnt_g)}:
                        g = Geo(lib, curve, grp[2], c, grp[:2], bool(flags[1]), no_glv)
                        assert g.refused is None, (curve, n, c, no_glv, budget, tab_T, k, grp, g.refused)
                        seen += 1
                    if flags[4]:                                       # one digit launch over both groups' windows
                        assert Geo(lib, curve, n, c, (ka[0], kb[1]), bool(flags[1]), no_glv).refused is None, (curve, n, c, no_glv, k)
    assert seen > 0
