"""The window-group schedule of a call on the CPU: msmi::group_schedule (montgomery_amd/csrc/msm_plan.hip) through the shim
tests/csrc/schedule_host.hip -- how windows [k_lo, k_hi) over n points are cut into window groups and ranges of the points under a
workspace budget.  No GPU: the schedule is plain arithmetic over the plan, the CU count and the budget.

Named cases: schedules derived by hand from the rules (the arithmetic is in each case's comment), not from running the code.
Grid: invariants that every schedule must keep -- the ones a kernel would otherwise find out (a WinSplit of 16 entries, tab_T
tables, rows of other points' tables) -- over both curve kinds, n = 2^10 .. 2^29, every window make_plan accepts, budgets from
64 MiB to 250 GiB, tables absent / matching / over another range, full and partial window ranges."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]

from host_lib import host_library  # noqa: E402

BLS377, ED377 = 0, 1            # MSM_CURVE_BLS12_377_G1, MSM_CURVE_ED_ON_BLS12_377 (include/msm_hip.h)
MiB, GiB = 1 << 20, 1 << 30
CAP = 40000                     # groups: at most 126 windows x 256 ranges


@pytest.fixture(scope="module")
def lib():
    L = host_library("schedule_host")
    i32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    L.gs_plan.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, i32p]
    L.gs_window_bytes.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int]
    L.gs_window_bytes.restype = C.c_uint64
    L.gs_leaves_one_level.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int]
    L.gs_schedule.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, i32p, i32p, u64p, u64p, i32p, i32p]
    return L


class Sched:
    """arrays: ka, kb, p_lo, p_n, piece of the groups; groups: the same as [(ka, kb, p_lo, p_n, piece)]"""
    _bufs = None

    @property
    def groups(self):
        return list(zip(*(a.tolist() for a in self.arrays)))

    def __init__(self, L, curve, n, c, budget, k=None, p_off=0, tab=None, no_glv=False, host=False, serial=False, n_cu=256):
        if Sched._bufs is None:
            Sched._bufs = ((C.c_int32 * CAP)(), (C.c_int32 * CAP)(), (C.c_uint64 * CAP)(), (C.c_uint64 * CAP)(), (C.c_int32 * CAP)(),
                           (C.c_int32 * 6)())
        ka, kb, lo, cnt, piece, flags = Sched._bufs
        plan = (C.c_int32 * 2)()
        assert L.gs_plan(curve, n, c, int(no_glv), plan), (curve, n, c, no_glv)
        self.c, self.K, self.L_log = c, plan[0], plan[1]
        self.leaves_one_level = L.gs_leaves_one_level(curve, n, c, int(no_glv)) == 1
        self.k_lo, self.k_hi = k if k is not None else (0, self.K)
        tab_T, tab_lo, tab_n = tab if tab is not None else (0, 0, 0)
        g = L.gs_schedule(curve, n_cu, budget, n, p_off, c, int(no_glv), self.k_lo, self.k_hi, tab_T, tab_lo, tab_n, int(host),
                          int(serial), CAP, ka, kb, lo, cnt, piece, flags)
        assert g > 0, g
        self.arrays = tuple(np.ctypeslib.as_array(a)[:g].astype(np.int64) for a in (ka, kb, lo, cnt, piece))
        self.wpg = flags[0]
        self.tables, self.split_points, self.piped, self.share_digits, self.lone = (bool(f) for f in flags[1:6])


# ---------------------------------------------------------------------------------------------- named cases
# window_bytes (msm_plan.hip), 256 CUs: BLS12-377 under a window above 16 bits 293 bytes per point, + 2^L_log * 160 + 2^(L_log - 7)
# * 2048 for the buckets; Ed-on-BLS12-377 113 bytes per point.  A workspace gets room = budget / 2.

def test_two_groups_share_one_digit_launch(lib):
    """BLS12-377, 2^22 points, c = 18: 127 = 7 * 18 + 1 folds, K = 7, 2^18 buckets.  A window takes 2^22 * 293 + 46 MB = 1.28 GB, the
    room of 100 GiB holds all seven; a window of 2^18 buckets does not fit the LDS: 16 at most; two groups from 2^22 points:
    wpg = ceil(7 / 2) = 4."""
    s = Sched(lib, BLS377, 1 << 22, 18, 200 * GiB)
    assert s.K == 7
    assert s.groups == [(0, 4, 0, 1 << 22, -1), (4, 7, 0, 1 << 22, -1)]
    assert (s.wpg, s.tables, s.split_points, s.piped, s.share_digits, s.lone) == (4, False, False, False, True, False)


def test_two_groups_on_four_tables(lib):
    """the same on window tables over the same range, tab_T = 4: the tables stay"""
    n = 1 << 22
    s = Sched(lib, BLS377, n, 18, 200 * GiB, tab=(4, 0, n))
    assert s.groups == [(0, 4, 0, n, -1), (4, 7, 0, n, -1)]
    assert (s.wpg, s.tables, s.split_points, s.share_digits, s.lone) == (4, True, False, True, False)


def test_tight_budget_cuts_every_window_into_three_ranges(lib):
    """budget 1 GiB, room 537 MB: one window (1.28 GB) does not fit, wpg = 1; halves take 2^21 * 293 + 46 MB = 661 MB, thirds
    1 398 102 * 293 + 46 MB = 456 MB: three ranges per window, window-major"""
    n = 1 << 22
    s = Sched(lib, BLS377, n, 18, 1 * GiB)
    want = [(k, k + 1, n * q // 3, n * (q + 1) // 3 - n * q // 3, -1) for k in range(7) for q in range(3)]
    assert len(want) == 21 and s.groups == want
    assert (s.wpg, s.tables, s.split_points, s.share_digits) == (1, False, True, False)


def test_edwards_one_level_sort_keeps_eighteen_windows(lib):
    """Ed-on-BLS12-377, 2^20 points, c = 14: K = 252 / 14 = 18; 2^13 buckets fit the LDS and 2^20 entries stay below the 2^22 of
    the radix split: no cap of 16; one group below 2^22 points"""
    s = Sched(lib, ED377, 1 << 20, 14, 200 * GiB)
    assert s.K == 18
    assert s.groups == [(0, 18, 0, 1 << 20, -1)]
    assert (s.wpg, s.split_points, s.share_digits, s.lone) == (18, False, False, False)


def test_edwards_on_tables_runs_two_groups(lib):
    """Ed-on-BLS12-377, 2^20 points, c = 17 on tables: K = ceil(252 / 17) = 15; on tables two groups from 2^20 points:
    wpg = ceil(15 / 2) = 8 = tab_T.  The Edwards digit kernel is not shared."""
    n = 1 << 20
    s = Sched(lib, ED377, n, 17, 200 * GiB, tab=(8, 0, n))
    assert s.K == 15
    assert s.groups == [(0, 8, 0, n, -1), (8, 15, 0, n, -1)]
    assert (s.wpg, s.tables, s.split_points, s.share_digits) == (8, True, False, False)


@pytest.mark.parametrize("tab", [None, (3, 0, 1 << 24)])
def test_lone_window_is_split_into_two_halves(lib, tab):
    """BLS12-377, 2^24 points, c = 21 (K = 6), windows [2, 3): a single Weierstrass window from 2^24 points runs as two halves on
    the two streams, which leaves the tables"""
    n = 1 << 24
    s = Sched(lib, BLS377, n, 21, 200 * GiB, k=(2, 3), tab=tab)
    assert s.K == 6
    assert s.groups == [(2, 3, 0, n // 2, -1), (2, 3, n // 2, n // 2, -1)]
    assert (s.tables, s.split_points, s.share_digits, s.lone) == (False, True, False, False)
    assert Sched(lib, BLS377, n, 21, 200 * GiB, k=(2, 3), tab=tab, serial=True).lone


def test_tables_of_another_range_are_left_but_still_cap_the_groups(lib):
    """BLS12-377, 2^22 points from point 4096, c = 18 on tables that start at point 0: the plain path, under the wpg the tables
    gave (min(4, tab_T = 2): the rules read the tables before they are dropped)"""
    n = 1 << 22
    s = Sched(lib, BLS377, n, 18, 200 * GiB, p_off=4096, tab=(2, 0, n))
    assert s.groups == [(0, 2, 0, n, -1), (2, 4, 0, n, -1), (4, 6, 0, n, -1), (6, 7, 0, n, -1)]
    assert (s.wpg, s.tables, s.split_points, s.share_digits) == (2, False, False, False)


def test_piped_host_scalars_run_piece_by_piece(lib):
    """BLS12-377, 2^24 host scalars, c = 21, windows [0, 6): pieces end at n / 8, n / 2 and n (whole 16 MiB chunks of 2^19
    scalars); wpg = ceil(6 / 2) = 3 caps the one group a piece below 2^22 points would run as: every piece runs [0, 3), [3, 6)"""
    n = 1 << 24
    s = Sched(lib, BLS377, n, 21, 200 * GiB, host=True)
    ends = [0, 1 << 21, 1 << 23, 1 << 24]
    want = [(k, k + 3, ends[q], ends[q + 1] - ends[q], q) for q in range(3) for k in (0, 3)]
    assert s.groups == want and [g[4] for g in s.groups] == [0, 0, 1, 1, 2, 2]
    assert (s.wpg, s.piped, s.split_points, s.share_digits, s.tables) == (3, True, True, False, False)
    # the workspace forces its own ranges: the pipelined upload gives way
    s = Sched(lib, BLS377, n, 21, 4 * GiB, host=True)
    assert not s.piped and all(g[4] == -1 for g in s.groups) and s.split_points and len(s.groups) > 6


# ---------------------------------------------------------------------------------------------- the grid

BUDGETS = (64 * MiB, 512 * MiB, 4 * GiB, 32 * GiB, 250 * GiB)


def _plans(lib, curve, n):
    """every (c, no_glv) make_plan accepts"""
    plan = (C.c_int32 * 2)()
    out = [(c, ng) for ng in ((0,) if curve == ED377 else (0, 1)) for c in range(1, 26) if lib.gs_plan(curve, n, c, ng, plan)]
    assert {c for c, _ in out} == set(range(2, 25)) and (curve == ED377 or (4, 1) in out and (3, 1) not in out)
    return out


def _check(s, te, n, p_off, tab, budget, wb):
    """wb(points) = window_bytes of the call's plan"""
    nwin = s.k_hi - s.k_lo
    ka, kb, lo, cnt, piece = s.arrays
    tag = (te, n, s.c, budget, tab, (s.k_lo, s.k_hi), [a[:4].tolist() for a in s.arrays])
    assert (s.k_lo <= ka).all() and (ka < kb).all() and (kb <= s.k_hi).all() and (cnt > 0).all(), tag
    assert ((piece >= 0) == s.piped).all(), tag
    # every (window, point) pair lies in exactly one group: per window, the groups' ranges in order tile [0, n)
    width = kb - ka
    win = np.repeat(ka, width) + (np.arange(width.sum()) - np.repeat(np.cumsum(width) - width, width))
    w_lo, w_cnt = np.repeat(lo, width), np.repeat(cnt, width)
    order = np.lexsort((w_lo, win))
    win, w_lo, w_end = win[order], w_lo[order], (w_lo + w_cnt)[order]
    first = np.r_[True, win[1:] != win[:-1]]
    assert (np.unique(win) == np.arange(s.k_lo, s.k_hi)).all(), tag
    assert (w_lo[first] == 0).all() and (w_lo[~first] == w_end[:-1][~first[1:]]).all() and (w_end[np.r_[first[1:], True]] == n).all(), tag
    assert width.max() <= 128 and width.max() <= s.wpg, tag
    # a group that may leave the one-level sort, and any group of a plan on tables: a WinSplit of 16 entries
    if s.leaves_one_level or tab is not None:          # (the library's own rule, through the shim: msm_internal.h)
        assert width.max() <= 16, tag
    if tab is not None:
        assert width.max() <= tab[0], tag           # (kept or dropped: the cap is read before the drop)
    whole = bool(((lo == 0) & (cnt == n)).all())
    assert s.split_points == (not whole), tag
    if s.tables:
        assert tab is not None and whole and (tab[1], tab[2]) == (p_off, n), tag
    # the budget: a group's windows fit a workspace's room, unless point_pieces stopped at one of its own limits
    for size in np.unique(cnt).tolist():
        over = (cnt == size) & (width.astype(object) * wb(size) > budget // 2)
        if over.any():
            pieces = int(np.count_nonzero(win == ka[over][0]))
            assert (width[over] == 1).all() and (pieces == 256 or n // pieces <= 4096), (tag, pieces)
    if s.share_digits:
        (ka0, kb0, lo0, n0, q0), (ka1, kb1, lo1, n1, q1) = s.groups
        assert not te and not s.piped and q0 == q1 == -1 and (lo0, n0) == (lo1, n1) and kb0 == ka1 and kb1 - ka0 <= 16, tag
    assert s.lone == (len(ka) == 1 and (nwin == 1 or s.tables)), tag


@pytest.mark.parametrize("lg", range(10, 30))
@pytest.mark.parametrize("curve", [BLS377, ED377])
def test_schedule_invariants(lib, curve, lg):
    te = curve == ED377
    n = (1 << lg) + (37 if lg % 3 == 0 else 0)      # (odd sizes too: ranges n q / pieces that do not divide)
    p_off = 4096
    seen = set()
    for c, no_glv in _plans(lib, curve, n):
        wb_cache = {}

        def wb(cnt):
            if cnt not in wb_cache:
                wb_cache[cnt] = lib.gs_window_bytes(curve, 256, cnt, c, no_glv)
            return wb_cache[cnt]

        plan = (C.c_int32 * 2)()
        lib.gs_plan(curve, n, c, no_glv, plan)
        K = plan[0]
        k_ranges = {(0, K), (K // 2, K // 2 + 1), (min(1, K - 1), K)}
        for budget in BUDGETS:
            for tab in (None, (-(-K // 2), p_off, n), (K, p_off, n), (-(-K // 2), 0, n), (K, p_off, n + 1)):
                for k in k_ranges:
                    for host in ((False, True) if lg >= 24 else (False,)):
                        s = Sched(lib, curve, n, c, budget, k=k, p_off=p_off, tab=tab, no_glv=no_glv, host=host)
                        _check(s, te, n, p_off, tab, budget, wb)
                        seen.add((s.tables, s.split_points, s.piped, s.share_digits, len(s.arrays[0]) > 2))
    # the grid reaches the branches it is there for
    assert any(t for t, *_ in seen) and any(m for *_, m in seen), seen
    if lg >= 14:
        assert any(sp for _, sp, *_ in seen), seen
    if lg >= 24:
        assert any(p for _, _, p, _, _ in seen), seen
    if not te and 22 <= lg <= 27:           # (from 2^28 points no call is cut into just two window groups under these budgets)
        assert any(sh for _, _, _, sh, _ in seen), seen
