"""Degenerate point multisets (tests/degenerate_inputs.py) through every MSM entry point, plan and curve: `-m gpu`.

Points generated on the GPU are pairwise distinct, so the other suites mostly meet two finite points with different x.  Here
every input is full of equal points (P + P in every round of the tree), opposite points (P - P), identities (at both ends, a
run longer than a wave, every 8th point of the rest) and, where the path has no endomorphism, points of even order outside the
subgroup (a doubling with denominator 0 inside a lane's batched inversion).  Each cell of

    run x {default, 5, 13, 16, 18, 21, no_glv at 13}  |  window tables x two windows, and the chains whose rows of DIFFERENT
    windows are equal or opposite points of one merged bucket  |  run_batch (fused)  |  run_narrow x three formats x two
    windows, run_batch_narrow  |  bucket-range shards and a points split cutting a run, through window_sums and
    combine_groups_host  |  compressed reload

runs the four scalar layouts at n = 5000 (default plan c = 16) and n = 1000 (c = 8) on all seven curves, and is compared for
exact equality with ONE scaling of G computed from the known discrete logs (tests/test_degenerate_inputs.py proves that value
equal to the oracle's plain sum).  One context per curve for the whole module.

Cells that are not there, and why:
  * no path refuses any of these options with MSM_ERR_ARG on any curve, so no cell is replaced by an asserted refusal;
  * window tables exist from 4096 points (tables_eligible): the tables cells run at n = 5000; at n = 1000 the test asserts that
    msm_precompute builds nothing and the run stays right on the plain path.  The chains are padded to 4096 points with zero
    scalars for the same reason;
  * the Edwards path has no endomorphism, hence no no_glv cell; its table windows are 14 and 17;
  * `cancel` on narrow values is v, -v: it exists in the signed formats only (uint64 runs the other three layouts);
  * the torsion inputs run only without the endomorphism (phi(T) != lambda T): no_glv, run_narrow, the Edwards path.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degenerate_inputs as D  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (5000, 1000)
WINDOWS = (None, 5, 13, 16, 18, 21)
TORSION_N = 4200          # >= 4096: the same input also runs on window tables, through k_table_next's even-order branch
_CASES = {}


class Case:
    def __init__(self, name):
        from montgomery_amd.api import MsmContext

        self.name, self.cv = name, D.CURVE_TABLE[name]
        self.ctx = MsmContext(self.cv.cid)
        assert self.ctx.coord_bytes == self.cv.cb
        self._wire, self._sc, self._nar = {}, {}, {}

    def key(self, res):
        return (res.x, res.y) if self.cv.te else res.as_tuple()

    def load(self, n):
        """The layout's points as the current point set, checked against the curve equation (dropping any window tables)."""
        lay = D.layout(n)
        if n not in self._wire:
            self._wire[n] = self.cv.wire(D.points_of(self.cv, lay.entries))
        self.ctx.set_points(self._wire[n], check_curve=True)
        assert self.ctx.n_points == n
        return lay

    def load_raw(self, points, **kw):
        if kw:
            self.ctx.load_points(self.cv.wire(points), **kw)
        else:
            self.ctx.set_points(self.cv.wire(points), check_curve=True)

    def scalars(self, n, kind):
        """(32-byte scalars, expected value) of one scalar layout; computed once."""
        if (n, kind) not in self._sc:
            lay = D.layout(n)
            sc = D.scalars(self.cv, lay, kind)
            self._sc[n, kind] = (O.scalars_to_bytes(sc), D.expected(self.cv, lay.entries, sc))
        return self._sc[n, kind]

    def narrow(self, n, kind, fmt):
        """(run_narrow arguments, expected value) of one layout restated on narrow values."""
        import numpy as np

        from montgomery_amd import narrow as N

        if (n, kind, fmt) not in self._nar:
            lay = D.layout(n)
            vals = D.narrow_values(self.cv, lay, kind, fmt)
            width, signed, bits, _ = D.NARROW_FORMATS[fmt]
            if fmt == "int32_b16":
                args = (np.array(vals, dtype=np.int32), {"bits": bits})
            elif fmt == "uint64":
                args = (np.array(vals, dtype=np.uint64), {})
            else:
                args = (N.pack(vals, width, signed, self.cv.q), {"bits": bits, "width": width, "signed": signed})
            self._nar[n, kind, fmt] = (args, D.expected(self.cv, lay.entries, vals))
        return self._nar[n, kind, fmt]


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for cs in _CASES.values():
        cs.ctx.close()
    _CASES.clear()


def table_windows(name):
    return (14, 17) if D.CURVE_TABLE[name].te else (16, 18)


def narrow_kinds(fmt):
    return [k for k in D.SCALAR_LAYOUTS if k != "cancel" or D.NARROW_FORMATS[fmt][1]]


# ---------------------------------------------------------------------------------------------- run

RUN_CELLS = [(name, n, c, False) for name in D.NAMES for n in NS for c in WINDOWS] + \
            [(name, n, 13, True) for name in D.NAMES if not D.CURVE_TABLE[name].te for n in NS]


@pytest.mark.parametrize("name,n,c,no_glv", RUN_CELLS)
def test_run(name, n, c, no_glv):
    """The plain path under every sort: the one-level sort (5, 13, 16), the bin split (18 and 21: a folded top window on the
    126-bit curves, a short one on the 127-bit ones, plain on Edwards), the default plan, and without GLV."""
    cs = case(name)
    cs.load(n)
    for kind in D.SCALAR_LAYOUTS:
        sb, exp = cs.scalars(n, kind)
        res, info = cs.ctx.run(sb, c=c, no_glv=no_glv, no_tables=True)
        assert cs.key(res) == exp, (kind, info)
        assert not info["tables"] and (c is None or info["c"] == c)
    assert cs.scalars(n, "generic")[1] != cs.cv.zero


# ---------------------------------------------------------------------------------------------- window tables

@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", D.NAMES)
def test_tables(name, which):
    """All windows in one set of buckets: rows 2^(c k) P of equal points are equal again, those of identities identities
    (k_table_next), and the merged buckets hold the runs of every window at once."""
    cs, n, c = case(name), 5000, table_windows(name)[which]
    cs.load(n)
    cc, K, nbytes = cs.ctx.precompute(n, c=c)
    assert (cc, K) == (c, cs.cv.plan_k(c)) and nbytes > 0
    for kind in D.SCALAR_LAYOUTS:
        sb, exp = cs.scalars(n, kind)
        res, info = cs.ctx.run(sb, c=c)
        assert info["tables"] and info["K"] == K, info
        assert cs.key(res) == exp, (kind, info)


@pytest.mark.parametrize("name", D.NAMES)
def test_tables_need_4096_points(name):
    """n = 1000: msm_precompute builds nothing and the call stays on the plain path, with the right value."""
    cs, n, c = case(name), 1000, table_windows(name)[0]
    cs.load(n)
    assert cs.ctx.precompute(n, c=c) == (0, 0, 0)
    for kind in D.SCALAR_LAYOUTS:
        sb, exp = cs.scalars(n, kind)
        res, info = cs.ctx.run(sb, c=c)
        assert not info["tables"] and cs.key(res) == exp, (kind, info)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", D.NAMES)
def test_chain_on_tables_and_plain(name, which):
    """P, 2^c P, 2^2c P, ... under scalars d 2^(c (K - 1 - i)): on tables K equal points (and K alternating +-) of DIFFERENT windows
    in the merged bucket d, which no plain plan can produce; the same input on the plain path and at c = 13."""
    cs, c = case(name), table_windows(name)[which]
    points, sc, exp, K, d = D.chain(name, c, 4096)
    cs.load_raw(points)
    sb = O.scalars_to_bytes(sc)
    assert cs.ctx.precompute(4096, c=c)[:2] == (c, cs.cv.plan_k(c))
    res, info = cs.ctx.run(sb, c=c)
    assert info["tables"] and cs.key(res) == exp, (K, d, info)
    res, info = cs.ctx.run(sb, c=c, no_tables=True)
    assert not info["tables"] and cs.key(res) == exp, (K, d, info)
    res, info = cs.ctx.run(sb, c=13, no_tables=True)
    assert cs.key(res) == exp, (K, d, info)
    res, info = cs.ctx.run(sb, no_tables=True)
    assert cs.key(res) == exp, (K, d, info)


# ---------------------------------------------------------------------------------------------- run_batch

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_run_batch(name, n):
    """One call, the four scalar layouts as its elements plus an all-zero one, over the one point set; fused."""
    cs = case(name)
    cs.load(n)
    vecs = [cs.scalars(n, kind)[0] for kind in D.SCALAR_LAYOUTS] + [bytes(32 * n)]
    exps = [cs.scalars(n, kind)[1] for kind in D.SCALAR_LAYOUTS] + [cs.cv.zero]
    single_rounds = 0
    for v, exp in zip(vecs, exps):
        res, info = cs.ctx.run(v, no_tables=True)
        assert cs.key(res) == exp
        single_rounds += info["rounds"]
    got = cs.ctx.run_batch(vecs)
    for kind, (res, info), exp in zip(D.SCALAR_LAYOUTS + ("zero",), got, exps):
        assert cs.key(res) == exp, (kind, info)
    # the fused path is what ran: the elements share the tree rounds (element by element every call has its own)
    assert got[0][1]["rounds"] < single_rounds and not got[0][1]["tables"], (got[0][1], single_rounds)


# ---------------------------------------------------------------------------------------------- run_narrow

@pytest.mark.parametrize("fmt", sorted(D.NARROW_FORMATS))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_run_narrow(name, n, fmt):
    """No GLV and a digit kernel of its own: one value per run, v / -v, independent values, 90 % zeros."""
    cs = case(name)
    cs.load(n)
    for kind in narrow_kinds(fmt):
        (arr, kw), exp = cs.narrow(n, kind, fmt)
        for c in (None, 13):
            res, info = cs.ctx.run_narrow(arr, c=c, **kw)
            assert cs.key(res) == exp, (kind, c, info)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_run_batch_narrow(name, n):
    cs = case(name)
    cs.load(n)
    kinds = narrow_kinds("int32_b16")
    arrs = [cs.narrow(n, kind, "int32_b16")[0][0] for kind in kinds]
    single_rounds = sum(cs.ctx.run_narrow(a, bits=16)[1]["rounds"] for a in arrs)
    got = cs.ctx.run_batch_narrow(arrs, bits=16)
    for kind, (res, info) in zip(kinds, got):
        assert cs.key(res) == cs.narrow(n, kind, "int32_b16")[1], (kind, info)
    # the fused path is what ran: the elements share the tree rounds
    assert got[0][1]["rounds"] < single_rounds, (got[0][1], single_rounds)


# ---------------------------------------------------------------------------------------------- shards

@pytest.mark.parametrize("c", [13, 18])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_bucket_range_shards(name, n, c):
    """G = 3 uneven bucket ranges of every window, summed per window by combine_groups_host: a run of one point falls into one
    shard as a whole, the other two see an empty bucket there."""
    from montgomery_amd.distributed import combine_groups_host

    cs = case(name)
    cs.load(n)
    cc, K = cs.ctx.plan(n, c, no_tables=True)
    assert (cc, K) == (c, cs.cv.plan_k(c))
    for kind in D.SCALAR_LAYOUTS:
        sb, exp = cs.scalars(n, kind)
        parts = b"".join(cs.ctx.window_sums(sb, n, 0, K, c=c, bucket_shard=(g, 3))[0] for g in range(3))
        assert combine_groups_host(parts, 3, K, c, cs.cv.cid) == exp, kind


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_points_split_through_a_run(name, n):
    """A two-way points split whose cut goes through the longest run of one point at an odd offset: which pairs of the run are
    doublings changes on both sides (point_lo), the sum does not."""
    from montgomery_amd.distributed import combine_groups_host

    cs = case(name)
    lay = cs.load(n)
    # the 257-run at n = 5000; at n = 1000 the runs stop at 129 and the cut goes through that one
    start, length, _ = next(r for r in lay.runs if r[1:] == (257 if n >= 5000 else 129, "eq"))
    off = 101 if length == 257 else 51
    cut = start + off
    assert off % 2 == 1 and (length - off) % 2 == 0 and start < cut < start + length
    for c in (13, None):
        cc, K = cs.ctx.plan(n, c, no_tables=True)
        for kind in D.SCALAR_LAYOUTS:
            sb, exp = cs.scalars(n, kind)
            g0 = cs.ctx.window_sums(sb[: 32 * cut], cut, 0, K, c=cc, point_lo=0)[0]
            g1 = cs.ctx.window_sums(sb[32 * cut :], n - cut, 0, K, c=cc, point_lo=cut)[0]
            assert combine_groups_host(g0 + g1, 2, K, cc, cs.cv.cid) == exp, (kind, cc)


# ---------------------------------------------------------------------------------------------- compressed reload

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", D.NAMES)
def test_compressed_reload(name, n):
    """The layout through the compressed encoding and the subgroup check: the same rows, the same MSM."""
    cs = case(name)
    cs.load(n)
    raw = cs.ctx.get_points(0, n)
    comp = cs.ctx.get_points(0, n, compressed=True)
    assert len(comp) == cs.cv.cb * n
    assert cs.ctx.load_points(comp, compressed=True, validate="subgroup") == n
    assert cs.ctx.get_points(0, n) == raw
    sb, exp = cs.scalars(n, "dbl")
    res, info = cs.ctx.run(sb, no_tables=True)
    assert cs.key(res) == exp, info


# ---------------------------------------------------------------------------------------------- points outside the subgroup

@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_torsion_points_in_run(name):
    """Points of order 2 (and 4 on the Edwards curve) among ordinary ones, two of them adjacent under one scalar: on BLS12-377
    (p - 1, 0) + (p - 1, 0) is a doubling with denominator 2 y = 0 inside a lane's batched inversion, which must not poison the
    lane's other pairs.  Accepted by validate="curve", refused by "subgroup"."""
    from montgomery_amd import MsmError

    cs = case(name)
    points, sc, exp = D.torsion(name, TORSION_N)
    with pytest.raises(MsmError) as e:
        cs.load_raw(points, validate="subgroup")
    assert e.value.code == 3 and e.value.bad_index == 3
    cs.load_raw(points, validate="curve")
    sb = O.scalars_to_bytes(sc)
    no_glv = not cs.cv.te
    for c in (13, 16, 18):
        res, info = cs.ctx.run(sb, c=c, no_glv=no_glv, no_tables=True)
        assert not info["tables"] and cs.key(res) == exp, (c, info)
    # on window tables: a point of order 2 doubles to the identity in k_table_next, a point of order 4 after two doublings
    c = 16
    cs.ctx.precompute(TORSION_N, c=c, no_glv=no_glv)
    assert cs.ctx.tables_info()[0] == c
    res, info = cs.ctx.run(sb, c=c, no_glv=no_glv)
    assert info["tables"] and cs.key(res) == exp, info


@pytest.mark.parametrize("fmt", ["uint64", "int32_b16"])
@pytest.mark.parametrize("name", ["bls377", "ed377"])
def test_torsion_points_in_run_narrow(name, fmt):
    import numpy as np

    cs = case(name)
    points, vals, exp = D.torsion(name, TORSION_N, fmt)
    cs.load_raw(points, validate="curve")
    arr, kw = (np.array(vals, dtype=np.uint64), {}) if fmt == "uint64" else (np.array(vals, dtype=np.int32), {"bits": 16})
    for c in (None, 13):
        res, info = cs.ctx.run_narrow(arr, c=c, **kw)
        assert cs.key(res) == exp, (c, info)


# ---------------------------------------------------------------------------------------------- no entry at all

@pytest.mark.parametrize("name", ["bls377", "pallas", "ed377"])
def test_all_zero_scalars(name):
    """A whole MSM whose window groups have no entry: every bucket sum is the identity the finish writes (from 4096 buckets on
    behind its ordering pass), and the reduction over them -- bit-sliced at the default window -- gives the identity.  On the
    plain path and on window tables (which exist from 4096 points)."""
    cs, n = case(name), 4096
    cs.load_raw(list(D.pool(name)[0]) * (n // D.POOL))
    sb = bytes(32 * n)
    res, info = cs.ctx.run(sb, no_tables=True)
    assert not info["tables"] and cs.key(res) == cs.cv.zero, info
    assert cs.ctx.precompute(n)[2] > 0
    res, info = cs.ctx.run(sb)
    assert info["tables"] and cs.key(res) == cs.cv.zero, info


# ---------------------------------------------------------------------------------------------- one larger shape

@pytest.mark.parametrize("name", ["bls381", "bn254", "vesta"])
def test_2p18_copies_of_one_point(name):
    """One larger shape per limb count and reduction kind (13 limbs; 9 limbs with the general and with the special reduction row),
    c = 18, plain path: 2^18 copies of one point under one scalar -- the bin split's "parts of heavy bins" with every pair a
    doubling -- and P, -P alternating, where every pair cancels."""
    cs, n = case(name), 1 << 18
    cv = cs.cv
    pts, logs = D.pool(name)
    s = O.prng_ints(f"gpu/degenerate/{name}/2p18", 1, cv.q)[0]
    sb = s.to_bytes(32, "little") * n
    cs.ctx.set_points(cv.wire([pts[9], pts[9]]) * (n // 2), check_curve=True)
    res, info = cs.ctx.run(sb, c=18, no_tables=True)
    assert cs.key(res) == cv.scale_g(n * s * logs[9]), info
    assert info["c"] == 18 and not info["tables"], info
    cs.ctx.set_points(cv.wire([pts[9], cv.neg(pts[9])]) * (n // 2), check_curve=True)
    res, info = cs.ctx.run(sb, c=18, no_tables=True)
    assert cs.key(res) == cv.zero, info
