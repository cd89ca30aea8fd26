"""tests/crafted_buckets.py proved on the CPU before tests/test_gpu_bucket_sums.py relies on it: at K = 2, L = 8 every fill
pattern's expected window sums -- one scaling of G per window, from the discrete logs -- equal the direct sum
sum_l l sum_(e in bucket) P_e formed with the oracle's point arithmetic (aff_add / aff_scale; te_add / te_scale on the Edwards
curve), the merged group sum equals its Horner combination, and off / elems describe the buckets the pattern promises.  No GPU."""
import numpy as np
import pytest

import crafted_buckets as B
from degenerate_inputs import CURVE_TABLE

K, L, TC = 2, 8, 2
CURVES = ("bls377", "pallas", "ed377")


def direct_sums(cr):
    """P_k = sum_l l * (sum of the bucket's points), with the curve's own additions and scalings"""
    cv = cr.cv
    out = []
    for k in range(cr.K):
        acc = cv.zero
        for l in range(1, cr.L + 1):
            bsum = cv.zero
            for j in cr.bucket(k, l):
                bsum = cv.add(bsum, cr.points[j])
            acc = cv.add(acc, cv.scale(l, bsum))
        out.append(acc)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_pool_points_have_the_logs_they_claim(curve):
    cv = CURVE_TABLE[curve]
    pts, logs = B.base_pool(curve)
    assert len(pts) == B.POOL == 32 and pts[B.IDENT] == cv.zero and logs[B.IDENT] == 0
    for j in (0, B.N_RANDOM - 1, B.N_RANDOM, B.GEN, B.POOL - 1):
        assert cv.scale_g(logs[j]) == pts[j], j
    for j in range(2 * B.N_RANDOM):
        assert pts[B.neg_index(j)] == cv.neg(pts[j]) and (logs[j] + logs[B.neg_index(j)]) % cv.q == 0
        assert cv.add(pts[j], pts[B.neg_index(j)]) == cv.zero
    assert len(set(pts[:2 * B.N_RANDOM])) == 2 * B.N_RANDOM
    wire = cv.wire(pts)
    assert len(wire) == 2 * cv.cb * B.POOL
    ident = wire[2 * cv.cb * B.IDENT:2 * cv.cb * (B.IDENT + 1)]
    assert ident == ((0).to_bytes(cv.cb, "little") + (1).to_bytes(cv.cb, "little") if cv.te else bytes(2 * cv.cb))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("pattern", sorted(B.PATTERNS))
def test_expected_values_are_the_direct_sums(pattern, curve):
    cr = B.PATTERNS[pattern](curve, K, L, TC)
    cv = cr.cv
    assert cr.off[0] == 0 and len(cr.off) == K * L + 1 and (np.diff(cr.off.astype(np.int64)) >= 0).all()
    assert len(cr.elems) == cr.off[-1] == cr.counts.sum()
    assert [len(cr.bucket(k, l)) for k in range(K) for l in range(1, L + 1)] == cr.counts.tolist()
    direct = direct_sums(cr)
    assert cr.expected() == direct
    for stride in (4, 3):                         # log2 L + 1: the plain plan; log2 L: the folded top window
        assert cr.expected_group(stride) == B.horner(cv, direct, stride) == cv.add(direct[0], cv.scale(1 << stride, direct[1]))


@pytest.mark.parametrize("curve", CURVES)
def test_patterns_fill_the_buckets_they_promise(curve):
    cv = CURVE_TABLE[curve]
    pts, logs = B.base_pool(curve)
    make = lambda name: B.PATTERNS[name](curve, K, L, TC)      # noqa: E731
    cnt = lambda cr: cr.counts.reshape(K, L)                   # noqa: E731

    cr = make("random")
    assert cr.counts.min() == 0 and cr.counts.max() == 3 and set(np.unique(B.random(curve, 4, 256).elems).tolist()) == set(range(B.POOL))
    cr = make("one_point")
    assert (cr.counts == 1).all() and len(set(cr.elems.tolist())) == 1
    d = cr.logs[int(cr.elems[0])]
    assert cr.window_logs() == [d * (L * (L + 1) // 2) % cv.q] * K
    cr = make("all_empty")
    assert cr.off.tolist() == [0] * (K * L + 1) and cr.expected() == [cv.zero] * K
    cr = make("one_window_empty")
    assert (cnt(cr)[1] == 0).all() and cnt(cr)[0].min() >= 1 and cr.expected()[1] == cv.zero != cr.expected()[0]
    for name, ls in (("only_first", [1]), ("only_last", [L]), ("one_chunk", [5, 6])):
        cr = make(name)
        for k in range(K):
            assert np.nonzero(cnt(cr)[k])[0].tolist() == [l - 1 for l in ls] and cr.expected()[k] != cv.zero
    assert np.nonzero(B.one_chunk(curve, 1, 64, 8).counts)[0].tolist() == list(range(40, 48))      # chunk 5 of 8 buckets
    cr = make("cancel_in_chunk")
    for k in range(K):
        for ch in range(L // TC):
            (a,), (b,) = cr.bucket(k, ch * TC + 1), cr.bucket(k, ch * TC + 2)
            assert b == B.neg_index(a) and cv.add(cr.points[a], cr.points[b]) == cv.zero
    cr4 = B.cancel_in_chunk(curve, 1, 16, 4)
    assert cr4.counts.tolist() == [1, 1, 0, 0] * 4
    cr = make("cancel_chunk_pairs")
    for k in range(K):
        heads = [cr.bucket(k, ch * TC + 1) for ch in range(L // TC)]
        assert all(len(h) == 1 for h in heads) and cnt(cr)[k].sum() == L // TC
        assert all(heads[i + 1][0] == B.neg_index(heads[i][0]) for i in range(0, L // TC, 2))
    cr = make("zero_window")
    assert cr.expected()[0] == cv.zero and cr.window_logs()[0] == 0 and cr.expected()[1] != cv.zero
    assert B.POOL in cr.bucket(0, 1) and len(cr.points) == B.POOL + 1 and cv.scale_g(cr.logs[B.POOL]) == cr.points[B.POOL]
    # deep: enough buckets for every count to meet every kind of content
    cr = B.deep(curve, 1, 64)
    assert sorted(set(cr.counts.tolist())) == list(B.DEEP_COUNTS) and cr.counts.max() == B.FINISH_BINS
    seen = set()
    for b in range(64):
        el, kind = cr.bucket(0, b + 1), (b // len(B.DEEP_COUNTS)) % 3
        seen.add((len(el), kind))
        if kind == 0:
            assert len(set(el)) <= 1
        elif kind == 1 and len(el) >= 3:
            assert el[1] == B.neg_index(el[0]) and el[2] < B.N_RANDOM and (len(el) < 6 or el[:3] == el[3:6])
        elif kind == 2 and el:
            assert el[0] == el[len(el) // 2] == el[-1] == B.IDENT
    assert {c for c, k in seen if k == 0} == {c for c, k in seen if k == 1} == set(B.DEEP_COUNTS)


# ---------------------------------------------------------------------------------------------- flags and the tree's patterns

def direct_sums_flagged(cr):
    """direct_sums with the payload bits applied to every element: bit 0 negates the point, bit 1 takes (beta x, y)"""
    cv = cr.cv
    out = []
    for k in range(cr.K):
        acc = cv.zero
        for l in range(1, cr.L + 1):
            b = k * cr.L + l - 1
            bsum = cv.zero
            for e in range(int(cr.off[b]), int(cr.off[b + 1])):
                P, f = cr.points[int(cr.elems[e])], int(cr.flags[e])
                if f & 2 and P is not None:
                    P = (cv.B.beta * P[0] % cv.p, P[1])
                if f & 1 and P != cv.zero:
                    P = cv.neg(P)
                bsum = cv.add(bsum, P)
            acc = cv.add(acc, cv.scale(l, bsum))
        out.append(acc)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_flagged_elements_stand_for_the_logs_they_claim(curve):
    cv = CURVE_TABLE[curve]
    if not cv.te:
        G = (cv.B.gx, cv.B.gy)
        assert (cv.B.beta * G[0] % cv.p, G[1]) == cv.scale_g(cv.B.lam)       # the beta x line of a row is lambda times its point
    cr = B.tree_threshold(curve, 9, flags=True, bucket=5)
    assert cr.flags is not None and set(cr.flags.tolist()) == ({0, 1} if cv.te else {0, 1, 2, 3})
    small = B.Crafted("flagged", curve, K, L, cr.counts[:K * L], cr.elems[:int(cr.off[K * L])], flags=cr.flags[:int(cr.off[K * L])])
    assert small.expected() == direct_sums_flagged(small)
    plain = B.Crafted("plain", curve, K, L, small.counts, small.elems, flags=np.zeros(len(small.elems), dtype=np.uint8))
    assert plain.expected() == direct_sums(plain) == B.Crafted("plain", curve, K, L, small.counts, small.elems).expected()


def test_tree_patterns_fill_the_buckets_they_promise():
    curve = "bls377"
    cr = B.tree_threshold(curve, 65)
    assert (cr.K, cr.L) == (2, 64) and cr.counts.max() == 65 and np.sort(cr.counts)[-2] <= 3 and cr.flags is None
    cr = B.tree_every_size(curve, 258)
    assert cr.L == 512 and cr.counts[:259].tolist() == list(range(259)) and cr.counts[259:].sum() == 0
    assert B.tree_every_size(curve, 258, reverse=True).counts[:259].tolist() == list(range(258, -1, -1))
    for extra in (0, 1):
        cr = B.tree_desc_blocks(curve, extra)
        out = (cr.counts + 3) // 4                                           # outputs of the first tail round at logG = 1
        start = np.concatenate([[0], np.cumsum(out)])
        run, d = B.TREE_EMPTY_RUN, 2 * B.TREE_EMPTY_RUN + 1
        assert int(start[-1]) % B.TREE_BLOCK == extra
        assert cr.counts[:run].sum() == 0 and cr.counts[-run:].sum() == 0 and cr.counts[run + 1:d].sum() == 0
        assert start[run + 1] == start[d] == B.TREE_BLOCK                    # D starts a block, behind a run of empty buckets
        assert out[d] >= 4 * B.TREE_BLOCK and start[d + 1] - start[d] == out[d]
    cr = B.tree_scan_blocks(curve, 3, 2048)
    deep = np.nonzero(cr.counts >= 65)[0].tolist()
    assert deep == [0, 308, 309, 310, 311, 4095, 4096, 6143] and len(set(cr.counts[deep].tolist())) == len(deep)
    cr = B.tree_sparse(curve, 2, 1 << 14, every=1 << 10)
    assert np.count_nonzero(cr.counts) == 32 + 1 + 2 and cr.counts[-1] > 0 and np.sort(cr.counts)[-2:].tolist() == [70, 71]
    cr = B.tree_degenerate(curve, 128)
    P = 3
    assert cr.bucket(0, 1) == [P] * 128 and cr.bucket(0, 2)[:4] == [P, B.neg_index(P)] * 2 and cr.bucket(0, 3)[:4] == [P, P, B.neg_index(P), B.neg_index(P)]
    assert cr.bucket(0, 4)[1::2] == [B.IDENT] * 64 and B.IDENT not in cr.bucket(0, 4)[0::2] and cr.bucket(0, 5) == [B.IDENT] * 128
    d = cr.logs[P]
    assert cr.window_logs()[0] == (128 * d + sum(cr.logs[j] for j in cr.bucket(0, 4)) * 4 + sum(cr.logs[j] for j in cr.bucket(0, 6)) * 6) % cr.cv.q
    assert [int(B.tree_few(curve, n).counts.sum()) for n in (0, 1, 2)] == [0, 1, 2]
    cr = B.tree_equal(curve, 1 << 10, 64, odd_one=0)
    assert (cr.counts == 64).all() and B.IDENT not in cr.elems
