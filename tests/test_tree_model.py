"""tests/tree_model.py proved on the CPU before tests/test_gpu_tree.py relies on it.  The whole tree runs on integers, every
element being the discrete log it stands for: regular rounds add neighbours, tail rounds add by the model's descriptors, the
finish adds what is left.  Every bucket must come out as the sum of its entries -- a descriptor that names a wrong operand, or a
present bit set at a bucket's last odd element, adds a neighbour's entry -- and when the tail rounds stop no bucket may hold more
than FINISH_MAX elements.  No GPU."""
import numpy as np
import pytest

import crafted_buckets as B
import tree_model as T


def check(counts, logG, c, reported_max=0, seed=0):
    counts = np.asarray(counts, dtype=np.int64)
    plan = T.TreePlan(counts, logG, c, reported_max)
    values = np.random.default_rng(seed).integers(1, 1 << 20, size=int(counts.sum()))      # never 0: a wrong operand shows
    sums, left = T.simulate(plan, values)
    start = np.concatenate([[0], np.cumsum(counts)])
    csum = np.concatenate([[0], np.cumsum(values)])
    assert (sums == csum[start[1:]] - csum[start[:-1]]).all()
    assert left.max(initial=0) <= plan.FINISH_MAX
    assert ((left > 0) == (counts > 0)).all()
    return plan


def test_the_scanned_quantities():
    n = np.arange(0, 70)
    for logG in (1, 2, 3, 5, 10):
        G = 1 << logG
        assert (T.scan_quantity(n, logG, 0) == -(-n // G) * G).all()
        for r in range(6):
            assert (T.scan_quantity(n, logG, 1 + r) == -(-(-(-n // G)) // (1 << r))).all()
    # RT: the smallest r with 2^r >= ceil(max / G)
    assert [T.tail_rounds(m, 1) for m in (0, 1, 2, 3, 4, 5, 8, 9, 64, 65, 66, 67)] == [0, 0, 0, 1, 1, 2, 2, 3, 5, 6, 6, 6]
    assert T.tail_rounds(1 << 20, 10) == 10 and T.tail_rounds((1 << 20) + 1, 10) == 11 and T.pscan_nq(65, 1) == 8
    assert T.thresholds(17) == (32, 1 << 21) and T.thresholds(18) == (64, 1 << 23)


def test_cursor_and_tail_tables_of_a_small_vector():
    p = T.TreePlan([0, 1, 5, 0, 8, 3], 2, 16)
    assert p.cursor.tolist() == [0, 0, 4, 12, 12, 20, 24] and p.total_slots == 24 and p.max_bucket == 8 and p.RT == 1
    assert p.tail_off.tolist() == [[0, 0, 1, 3, 3, 5, 6], [0, 0, 1, 2, 2, 3, 4]] and p.tail_tot == [6, 4]
    assert p.r_stop == 0 and p.rounds == 2 and p.n_pairs == 12 + 6
    ia, present = p.desc(1)
    assert ia.tolist() == [0, 1, 3, 5] and present.tolist() == [False, True, True, False]
    assert p.desc_words(1).tolist() == [0, 3, 7, 10]
    empty = T.TreePlan(np.zeros(16, dtype=np.int64), 3, 21)
    assert (empty.total_slots, empty.RT, empty.r_stop, empty.rounds, empty.n_pairs) == (0, 0, 0, 0, 0) and empty.tail_off.shape == (1, 17)


@pytest.mark.parametrize("c,F", [(16, 32), (21, 64)])
@pytest.mark.parametrize("logG", [1, 2, 3, 5, 10])
def test_r_stop_at_the_threshold(c, F, logG):
    G = 1 << logG
    for deep, r_stop in ((F * G, 0), (F * G + 1, 1), (2 * F * G, 1), (2 * F * G + 1, 2)):
        counts = np.array([2, 0, deep, 3, 1])
        assert check(counts, logG, c).r_stop == r_stop
        # an over-reported maximum runs the rounds the reported bucket would need
        assert check(counts, logG, c, reported_max=2 * deep).r_stop == r_stop + 1
        over = check(counts, logG, c, reported_max=64 * deep)
        assert over.RT == T.tail_rounds(64 * deep, logG) and over.r_stop == r_stop + 6


def test_r_stop_by_the_pair_count():
    # 2^17 buckets of 64 entries at G = 2: 32 elements each, which the finish takes -- but the first tail round has 2^21 outputs
    p = T.TreePlan(np.full(1 << 17, 64), 1, 16)
    assert p.tail_tot[1] == 1 << 21 and p.r_stop == 1 and p.tail_tot[2] == 1 << 20
    counts = np.full(1 << 17, 64)
    counts[1000] = 60
    p = T.TreePlan(counts, 1, 16)
    assert p.tail_tot[1] == (1 << 21) - 1 and p.r_stop == 0
    assert T.TreePlan(np.full(1 << 17, 64), 1, 21).r_stop == 0      # the class of c >= 18 asks for 2^23


@pytest.mark.parametrize("seed", range(8))
def test_random_size_vectors(seed):
    rng = np.random.default_rng(seed)
    logG = int(rng.integers(1, 6))
    nb = int(rng.integers(1, 700))
    counts = rng.integers(0, 5, size=nb)
    deep = rng.integers(0, nb, size=3)
    counts[deep] = rng.integers(1, 70 << logG, size=3)
    for c in (16, 21):
        p = check(counts, logG, c, seed=seed)
        check(counts, logG, c, reported_max=int(p.max_bucket * 3 + 1), seed=seed)


def test_crafted_size_vectors():
    for logG, F, c in ((1, 32, 16), (3, 32, 16), (1, 64, 21)):
        G = 1 << logG
        top = 4 * F * G + G
        for reverse in (False, True):
            p = check(B.tree_every_size("bls377", top, reverse).counts, logG, c)
            assert p.r_stop == 3 and p.max_bucket == top
    check(B.tree_one_bucket("bls377", 1000).counts, 1, 16)
    check(B.tree_last_deep("bls377", 200).counts, 1, 16)
    check(B.tree_scan_blocks("bls377", 3, 2048).counts, 1, 16)
    check(B.tree_degenerate("bls377").counts, 3, 21)
    for entries in (0, 1, 2):
        p = check(B.tree_few("bls377", entries).counts, 1, 16)
        assert p.rounds == (1 if entries else 0) and p.total_slots == (2 if entries else 0)
