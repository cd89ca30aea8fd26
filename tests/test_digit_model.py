"""tests/digit_model.py proved on the CPU before tests/test_gpu_digits.py compares the digit kernels with it: the words of every
configuration of the GPU sweep add up to the value they stand for (with the endomorphism: s0 + lambda s1 = s mod q, both halves
below 2^glv_max_bits), agree with the oracle's signed_digits where no fold and no shard is in play, the plan restates make_plan
as the library's own documented plans and tests/crafted_digits.py have it, the shards partition the entries, the narrow formats
decode as documented, and the scalars tests/crafted_digits.py crafts for chosen digits map back to those digits.  No GPU."""
import numpy as np
import pytest

import crafted_digits as D
import digit_model as M
from oracle import msm_oracle as O

SIGN = M.SIGN
CS = range(1, 26)   # 1 and 25: refused


def entry_words(mag, neg, pl):
    words, clamped = M.recode(mag, neg, pl)
    assert not clamped
    return words


def test_plan_restates_make_plan():
    """K and the fold against the plans the library documents and tests/crafted_digits.py pins (BLS12-377 after GLV: 127 = 7 * 18 +
    1 = 6 * 21 + 1), against crafted_digits.Plan for every curve and window, and the refusals of make_plan."""
    for curve, c, no_glv, K, fold in (("bls377", 16, False, 8, False), ("bls377", 18, False, 7, True), ("bls377", 21, False, 6, True),
                                      ("bls377", 22, False, 6, False), ("bn254", 21, False, 6, True), ("bls381", 22, False, 6, False),
                                      ("pallas", 16, False, 8, False), ("ed377", 21, False, 12, False), ("ed377", 2, False, 126, False),
                                      ("bls377", 23, True, 11, True), ("bls377", 4, True, 64, False), ("bls381", 16, True, 16, False)):
        pl = M.plan(curve, c, no_glv)
        assert (pl.K, pl.fold) == (K, fold), (curve, c, no_glv)
    for curve in M.NAMES:
        te = M.CURVE_TABLE[curve].te
        for c in CS:
            pl = M.plan(curve, c)
            assert (pl is None) == (c < 2 or c > 24)
            assert (M.plan(curve, c, no_glv=True) is None) == (c < 2 or c > 24 or (c < 4 and not te))
            if pl is None:
                continue
            assert pl.K == M.CURVE_TABLE[curve].plan_k(c)
            assert pl.K <= 126 and pl.K * c + (1 if pl.fold else 0) >= pl.bits
            try:
                ref = D.Plan(curve, c)
            except AssertionError:
                continue   # (crafted_digits has no crafted values for this plan: their top window would stay empty)
            assert (pl.K, pl.fold, pl.L_log, pl.bits, pl.per_point) == (ref.K, ref.fold, ref.L_log, ref.bits, ref.per_point)
            for G in (2, 3, 8):
                for g in range(G):
                    assert M.plan(curve, c, shard=(g, G)).ranges == [tuple(r) for r in D.shard_ranges(ref, g, G)]
            assert M.plan(curve, c, shard=(2, 2)) is None
    # narrow: b = the declared bits; 128 bits under c = 2 would be 65 windows
    assert M.plan("bls377", 2, narrow_bits=128) is None and M.plan("bls377", 2, narrow_bits=127).K == 64
    pl = M.plan("bls377", 18, narrow_bits=36)
    assert (pl.K, pl.fold, pl.glv, pl.per_point) == (2, True, False, 2)
    assert M.plan("ed377", 18, narrow_bits=36).fold is False and M.plan("ed377", 18, narrow_bits=36).K == 3
    ref = D.Plan("bls377", 21, D.NARROW_BITS)
    assert (M.plan("bls377", 21, narrow_bits=D.NARROW_BITS).K, ref.fold) == (ref.K, False)


def test_every_weierstrass_curve_with_a_fold_has_it_in_the_sweep():
    """127 bits after GLV fold at c = 18 and 21 (BLS12-377, BN254, Grumpkin); 128 bits (BLS12-381, Pallas, Vesta) never do: 127 is
    prime.  Without GLV only BLS12-377 folds: 253 = 11 * 23."""
    for curve in M.NAMES:
        cv = M.CURVE_TABLE[curve]
        folds = [(c, ng) for c in range(18, 25) for ng in (False, True) if M.plan(curve, c, ng).fold]
        if cv.te:
            want = []
        elif cv.glv.max_bits == 126:
            want = [(18, False), (21, False)] + ([(23, True)] if curve == "bls377" else [])
        else:
            assert cv.glv.max_bits == 127
            want = []
        assert sorted(folds) == sorted(want), curve


@pytest.mark.parametrize("curve", M.NAMES)
def test_words_add_up_to_the_value(curve):
    cv = M.CURVE_TABLE[curve]
    q = cv.q
    for c in CS:
        for no_glv in (False, True):
            pl = M.plan(curve, c, no_glv)
            if pl is None:
                continue
            low, high = M.full_scalars(pl, n_random=60)
            assert all(0 <= s < q for s in low) and all(q <= s < M.TWO256 for s in high) and len(high) >= 7
            for raw in low + high:
                ent, flags = M.scalar_entries(raw, pl)
                assert ("ge_q" in flags) == (raw >= q) and len(ent) == pl.per_point
                vals = []
                for mag, neg in ent:
                    words = entry_words(mag, neg, pl)
                    assert len(words) == pl.K and M.word_value(words, c) == (-mag if neg else mag)
                    assert all((w & ~SIGN) <= (1 << pl.L_log) for w in words) and SIGN not in words   # no "-0"
                    top = words[-1] & ~SIGN
                    assert top <= (1 << pl.top_bits if pl.fold or pl.kind() == "short" else 1 << (c - 1))
                    vals.append(-mag if neg else mag)
                    if not pl.fold:
                        # the oracle recodes the magnitude: its sign is the carry alone, also where a zero digit passes one on
                        assert [(w & ~SIGN, bool(w & SIGN)) for w in words] == [(l, (ng != neg) and l != 0) for l, ng in O.signed_digits(mag, c, pl.K)]
                if pl.glv:
                    assert (vals[0] + cv.B.lam * vals[1] - raw) % q == 0
                    assert abs(vals[0]) < (1 << cv.glv.max_bits) and abs(vals[1]) < (1 << cv.glv.max_bits)
                else:
                    assert vals[0] == raw % q and (cv.te or vals[1] == 0)


def test_patterns_reach_the_edges():
    """The raw digits the issue names really occur: L - 1, L, L + 1, 2^c - 1 in every window that has room for them, a carry through
    every window, and a top window that holds the carry alone."""
    for c, K, fold, b in ((16, 8, False, 126), (21, 6, True, 126), (13, 10, False, 126), (22, 6, False, 127), (7, 36, False, 251)):
        pat = M.patterns(c, K, fold, b)
        L = 1 << (c - 1)
        raw = {(j, (v >> (c * j)) & ((1 << c) - 1)) for v in pat for j in range(K)}
        for j in range(K):
            room = b - c * j
            for d in (L - 1, L, L + 1, (1 << c) - 1):
                if d < (1 << room):
                    assert (j, d) in raw, (c, j, d)
        assert (1 << b) - 1 in pat and (1 << (c * (K - 1))) - 1 in pat
        # all-ones below the top window: -1 at the bottom, the carry through every window (magnitude 0: no entry), +1 on top
        words, _ = M.recode((1 << (c * (K - 1))) - 1, False, type("P", (), {"c": c, "K": K, "fold": fold}))
        assert words == [1 | SIGN] + [0] * (K - 2) + [1]


@pytest.mark.parametrize("curve", M.NAMES)
def test_sweep_scalars_put_the_edges_into_the_words(curve):
    """What the construction is for, read off the model's words: in every window whose bits the crafted values control -- all below
    the top one without the endomorphism, those below bit 120 of a half with it (above, (+-h0 +- lambda h1) mod q no longer
    decomposes into the same halves) -- the words L (raw digit L), L - 1 (raw L - 1), -(L - 1) (raw L + 1) and -1 (raw 2^c - 1)
    occur on the first entry of some scalar."""
    for c, no_glv in ((4, False), (7, True), (13, False), (16, False), (16, True), (21, False), (23, True)):
        pl = M.plan(curve, c, no_glv)
        low, high = M.full_scalars(pl, n_random=0)
        words, _ = M.model_words(pl, low + high)
        L = 1 << (c - 1)
        first = words[:, ::pl.per_point]
        for k in range(pl.K - 1):
            if pl.glv and c * (k + 1) > 120:
                break
            seen = set(first[k].tolist())
            assert {L, L - 1, (L - 1) | SIGN, 1 | SIGN} <= seen, (curve, c, no_glv, k)
        if pl.glv:
            second = words[:, 1::2]
            assert {L, (L - 1) | SIGN} <= set(second[0].tolist())


@pytest.mark.parametrize("curve,c,no_glv", [("bls377", 16, False), ("bls377", 20, False), ("bls377", 21, False), ("bls381", 13, False),
                                            ("ed377", 14, False), ("ed377", 21, False), ("bls377", 23, True), ("vesta", 22, False)])
def test_shards_partition_the_entries(curve, c, no_glv):
    """G = 2, 3, 8 on plans with a full, a short and a folded top window: every non-zero word of the unsharded model is kept by
    exactly one shard, unchanged, and lies in that shard's cut."""
    base = M.plan(curve, c, no_glv)
    low, _ = M.full_scalars(base, n_random=100)
    full, rc = M.model_words(base, low)
    assert rc == M.MSM_OK
    for G in (2, 3, 8):
        kept = np.zeros(full.shape, dtype=np.int64)
        for g in range(G):
            pl = M.plan(curve, c, no_glv, shard=(g, G))
            got, _ = M.model_words(pl, low)
            assert ((got == 0) | (got == full)).all()
            kept += got != 0
            for k in range(pl.K):
                idx = (got[k][got[k] != 0] & ~np.uint32(SIGN)).astype(np.int64) - 1
                assert ((idx >= pl.ranges[k][0]) & (idx < pl.ranges[k][1])).all()
        assert (kept == (full != 0)).all()
    kinds = {M.plan(cv, cc, ng).kind() for cv, cc, ng in (("ed377", 14, False), ("bls377", 20, False), ("bls377", 21, False))}
    assert kinds == {"full", "short", "folded"}


def test_narrow_formats_decode_as_documented():
    q = O.BLS12_377.q
    assert M.decode_narrow(0xFF, 1, 7, True, q) == (1, True, False)             # -1
    assert M.decode_narrow(0x80, 1, 7, True, q) == (128, True, False)            # -2^7: the negative extreme is in range
    assert M.decode_narrow(0x80, 1, 7, False, q) == (0, False, True)             # +2^7 is not
    assert M.decode_narrow(0x80, 1, 8, False, q) == (128, False, False)
    assert M.decode_narrow(0xFFFF, 2, 16, False, q) == (0xFFFF, False, False)
    assert M.decode_narrow(0x8000, 2, 8, True, q) == (0, False, True)            # the width's minimum under fewer bits
    assert M.decode_narrow(q - 5, 32, 8, True, q) == (5, True, False)
    assert M.decode_narrow(q - 5, 32, 8, False, q) == (0, False, True)
    assert M.decode_narrow(q - (1 << 128), 32, 128, True, q) == (1 << 128, True, False)
    assert M.decode_narrow(1 << 128, 32, 128, True, q) == (0, False, True)       # below 2^129: positive, and out of range
    assert M.decode_narrow(q, 32, 128, True, q)[2] and M.decode_narrow(M.TWO256 - 1, 32, 128, False, q)[2]
    for width in M.WIDTHS:
        for signed in (False, True):
            for v in (0, 1, 5, -1, -5):
                if v < 0 and not signed:
                    continue
                mag, neg, bad = M.decode_narrow(M.encode_narrow(v, width, q), width, 3, signed, q)
                assert (mag, neg, bad) == (abs(v), v < 0, False)


@pytest.mark.parametrize("width", M.WIDTHS)
def test_narrow_words_add_up_to_the_value(width):
    for signed in (False, True):
        full = M.width_full_bits(width, signed)
        for bits in (1, 7, 8, 31, 32, 36, 63, 64, 127, 128):
            if bits > full:
                continue
            for c in (2, 5, 13, 16, 18, 21):
                for curve in ("bls377", "ed377"):
                    pl = M.plan(curve, c, narrow_bits=bits)
                    if pl is None:
                        assert (bits + c) // c > 64
                        continue
                    ok, bad = M.narrow_values(pl, width, bits, signed, n_random=20)
                    assert -(1 << bits) in ok or not signed
                    assert (1 << bits) in bad or (1 << bits) > ((1 << (8 * width - (1 if signed else 0))) - 1 if width < 32 else M.TWO256)
                    for v in ok + bad:
                        ent, flags = M.scalar_entries(M.encode_narrow(v, width, pl.cv.q), pl, (width, bits, signed))
                        assert ("range" in flags) == (v in bad)
                        mag, neg = ent[0]
                        assert (-mag if neg else mag) == (0 if v in bad else v)
                        words = entry_words(mag, neg, pl)
                        assert M.word_value(words, c) == (0 if v in bad else v)
                        assert (words[-1] & ~SIGN) <= (1 << pl.L_log)
                        assert len(ent) == pl.per_point and (pl.te or ent[1] == (0, False))
    assert M.plan("bls377", 18, narrow_bits=36).fold


CRAFTED = [D.Case("exact_edges", c=21, n=1 << 18), D.Case("short_top", c=20, n=1 << 18), D.Case("full_bin", c=16, n=D.RADIX_N),
           D.ED_CASES[0], D.NARROW_CASE, D.BN254_CASE]


@pytest.mark.parametrize("cs", CRAFTED, ids=[cs.id for cs in CRAFTED])
def test_crafted_scalars_map_back_to_their_digits(cs):
    """The inverse direction, which tests/crafted_digits.py already has: digits -> scalar.  The model must give the digits back."""
    cr = cs.make()
    dp = cr.plan
    pl = M.plan(cs.curve, cs.c, narrow_bits=cs.narrow_bits)
    assert (pl.K, pl.fold) == (dp.K, dp.fold)
    pool = cr.pool_scalars()
    fmt = (16, cs.narrow_bits, False) if cs.narrow_bits else None
    got, rc = M.model_words(pl, pool, fmt)
    assert rc == M.MSM_OK
    want = np.zeros_like(got)
    dig = np.asarray(cr.digits, dtype=np.int64)                       # (pool, halves, K) signed
    enc = (np.abs(dig) | np.where(dig < 0, SIGN, 0)).astype(np.uint32)
    for h in range(dp.halves):
        want[:, h::pl.per_point] = enc[:, h, :].T
    assert (got == want).all()
