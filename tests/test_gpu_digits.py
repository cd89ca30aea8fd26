"""The twelve digit kernels word for word against tests/digit_model.py, through msm_test_digits (`-m gpu`): the entry builds the
plan, stages the scalars and launches k_digits / k_te_digits / k_digits_narrow<W> / k_te_digits_narrow<W> or their _batch forms
through the pipeline's own launch code, and hands back the window words `magnitude | sign << 31` -- nothing sorts them, so a wrong
digit is a failed comparison here and never a bucket index.  Every comparison is exact.  The model and the scalars are proved on
the CPU by tests/test_digit_model.py.

    sizes    c <= 16: n = 1037 -- 256-thread blocks, a ragged last one (narrow widths 1 and 2: 4 and 2 scalars per lane);
             c >= 17: n = 8229 -- the bin-split launch, two slices of 4115 points under 1024-thread blocks, so that a slice ends
             inside a block's stride, and inside the dword a lane of the 1- and 2-byte formats loads
    scalars  per configuration the edge values of digit_model.full_scalars / narrow_values (the raw digits L - 1, L, L + 1, 2^c - 1 in
             every window, carries through all windows, a top window of the carry alone, q - 1, q, 2 q + 3, 2^256 - 1, lambda, the
             formats' extremes) and randoms from O.prng_ints, repeated over the n points
    refused  configurations make_plan refuses must come back as MSM_ERR_ARG: nothing is skipped
"""
import functools

import numpy as np
import pytest

import digit_model as M

pytestmark = pytest.mark.gpu

N_SMALL, N_BIG = 1000 + 37, 8192 + 37
CS = range(1, 26)                      # 1 and 25: refused
NARROW_BITS = (1, 7, 8, 18, 31, 32, 36, 63, 64, 127, 128)   # 18 = 1 * 18, 36 = 2 * 18, 63 = 3 * 21: folded plans under c = 18 / 21
NARROW_CS = (2, 5, 13, 16, 18, 21)
SIGN = np.uint32(M.SIGN)


def n_of(c):
    return N_SMALL if c <= 16 else N_BIG


@pytest.fixture(scope="module")
def ctx_of():
    from montgomery_amd.api import MsmContext

    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = MsmContext(M.CURVE_TABLE[curve].cid)
        return made[curve]

    yield get
    for c in made.values():
        c.close()


def refused(call):
    """the call must be answered with MSM_ERR_ARG"""
    from montgomery_amd import MsmError

    with pytest.raises(MsmError) as e:
        call()
    assert e.value.code == M.MSM_ERR_ARG, e.value
    return True


def spread(words_u, idx, per):
    """model words of the distinct scalars -> the words of a call whose point i holds distinct scalar idx[i]"""
    cols = (per * np.asarray(idx)[:, None] + np.arange(per)[None, :]).ravel()
    return words_u[:, cols]


def same(got, want, what):
    """exact equality, naming the first word that differs"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        k, j = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} words differ; first at window row {k}, word {j}: "
                             f"kernel {int(got[k, j]):#x}, model {int(want[k, j]):#x}")


@functools.lru_cache(maxsize=None)
def full_case(curve, c, no_glv):
    """(plan, scalars below q, scalars from q up, model words of all of them, model words' return code) -- computed once"""
    pl = M.plan(curve, c, no_glv)
    low, high = M.full_scalars(pl, room=n_of(c))
    words, rc = M.model_words(pl, low + high)
    assert rc == M.MSM_OK and len(low) + len(high) <= n_of(c)
    return pl, low, high, words


def full_call(ctx, pl, raws, idx, no_glv=None, **kw):
    data = M.to_bytes(raws, 32)[idx]
    res = ctx.test_digits(data, c=pl.c, no_glv=pl.no_glv if no_glv is None else no_glv, **kw)
    assert (res["c"], res["K"], res["fold"]) == (pl.c, pl.K, pl.fold), (res["c"], res["K"], res["fold"])
    return res


# ---------------------------------------------------------------------------------------------- full-width scalars

@pytest.mark.parametrize("curve", M.NAMES)
def test_full_width_sweep(curve, ctx_of):
    """Every c in 2 .. 24 with and without no_glv (1 and 25, and no_glv under c < 4: refused), non-strict over all scalars and
    strict over those below q; a scalar >= q under strict is MSM_ERR_SCALAR, each of them on its own at c = 13."""
    ctx, cv = ctx_of(curve), M.CURVE_TABLE[curve]
    folded, n_refused = set(), 0
    for c in CS:
        for no_glv in (False, True):
            if M.plan(curve, c, no_glv) is None:
                n_refused += refused(lambda: ctx.test_digits(np.zeros((N_SMALL, 32), np.uint8), c=c, no_glv=no_glv))
                continue
            pl, low, high, words = full_case(curve, c, no_glv)
            n, m, m_low = n_of(c), len(low) + len(high), len(low)
            idx = np.arange(n) % m
            res = full_call(ctx, pl, low + high, idx, no_glv=no_glv)   # (the Edwards curve has no split: the option changes nothing)
            assert res["rc"] == M.MSM_OK
            same(res["words"], spread(words, idx, pl.per_point), f"{curve} c={c} no_glv={no_glv}")
            if pl.fold:
                folded.add((c, no_glv))
            # strict: the scalars below q alone pass and give the same words; with those from q up the call is refused
            idx_low = np.arange(n) % m_low
            res = full_call(ctx, pl, low, idx_low, strict=True)
            assert res["rc"] == M.MSM_OK
            same(res["words"], spread(words, idx_low, pl.per_point), f"{curve} c={c} no_glv={no_glv} strict")
            assert full_call(ctx, pl, low + high, idx, strict=True)["rc"] == M.MSM_ERR_SCALAR
            if c == 13:
                for j, s in enumerate(high):
                    one = idx_low.copy()
                    one[(97 * j + 5) % n] = m_low + j
                    res = full_call(ctx, pl, low + high, one, strict=True)
                    assert res["rc"] == M.MSM_ERR_SCALAR, hex(s)
                    same(res["words"], spread(words, one, pl.per_point), f"{curve} c=13 strict with {s:#x}")
    assert n_refused == (4 if cv.te else 4 + 2)
    want_folds = {(c, ng) for c in range(18, 25) for ng in (False, True) if M.plan(curve, c, ng).fold}
    assert folded == want_folds
    if curve == "bls377":
        assert {(18, False), (21, False)} <= folded
    if not cv.te and cv.glv.max_bits == 126:
        assert folded, "a curve whose halves have 127 bits folds at c = 18 and c = 21"


def test_ed377_reduces_up_to_55_times(ctx_of):
    """Scalars up to 2^256 - 1 on Ed-on-BLS12-377: 2^256 < 56 q, so the reduction subtracts q up to 55 times."""
    cv = M.CURVE_TABLE["ed377"]
    top = (M.TWO256 - 1) // cv.q
    assert top in (54, 55)
    raws = [m * cv.q + r for m in range(top + 1) for r in (0, 1, cv.q - 1) if m * cv.q + r < M.TWO256] + [M.TWO256 - 1]
    pl = M.plan("ed377", 12)
    words, rc = M.model_words(pl, raws)
    idx = np.arange(N_SMALL) % len(raws)
    res = full_call(ctx_of("ed377"), pl, raws, idx)
    assert res["rc"] == rc == M.MSM_OK
    same(res["words"], spread(words, idx, 1), "ed377 multiples of q")


RANGE_CONFIGS = ((3, False), (13, False), (16, False), (16, True), (18, False), (21, False), (23, True), (24, False))


@pytest.mark.parametrize("curve", M.NAMES)
def test_window_ranges(curve, ctx_of):
    """[0, K), single windows, [1, K - 1) and the top window alone are the same rows of the full call; and a call over the
    elements [first, first + n) of a longer array reads exactly those (the others would fail a strict call)."""
    ctx = ctx_of(curve)
    for c, no_glv in RANGE_CONFIGS:
        pl, low, high, words = full_case(curve, c, no_glv)
        n, K = n_of(c), pl.K
        idx = np.arange(n) % (len(low) + len(high))
        want = spread(words, idx, pl.per_point)
        whole = full_call(ctx, pl, low + high, idx)["words"]
        same(whole, want, f"{curve} c={c} all windows")
        singles = range(K) if K <= 12 else sorted({0, 1, 2, K // 2, K - 3, K - 2, K - 1})
        ranges = [(0, K)] + [(k, k + 1) for k in singles] + ([(1, K - 1)] if K > 2 else [])
        for lo, hi in ranges:
            res = full_call(ctx, pl, low + high, idx, k_lo=lo, k_hi=hi)
            assert res["rc"] == M.MSM_OK
            same(res["words"], whole[lo:hi], f"{curve} c={c} windows [{lo}, {hi})")
        for lo, hi in ((0, K + 1), (K, K + 1), (2, 2), (3, 1)):
            refused(lambda: full_call(ctx, pl, low + high, idx, k_lo=lo, k_hi=hi))
        # a range of a longer array: scalars >= q in front of it and behind it, under strict
        idx_low = np.arange(n) % len(low)
        data = np.concatenate([np.full((3, 32), 0xFF, np.uint8), M.to_bytes(low, 32)[idx_low], np.full((2, 32), 0xFF, np.uint8)])
        res = ctx.test_digits(data, n=n, first=3, c=c, no_glv=pl.no_glv, strict=True)
        assert res["rc"] == M.MSM_OK
        same(res["words"], spread(words, idx_low, pl.per_point), f"{curve} c={c} first=3")


def shard_configs(curve):
    """One window of the one-level launch and one of the bin-split launch per kind of top window -- full, short, folded -- the
    curve has at all (BLS12-377 has no full one: 127 is prime and 254 = 2 * 127), with the endomorphism where that gives it."""
    out = {}
    for no_glv in (False, True):
        for c in (13, 14, 16, 12, 15, 20, 21, 18, 22, 17, 24, 23):
            pl = M.plan(curve, c, no_glv)
            out.setdefault((pl.kind(), c > 16), (c, no_glv))
    return sorted(out.values())


@pytest.mark.parametrize("curve", M.NAMES)
def test_bucket_shards(curve, ctx_of):
    """G = 2, 3, 8: the words of shard g are the model's; every non-zero entry of the unsharded call is kept by exactly one
    shard, with the same word, inside the range the model's cut gives."""
    ctx = ctx_of(curve)
    kinds = set()
    for c, no_glv in shard_configs(curve):
        pl, low, high, words = full_case(curve, c, no_glv)
        kinds.add(pl.kind())
        n = n_of(c)
        idx = np.arange(n) % len(low)
        whole = full_call(ctx, pl, low, idx)["words"]
        same(whole, spread(words, idx, pl.per_point), f"{curve} c={c} unsharded")
        for G in (2, 3, 8):
            kept = np.zeros(whole.shape, dtype=np.int64)
            for g in range(G):
                ps = M.plan(curve, c, no_glv, shard=(g, G))
                res = full_call(ctx, ps, low, idx, bucket_shard=g, bucket_shards=G)
                assert res["rc"] == M.MSM_OK
                got = res["words"]
                same(got, spread(M.model_words(ps, low)[0], idx, pl.per_point), f"{curve} c={c} shard {g}/{G}")
                assert ((got == 0) | (got == whole)).all()
                kept += got != 0
                for k in range(pl.K):
                    b = (got[k][got[k] != 0] & ~SIGN).astype(np.int64) - 1
                    assert ((b >= ps.ranges[k][0]) & (b < ps.ranges[k][1])).all(), (c, g, G, k)
            assert (kept == (whole != 0)).all(), (c, G)
        refused(lambda: full_call(ctx, pl, low, idx, bucket_shard=2, bucket_shards=2))
    cv = M.CURVE_TABLE[curve]
    have = {M.plan(curve, c, ng).kind() for c in range(4, 25) for ng in (False, True)}
    assert kinds == have and "short" in kinds and (("full" in kinds) == (curve != "bls377"))
    assert ("folded" in kinds) == (not cv.te and cv.glv.max_bits == 126)


# ---------------------------------------------------------------------------------------------- narrow scalars

def narrow_bytes(values, width, q):
    return M.to_bytes([M.encode_narrow(v, width, q) for v in values], width)


@pytest.mark.parametrize("signed", (False, True), ids=("unsigned", "signed"))
@pytest.mark.parametrize("width", M.WIDTHS)
@pytest.mark.parametrize("curve", M.NAMES)
def test_narrow(curve, width, signed, ctx_of):
    """Every bits value the width holds under six windows: the accepted values (0, +-1, 2^bits - 1, -2^bits, the width's extremes,
    the recoding's edges) give the model's words; a refused one (+2^bits, an extreme beyond the bits) fails the call with
    MSM_ERR_SCALAR, each on its own, and counts as 0.  Widths 1 and 2 also as ranges that start at element 1, 2, 3 of a longer
    array whose other elements are refused values: inside the dword a lane loads, ending inside another."""
    ctx, cv = ctx_of(curve), M.CURVE_TABLE[curve]
    q = cv.q
    folds = 0
    for bits in NARROW_BITS:
        if bits > M.width_full_bits(width, signed):
            refused(lambda: ctx.test_digits(np.zeros((8, width), np.uint8), width=width, bits=bits, signed=signed, c=13))
            continue
        for c in NARROW_CS:
            pl = M.plan(curve, c, narrow_bits=bits)
            if pl is None:
                refused(lambda: ctx.test_digits(np.zeros((8, width), np.uint8), width=width, bits=bits, signed=signed, c=c))
                continue
            folds += pl.fold
            n = n_of(c)
            fmt = (width, bits, signed)
            ok, bad = M.narrow_values(pl, width, bits, signed)
            stored = [M.encode_narrow(v, width, q) for v in ok + bad]
            n_ok = len(ok)
            if width == 32:
                ext = M.stored_extremes_32(cv, signed)
                stored = [s for s, r in ext if not r] + stored + [s for s, r in ext if r]
                n_ok += sum(not r for _, r in ext)
            # (a width whose every value lies inside the bits -- 8 unsigned bits in a byte, 7 signed ones -- has nothing to refuse)
            any_bad = len(stored) > n_ok
            assert len(stored) <= n and (any_bad or (width < 32 and bits == M.width_full_bits(width, signed)))
            words, rc_all = M.model_words(pl, stored, fmt)
            assert rc_all == (M.MSM_ERR_SCALAR if any_bad else M.MSM_OK) and M.model_words(pl, stored[:n_ok], fmt)[1] == M.MSM_OK
            assert not words[:, pl.per_point * n_ok:].any()       # a refused value counts as 0
            table = M.to_bytes(stored, width)
            poison = table[n_ok:] if any_bad else table[:1]
            firsts = (0, 1, 2, 3) if (width <= 2 and c in (5, 18)) else (0,)
            for first in firsts:
                idx = np.arange(n) % n_ok
                data = np.concatenate([poison[np.arange(first) % len(poison)], table[idx], poison[np.arange(3) % len(poison)]])
                res = ctx.test_digits(data, n=n, first=first, width=width, bits=bits, signed=signed, c=c)
                assert (res["c"], res["K"], res["fold"]) == (pl.c, pl.K, pl.fold)
                assert res["rc"] == M.MSM_OK, (bits, c, first)
                same(res["words"], spread(words, idx, pl.per_point), f"{curve} width {width} bits {bits} signed {signed} c={c} first={first}")
            # all values, the refused ones among them
            idx = np.arange(n) % len(stored)
            res = ctx.test_digits(table[idx], width=width, bits=bits, signed=signed, c=c)
            assert res["rc"] == rc_all
            same(res["words"], spread(words, idx, pl.per_point), f"{curve} width {width} bits {bits} signed {signed} c={c} with refused values")
            if c == NARROW_CS[1]:
                # every refused value on its own, at every position of a lane's load
                for j in range(n_ok, len(stored)):
                    one = np.arange(9) % n_ok
                    one[j % 9] = j
                    res = ctx.test_digits(table[one], width=width, bits=bits, signed=signed, c=c)
                    assert res["rc"] == M.MSM_ERR_SCALAR, (bits, hex(stored[j]))
                    same(res["words"], spread(words, one, pl.per_point), f"{curve} width {width} bits {bits}: {stored[j]:#x} alone")
    if not cv.te and width >= 4:
        assert folds, "no folded narrow plan in the sweep"
    refused(lambda: ctx.test_digits(np.zeros((8, 3), np.uint8), width=3, bits=8, c=8))
    refused(lambda: ctx.test_digits(np.zeros((8, width), np.uint8), width=width, bits=1, signed=signed, c=8, bucket_shard=0, bucket_shards=2))


# ---------------------------------------------------------------------------------------------- batch forms

@pytest.mark.parametrize("curve", M.NAMES)
def test_batch_full_width(curve, ctx_of):
    """B = 3 and B = 16 vectors under c <= 16: element b's rows are the single-vector kernel's words for the same scalars, and the
    model's.  Folded plans (c = 18, 21, and c = 23 under no_glv; two elements) where the curve has them, and three elements under
    c = 17: the real call never fuses there, the kernel does.  In the folded top window of k_digits_batch the bit above the c-th is
    0 for every scalar -- a half is below 2^126 = 2^(c K), a reduced scalar below q < 2^253 -- so these cases pin the fold's rows and
    signs, not that bit; only the narrow forms see it, through -2^bits (test_narrow, test_batch_narrow)."""
    ctx, cv = ctx_of(curve), M.CURVE_TABLE[curve]
    configs = [(c, ng, B) for c, ng in ((2, False), (8, False), (13, False), (16, False), (13, True), (16, True)) for B in (3, 16)]
    configs += [(c, False, 2) for c in (18, 21) if M.plan(curve, c).fold]
    configs += [(23, True, 2)] if M.plan(curve, 23, True).fold else []   # (BLS12-377: 253 = 11 * 23, the fold without the split)
    configs += [(17, False, 3)]                                          # 24 windows from 8229 points: no cut of the sort is in the way
    for c, no_glv, B in configs:
        pl, low, high, words = full_case(curve, c, no_glv)
        n, m = n_of(c), len(low) + len(high)
        table = M.to_bytes(low + high, 32)
        idxs = [(np.arange(n) + 131 * b) % m for b in range(B)]
        res = ctx.test_digits([table[i] for i in idxs], c=c, no_glv=pl.no_glv)
        assert (res["rc"], res["c"], res["K"], res["fold"]) == (M.MSM_OK, c, pl.K, pl.fold)
        assert res["words"].shape == (B, pl.K, pl.per_point * n)
        for b in (range(B) if B <= 3 else (0, 1, 7, 15)):
            same(res["words"][b], full_call(ctx, pl, low + high, idxs[b])["words"], f"{curve} c={c} B={B} element {b} against the single call")
        for b in range(B):
            same(res["words"][b], spread(words, idxs[b], pl.per_point), f"{curve} c={c} no_glv={no_glv} B={B} element {b}")
        # strict: refused as soon as one element holds a scalar >= q
        low_idx = [(np.arange(n) + 131 * b) % len(low) for b in range(B)]
        assert ctx.test_digits([table[i] for i in low_idx], c=c, no_glv=pl.no_glv, strict=True)["rc"] == M.MSM_OK
        mixed = [table[i] for i in low_idx[:-1]] + [table[idxs[-1]]]
        assert ctx.test_digits(mixed, c=c, no_glv=pl.no_glv, strict=True)["rc"] == M.MSM_ERR_SCALAR
    data = [np.zeros((N_SMALL, 32), np.uint8)] * 17
    refused(lambda: ctx.test_digits(data, c=13))
    refused(lambda: ctx.test_digits(data[:2], c=0))
    refused(lambda: ctx.test_digits(data[:2], c=13, k_lo=0, k_hi=1))
    refused(lambda: ctx.test_digits(data[:2], c=13, bucket_shard=0, bucket_shards=2))


@pytest.mark.parametrize("curve", M.NAMES)
def test_batch_narrow(curve, ctx_of):
    """B = 5 and B = 64 narrow vectors, every width and signedness: each element's rows equal the single-vector kernel's and the
    model's; elements are staged 16 bytes apart, so with n = 1037 an element of 1- and 2-byte scalars ends inside a dword."""
    ctx, cv = ctx_of(curve), M.CURVE_TABLE[curve]
    q = cv.q
    for width in M.WIDTHS:
        for signed in (False, True):
            bits = min(M.width_full_bits(width, signed), 127)
            for c, B in ((5, 5), (13, 64), (16, 5)) + (((18, 2),) if width >= 4 else ()):
                bits_c = 36 if c == 18 and width >= 8 else 18 if c == 18 else bits
                pl = M.plan(curve, c, narrow_bits=bits_c)
                assert pl is not None, (width, signed, c, bits_c)   # (every plan of this list exists: nothing is skipped)
                n = n_of(c)
                fmt = (width, bits_c, signed)
                ok, bad = M.narrow_values(pl, width, bits_c, signed)
                stored = [M.encode_narrow(v, width, q) for v in ok]
                words, rc = M.model_words(pl, stored, fmt)
                assert rc == M.MSM_OK
                table = M.to_bytes(stored, width)
                idxs = [(np.arange(n) + 57 * b) % len(stored) for b in range(B)]
                res = ctx.test_digits([table[i] for i in idxs], width=width, bits=bits_c, signed=signed, c=c)
                assert (res["rc"], res["K"], res["fold"]) == (M.MSM_OK, pl.K, pl.fold)
                for b in range(B):
                    same(res["words"][b], spread(words, idxs[b], pl.per_point), f"{curve} width {width} signed {signed} c={c} B={B} element {b}")
                for b in (0, B - 1):
                    one = ctx.test_digits(table[idxs[b]], width=width, bits=bits_c, signed=signed, c=c)
                    same(res["words"][b], one["words"], f"{curve} width {width} c={c} B={B} element {b} against the single call")
                if not bad:
                    continue
                # one refused value in the last element
                worst = idxs[-1].copy()
                tb = np.concatenate([table, narrow_bytes(bad[:1], width, q)])
                worst[n - 1] = len(stored)
                res = ctx.test_digits([table[i] for i in idxs[:-1]] + [tb[worst]], width=width, bits=bits_c, signed=signed, c=c)
                assert res["rc"] == M.MSM_ERR_SCALAR
                assert not res["words"][B - 1][:, pl.per_point * (n - 1):].any()
    refused(lambda: ctx.test_digits([np.zeros((N_SMALL, 4), np.uint8)] * 65, width=4, bits=8, c=13))
