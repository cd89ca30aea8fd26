"""msm_run_narrow: MSMs over 1- to 16-byte and bit-bounded 32-byte scalars equal msm_run over the same values.  `-m gpu`."""
import ctypes

import numpy as np
import pytest

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

CURVES = ("bls377", "ed377", "bls381", "pallas")
BITS = (1, 7, 8, 31, 32, 63, 64, 127, 128)


def _ctx(name, **kw):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    cid = {"bls377": _lib.CURVE_BLS12_377_G1, "ed377": _lib.CURVE_ED_ON_BLS12_377, "bls381": _lib.CURVE_BLS12_381_G1,
           "pallas": _lib.CURVE_PALLAS}[name]
    return MsmContext(cid, **kw)


def _order(name):
    return {"bls377": O.BLS12_377.q, "ed377": O.ED_ON_BLS12_377.q, "bls381": O.BLS12_381.q, "pallas": O.PALLAS.q}[name]


@pytest.fixture(scope="module", params=CURVES)
def cv(request):
    ctx = _ctx(request.param)
    ctx.generate_points(1 << 14, seed=910)
    yield request.param, ctx
    ctx.close()


def _values(tag, n, bits, signed):
    """n integers over the whole declared range, the extremes 0, 2^bits - 1 and -2^bits among them when there is room."""
    from montgomery_amd import narrow as N

    lo, hi = N.value_range(bits, signed)
    vals = [lo + v for v in O.prng_ints(f"narrow/{tag}/{n}/{bits}/{signed}", n, hi - lo)]
    for i, e in enumerate([hi - 1, lo, 0][: max(0, n - 1)]):
        vals[(7 * i + 1) % n] = e
    return vals


def _formats():
    from montgomery_amd import narrow as N

    for width in N.WIDTHS:
        for signed in (False, True):
            for bits in BITS:
                if bits <= N.full_bits(width, signed):
                    yield width, signed, bits


def _windows(name, bits):
    """explicit windows next to the default: K c = bits + 1 where a c does it, one that leaves a short top window, and on the
    Weierstrass curves a c >= 18 whose top window folds (bits + 1 = K c + 1)"""
    cs = [13]
    cs += [c for c in range(24, 1, -1) if (bits + 1) % c == 0 and (bits + 1) // c <= 64][:1]
    if name != "ed377":
        cs += [c for c in (18, 19, 20, 21, 22, 23, 24) if (bits + 1) % c == 1 and bits + 1 > c][:1]
    if bits <= 8:
        cs.append(2)
    return sorted(set(cs))


def _narrow(ctx, vals, width, signed, bits, q, **kw):
    from montgomery_amd import narrow as N

    return ctx.run_narrow(N.pack(vals, width, signed, q), bits=bits, signed=signed, width=width, **kw)


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16, 32])
def test_narrow_equals_wide(cv, width):
    from montgomery_amd import narrow as N

    name, ctx = cv
    q = _order(name)
    for w, signed, bits in _formats():
        if w != width:
            continue
        for n in (1, 100, 1 << 10, 1 << 14):
            vals = _values(f"{name}/{width}", n, bits, signed)
            exp, _ = ctx.run(N.widen(vals, q))
            got, info = _narrow(ctx, vals, width, signed, bits, q)
            assert got == exp, (name, width, signed, bits, n, info["c"], info["K"])
            assert ctx.plan_narrow(n, bits) == (info["c"], info["K"])
            assert not info["tables"]
            if n in (100, 1 << 14):
                for c in _windows(name, bits):
                    got, info = _narrow(ctx, vals, width, signed, bits, q, c=c)
                    assert got == exp and info["c"] == c, (name, width, signed, bits, n, c, info["K"])


def test_narrow_numpy_arrays(cv):
    """The dtype gives width and signedness; default bits = all the width gives (int8 -128 at bits = 7 is the negative extreme)."""
    from montgomery_amd import narrow as N

    name, ctx = cv
    q = _order(name)
    rng = np.random.default_rng(5)
    for dt in ("uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64"):
        ii = np.iinfo(dt)
        arr = rng.integers(ii.min, ii.max, size=1000, dtype=dt, endpoint=True)
        arr[:3] = (ii.min, ii.max, 0)
        exp, _ = ctx.run(N.widen(arr, q))
        got, info = ctx.run_narrow(arr)
        assert got == exp, dt
        assert ctx.plan_narrow(1000, N.full_bits(*N.dtype_format(dt))) == (info["c"], info["K"])


def test_narrow_against_oracle(cv):
    from montgomery_amd import narrow as N

    name, ctx = cv
    q, n = _order(name), 300
    pts = O.points_from_bytes(ctx.get_points(0, n), ctx.coord_bytes)
    for width, signed, bits in ((8, False, 64), (4, True, 31), (32, True, 128), (1, False, 1)):
        vals = _values(f"oracle/{name}", n, bits, signed)
        got, info = _narrow(ctx, vals, width, signed, bits, q)
        ints = [v % q for v in vals]
        if name == "ed377":
            assert (got.x, got.y) == O.msm_basic_te(ints, pts, c=max(info["c"], 4))
        else:
            C = {"bls377": O.BLS12_377, "bls381": O.BLS12_381, "pallas": O.PALLAS}[name]
            assert got.as_tuple() == O.msm_batched_affine(ints, pts, C=C, c=16)


def test_narrow_edges(cv):
    """All zeros; every value at 2^bits - 1 and at -2^bits under windows where K c = bits + 1, where the top window folds and
    where it is short; all ones with bits = 1 (one bucket holds everything); point_lo; device scalars; n = 0."""
    from montgomery_amd import narrow as N

    name, ctx = cv
    q, n = _order(name), 1 << 12
    ident = ctx.run(bytes(32 * n))[0]
    assert ctx.run_narrow(np.zeros(n, dtype=np.uint64))[0] == ident
    assert ctx.run_narrow(np.zeros(0, dtype=np.int32))[0] == ident
    assert ctx.run_narrow(b"", width=16, signed=True)[0] == ident
    assert ctx.run_narrow(np.full(n, -128, dtype=np.int8))[0] == ctx.run(N.widen([-128] * n, q))[0]
    for width, bits in ((8, 63), (4, 31), (32, 128), (16, 127), (1, 7), (32, 36)):
        wins = {None, 2 if bits <= 8 else 13}
        wins |= {c for c in range(2, 25) if (bits + 1) % c == 0 and (bits + 1) // c <= 64}           # K c = bits + 1
        if name != "ed377":
            wins |= {c for c in range(18, 25) if (bits + 1) % c == 1 and bits + 1 > c}               # folded top window
        wins |= {c for c in (5, 11, 19) if (bits + 1) % c not in (0, 1) and (bits + c) // c <= 64}    # short top window
        for v in ((1 << bits) - 1, -(1 << bits)):
            exp = ctx.run(N.widen([v] * n, q))[0]
            for c in sorted(wins, key=lambda x: x or 0):
                got, info = _narrow(ctx, [v] * n, width, True, bits, q, c=c)
                assert got == exp, (name, width, bits, v < 0, c, info["K"])
    ones = np.ones(n, dtype=np.uint8)
    got, info = ctx.run_narrow(ones, bits=1)
    assert got == ctx.run(N.widen(ones, q))[0] and info["max_bucket"] == n
    vals = _values(f"lo/{name}", 1000, 16, True)
    arr = np.array(vals, dtype=np.int32)
    for lo in (0, 1, 777, (1 << 14) - 1000):
        p = ctx.device_alloc(32 * 1000)
        ctx.device_upload(p, N.widen(vals, q))
        exp = ctx.run_device(p, 1000, point_lo=lo)[0]
        ctx.device_free(p)
        assert ctx.run_narrow(arr, bits=16, point_lo=lo)[0] == exp
    exp = ctx.run(N.widen(vals, q))[0]
    for dt in ("int32", "int64"):
        raw = np.array(vals, dtype=dt).tobytes()
        p = ctx.device_alloc(len(raw) + 16)
        ctx.device_upload(p, raw)
        assert ctx.run_narrow_device(p, 1000, np.dtype(dt).itemsize, 16, True)[0] == exp
        ctx.device_free(p)
    # 1- and 2-byte scalars that start inside the dword a lane loads
    for dt, bits in (("int16", 15), ("uint8", 8)):
        small = np.array(_values(f"off/{name}", 1001, bits, dt == "int16"), dtype=dt)
        exp = ctx.run(N.widen(small, q))[0]
        w = small.dtype.itemsize
        p = ctx.device_alloc(len(small) * w + 16)
        for off in range(w, 4, w):
            ctx.device_upload(p, b"\xff" * off + small.tobytes())
            assert ctx.run_narrow_device(p + off, 1001, w, None, dt == "int16")[0] == exp, (dt, off)
        ctx.device_free(p)


def test_narrow_refusals(cv):
    from montgomery_amd import _lib
    from montgomery_amd import narrow as N
    from montgomery_amd.api import MsmError

    name, ctx = cv
    q, n = _order(name), 500
    good = _values(f"ref/{name}", n, 20, True)
    exp = ctx.run(N.widen(good, q))[0]

    def refused(code, f):
        with pytest.raises(MsmError) as e:
            f()
        assert e.value.code == code, e.value
        assert _narrow(ctx, good, 4, True, 20, q)[0] == exp   # the context still runs a correct MSM

    for width in (4, 32):
        for signed, bad in ((False, 1 << 20), (True, 1 << 20), (True, -(1 << 20) - 1)):
            vals = list(good) if signed else [abs(v) for v in good]
            vals[n // 2] = bad
            refused(_lib.MSM_ERR_SCALAR, lambda: _narrow(ctx, vals, width, signed, 20, q))
    mid = [q // 2 + 12345] + [0] * (n - 1)
    refused(_lib.MSM_ERR_SCALAR, lambda: ctx.run_narrow(O.scalars_to_bytes(mid), bits=128, signed=True, width=32))
    refused(_lib.MSM_ERR_SCALAR, lambda: ctx.run_narrow(O.scalars_to_bytes([q] + [0] * (n - 1)), bits=128, signed=False, width=32))
    refused(_lib.MSM_ERR_SCALAR, lambda: ctx.run_narrow(np.full(n, 4, dtype=np.uint8), bits=2))
    raw = bytes(8 * n)
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(bytes(3 * n), width=3))
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(bytes(32 * n), bits=129, width=32))
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(bytes(32 * n), width=32))            # width 32 needs bits
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(raw, bits=65, width=8))
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(raw, bits=64, signed=True, width=8))
    refused(_lib.MSM_ERR_ARG, lambda: ctx.run_narrow(bytes(16 * n), bits=128, c=2, width=16))  # 65 windows
    lib = _lib.load()
    buf = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
    res = _lib.MsmResult()
    for bad in ({"merged_sums": 1}, {"k_hi": 1}, {"bucket_shards": 2}, {"by_window": 1}):
        o = _lib.MsmOpts(**bad)
        assert lib.msm_run_narrow(ctx._h, buf, n, 0, 8, 0, 0, ctypes.byref(o), ctypes.byref(res)) == _lib.MSM_ERR_ARG
    assert lib.msm_run_narrow(ctx._h, buf, (1 << 14) + 1, 0, 8, 0, 0, None, ctypes.byref(res)) == _lib.MSM_ERR_NO_POINTS
    assert _narrow(ctx, good, 4, True, 20, q)[0] == exp


def test_narrow_refused_on_a_device_list_context():
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    ctx = _ctx("bls377", devices=[0, 0])
    ctx.generate_points(256, seed=3)
    with pytest.raises(MsmError) as e:
        ctx.run_narrow(np.ones(256, dtype=np.uint32))
    assert e.value.code == _lib.MSM_ERR_ARG
    ctx.close()


def test_narrow_leaves_window_tables_alone():
    from montgomery_amd import narrow as N

    ctx = _ctx("bls377")
    n = 1 << 14
    ctx.generate_points(n, seed=911)
    ctx.precompute()
    before = ctx.tables_info()
    assert before[1] > 0
    arr = np.arange(n, dtype=np.uint64) * 0x9E3779B97F4A7C15
    got, info = ctx.run_narrow(arr)
    assert not info["tables"] and ctx.tables_info() == before
    exp, winfo = ctx.run(N.widen(arr, O.BLS12_377.q))
    assert winfo["tables"] and got == exp and ctx.tables_info() == before
    ctx.close()


@pytest.mark.parametrize("B", [1, 2, 7, 16, 40])
def test_batch_narrow_equals_run_narrow(cv, B):
    name, ctx = cv
    rng = np.random.default_rng(B)
    for dt, bits, n in (("uint64", None, 1 << 12), ("int32", None, 1 << 10), ("uint8", 1, 1 << 14), ("int16", 9, 100)):
        ii = np.iinfo(dt)
        lo, hi = (ii.min, ii.max) if bits is None else ((-(1 << bits) if ii.min else 0), (1 << bits) - 1)
        sc = [rng.integers(lo, hi, size=n, dtype=dt, endpoint=True) for _ in range(B)]
        got = ctx.run_batch_narrow(sc, bits=bits)
        assert len(got) == B
        for s, (r, info) in zip(sc, got):
            assert r == ctx.run_narrow(s, bits=bits)[0], (name, dt, bits, n)
        infos = [i for _, i in got]
        assert all(i == infos[0] for i in infos)
    # K >= 4: 40 elements exceed one fused group of 128 windows
    sc = [rng.integers(0, (1 << 63) - 1, size=1 << 10, dtype=np.uint64) for _ in range(B)]
    got = ctx.run_batch_narrow(sc, c=13)
    assert got[0][1]["K"] == 5
    for s, (r, _) in zip(sc, got):
        assert r == ctx.run_narrow(s, c=13)[0]


def test_batch_narrow_device_and_fallback_region():
    """device elements (one of them misaligned: element by element), and 2^21 points: outside the fused region"""
    ctx = _ctx("bls377")
    n = 1 << 12
    ctx.generate_points(1 << 21, seed=912)
    rng = np.random.default_rng(9)
    sc = [rng.integers(0, 255, size=n, dtype=np.uint8, endpoint=True) for _ in range(5)]
    exp = [ctx.run_narrow(s)[0] for s in sc]
    ptrs = [ctx.device_alloc(n + 16) for _ in sc]
    for p, s in zip(ptrs, sc):
        ctx.device_upload(p, s.tobytes())
    assert [r for r, _ in ctx.run_batch_narrow_device(ptrs, n, 1)] == exp
    ctx.device_upload(ptrs[2], b"\0" + sc[2].tobytes())
    got = ctx.run_batch_narrow_device(ptrs[:2] + [ptrs[2] + 1] + ptrs[3:], n, 1)
    assert [r for r, _ in got] == exp
    for p in ptrs:
        ctx.device_free(p)
    big = [rng.integers(0, (1 << 32) - 1, size=1 << 21, dtype=np.uint32) for _ in range(2)]
    got = ctx.run_batch_narrow(big)
    for s, (r, _) in zip(big, got):
        assert r == ctx.run_narrow(s)[0]
    ctx.close()


@pytest.mark.parametrize("case", ["one_level", "radix_split", "bin_split"])
def test_narrow_large_against_known_discrete_logs(case):
    """BLS12-377, 64-bit unsigned and 33-bit signed scalars through every sort path, against sum_i s_i a_i G."""
    from oracle import c_oracle

    from montgomery_amd import narrow as N

    C = O.BLS12_377
    logn, c = {"one_level": (18, None), "radix_split": (21, 16), "bin_split": (22, None)}[case]
    n = 1 << logn
    ctx = _ctx("bls377")
    logs = ctx.generate_points(n, seed=913, want_scalars=True)
    rng = np.random.default_rng(logn)
    u64 = rng.integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)
    s33 = rng.integers(-(1 << 33), (1 << 33) - 1, size=n, dtype=np.int64, endpoint=True)
    s33[:2] = (-(1 << 33), (1 << 33) - 1)
    for arr, bits in ((u64, None), (s33, 33)):
        got, info = ctx.run_narrow(arr, bits=bits, c=c)
        if case == "bin_split":
            assert info["c"] > 16
        wide = np.zeros((n, 4), dtype=np.uint64)   # the 32-byte form, vectorised: v, or q - |v|
        if arr.dtype == np.int64:
            neg = arr < 0
            mag = np.where(neg, -arr, arr).astype(np.uint64)
            wide[:, 0] = mag
            k_pos = c_oracle.dot_mod(logs, np.where(neg[:, None], 0, wide).astype(np.uint64).tobytes(), n, C.q)
            k_neg = c_oracle.dot_mod(logs, np.where(neg[:, None], wide, 0).astype(np.uint64).tobytes(), n, C.q)
            k = (k_pos - k_neg) % C.q
        else:
            wide[:, 0] = arr
            k = c_oracle.dot_mod(logs, wide.tobytes(), n, C.q)
        assert got.as_tuple() == O.aff_scale(k, (C.gx, C.gy), C.p), (case, arr.dtype, info["c"], info["K"])
    ctx.close()


def test_scalar_bits(cv):
    from montgomery_amd import _lib, workloads
    from montgomery_amd import narrow as N
    from montgomery_amd.api import MsmError

    name, ctx = cv
    q = _order(name)
    for kind in workloads.KINDS:
        raw = workloads.scalars(kind, 1 << 12, seed=3).tobytes()
        ints = [v % q for v in O.scalars_from_bytes(raw)]
        raw = O.scalars_to_bytes(ints)
        want_u = max(v.bit_length() for v in ints)
        want_s = max(min(v.bit_length(), (q - v - 1).bit_length()) for v in ints)
        want = (want_u if want_u <= 128 else 255, want_s if want_s <= 128 else 255)
        assert ctx.scalar_bits(raw) == want, kind
        p = ctx.device_alloc(len(raw))
        ctx.device_upload(p, raw)
        assert ctx.scalar_bits(p, n=len(ints)) == want
        ctx.device_free(p)
    assert ctx.scalar_bits(bytes(32 * 100)) == (0, 0)
    assert ctx.scalar_bits(b"") == (0, 0)
    for vals in ([-1, 0, 1], [-128, 127], [-129, 5], [3, (1 << 40) - 1, -(1 << 40)], [-(1 << 128), (1 << 128) - 1], [1 << 128]):
        ub, sb = N.bits_needed(vals)
        want = (ub if ub <= 128 else 255, sb if sb <= 128 else 255)
        full = vals * 50
        raw = N.widen(full, q)
        assert ctx.scalar_bits(raw) == want, vals
        if 1 <= want[1] <= 128:
            exp = ctx.run(raw)[0] if len(full) <= ctx.n_points else None
            assert ctx.run_narrow(raw, bits=want[1], signed=True, width=32)[0] == exp
            if want[1] > 1:
                with pytest.raises(MsmError) as e:
                    ctx.run_narrow(raw, bits=want[1] - 1, signed=True, width=32)
                assert e.value.code == _lib.MSM_ERR_SCALAR


def test_batch_narrow_fuses_where_a_single_call_takes_the_big_window():
    """2^18 x 4 elements of 16 bits on BLS12-377: a single call runs one 17-bit window (bin split), the batch stays inside the
    one-level sort (c <= 16) and shares its launches."""
    ctx = _ctx("bls377")
    n = 1 << 18
    ctx.generate_points(n, seed=914)
    rng = np.random.default_rng(14)
    sc = [rng.integers(0, 65535, size=n, dtype=np.uint16, endpoint=True) for _ in range(4)]
    singles = [ctx.run_narrow(s) for s in sc]
    assert singles[0][1]["c"] == 17
    got = ctx.run_batch_narrow(sc)
    assert got[0][1]["c"] <= 16
    assert [r for r, _ in got] == [r for r, _ in singles]
    fused_c = got[0][1]["c"]
    assert got[0][1]["rounds"] < 4 * ctx.run_narrow(sc[0], c=fused_c)[1]["rounds"]
    ctx.close()


def test_narrow_device_alignment_is_an_argument_error(cv):
    """Device scalars of the 16- and 32-byte forms are loaded 16 bytes at a time: anything else is refused before the call runs."""
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    name, ctx = cv
    p = ctx.device_alloc(32 * 64 + 64)
    ctx.device_upload(p, bytes(32 * 64 + 64))
    for f in (lambda: ctx.run_narrow_device(p + 8, 64, 32, 64), lambda: ctx.run_narrow_device(p + 4, 64, 16),
              lambda: ctx.run_narrow_device(p + 4, 64, 8), lambda: ctx.scalar_bits(p + 8, n=64),
              lambda: ctx.run_batch_narrow_device([p, p + 8], 32, 16)):
        with pytest.raises(MsmError) as e:
            f()
        assert e.value.code == _lib.MSM_ERR_ARG
    assert ctx.run_narrow_device(p + 16, 64, 32, 64)[0] == ctx.run(bytes(32 * 64))[0]
    assert ctx.scalar_bits(p + 16, n=64) == (0, 0)
    ctx.device_free(p)
