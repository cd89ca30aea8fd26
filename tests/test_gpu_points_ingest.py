"""Compressed point loading, subgroup validation and the index of the first refused point (msm_set_points_ex,
msm_validate_points, msm_get_points_ex) on all four curves.  `-m gpu`."""
import pytest

from oracle import msm_oracle as O
from test_points_codec import CURVE_PARAMS, ZCASH_G1, decode, encode

pytestmark = pytest.mark.gpu

CURVES = ("bls377", "bls381", "pallas", "ed377")
BAD_AT = 12345
N_PLANT = 1 << 16


def _ctx(name, devices=None):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmContext

    cid = {"bls377": _lib.CURVE_BLS12_377_G1, "ed377": _lib.CURVE_ED_ON_BLS12_377, "bls381": _lib.CURVE_BLS12_381_G1,
           "pallas": _lib.CURVE_PALLAS}[name]
    return MsmContext(cid, devices=devices)


def _points(ctx, raw):
    nb = ctx.coord_bytes
    out = []
    for i in range(0, len(raw), 2 * nb):
        x, y = int.from_bytes(raw[i:i + nb], "little"), int.from_bytes(raw[i + nb:i + 2 * nb], "little")
        out.append(None if x == 0 and y == 0 else (x, y))   # (0, 0): the identity of a Weierstrass curve
    return out


def _raw(ctx, pts):
    nb = ctx.coord_bytes
    return b"".join(bytes(2 * nb) if P is None else P[0].to_bytes(nb, "little") + P[1].to_bytes(nb, "little") for P in pts)


def _neg(curve, P):
    C = CURVE_PARAMS[curve]
    if P is None:
        return None
    return ((-P[0]) % C.p, P[1]) if curve == "ed377" else (P[0], (-P[1]) % C.p)


def _expect_refused(ctx, fn, index, reason):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    with pytest.raises(MsmError) as e:
        fn()
    assert e.value.code == _lib.MSM_ERR_POINT, str(e.value)
    assert e.value.bad_index == index, str(e.value)
    assert f"point {index}: {reason}" in str(e.value), str(e.value)


def _scalars(curve, n, tag):
    return O.scalars_to_bytes(O.prng_ints(f"ingest/{curve}/{tag}", n, CURVE_PARAMS[curve].q))


# ---- 1. round trip ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(curve):
    ctx = _ctx(curve)
    try:
        n = 1 << 12
        ctx.generate_points(n, seed=71)
        pts = _points(ctx, ctx.get_points(0, n))
        pts = pts + [_neg(curve, P) for P in pts] + ([None] if curve != "ed377" else [])
        enc = b"".join(encode(curve, P) for P in pts)
        ctx.pointset_create()
        assert ctx.load_points(enc, compressed=True, validate="subgroup") == len(pts)
        assert ctx.get_points(0, len(pts)) == _raw(ctx, pts)
        assert ctx.get_points(0, len(pts), compressed=True) == enc
    finally:
        ctx.close()


# ---- 2. known answers and MSM equality -------------------------------------------------------------------------------

def test_zcash_vector_and_identity():
    ctx = _ctx("bls381")
    try:
        ctx.load_points(ZCASH_G1 + b"\xc0" + bytes(47), compressed=True, validate="subgroup")
        assert ctx.get_point(0) == (O.BLS12_381.gx, O.BLS12_381.gy)
        assert ctx.get_point(1) is None
        assert ctx.get_points(0, 2, compressed=True) == ZCASH_G1 + b"\xc0" + bytes(47)
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_msm_on_compressed_points_is_bit_identical(curve):
    ctx = _ctx(curve)
    try:
        n = 1 << 16
        ctx.generate_points(n, seed=72)
        raw, enc = ctx.get_points(0, n), ctx.get_points(0, n, compressed=True)
        for i in (0, 1, n // 2, n - 1):   # the library's encoder agrees with the test's
            assert enc[i * len(enc) // n:(i + 1) * len(enc) // n] == encode(curve, _points(ctx, ctx.get_points(i, 1))[0])
        sc = [_scalars(curve, n, f"msm{b}") for b in range(3)]
        ctx.pointset_create()
        ctx.set_points(raw)
        want_plain = ctx.run(sc[0], no_tables=True)[0].as_tuple()
        want_tab = ctx.run(sc[0])[0].as_tuple()
        want_batch = [r.as_tuple() for r, _ in ctx.run_batch(sc)]
        ctx.pointset_create()
        ctx.load_points(enc, compressed=True, validate="subgroup")
        assert ctx.run(sc[0], no_tables=True)[0].as_tuple() == want_plain
        res, info = ctx.run(sc[0])
        assert res.as_tuple() == want_tab
        assert [r.as_tuple() for r, _ in ctx.run_batch(sc)] == want_batch
        assert want_plain == want_tab == want_batch[0]
    finally:
        ctx.close()


# ---- 3. every refusal, planted at index 12345 of 2^16 valid points ----------------------------------------------------

def _nonsquare_x(curve):
    C = CURVE_PARAMS[curve]
    for x in range(2, 10 ** 6):
        if curve == "ed377":
            if not O.is_square((x * x - 1) * pow(C.d * x * x + 1, -1, C.p), C.p):
                return x
        elif not O.is_square(x ** 3 + C.b, C.p):
            return x
    raise AssertionError


def _le(v, n):
    return v.to_bytes(n, "little")


def _refusals():
    p377, p381, pp, pe = O.BLS12_377.p, O.BLS12_381.p, O.PALLAS.p, O.ED_ON_BLS12_377.p
    g381 = ZCASH_G1
    return [
        ("bls381", "coordinate >= p", (p381 | (1 << 383)).to_bytes(48, "big")),
        ("bls381", "invalid flags", bytes([g381[0] & 0x7F]) + g381[1:]),            # not marked compressed
        ("bls381", "invalid flags", b"\xe0" + bytes(47)),                            # infinity with the sign bit
        ("bls381", "invalid flags", b"\xc0" + bytes(46) + b"\x01"),                  # infinity with x bits
        ("bls381", "no curve point", (_nonsquare_x("bls381") | (1 << 383)).to_bytes(48, "big")),
        ("bls377", "coordinate >= p", _le(p377, 48)),
        ("bls377", "invalid flags", bytes(47) + b"\xc0"),                            # both flags
        ("bls377", "invalid flags", b"\x01" + bytes(46) + b"\x40"),                  # infinity with x bits
        ("bls377", "invalid flags", _le(1 | (1 << 377), 48)),                        # an unused bit
        ("bls377", "no curve point", _le(_nonsquare_x("bls377"), 48)),
        ("bls377", "invalid flags", _le((p377 - 1) | (1 << 383), 48)),               # y = 0 with the sign bit
        ("pallas", "coordinate >= p", _le(pp, 32)),
        ("pallas", "no curve point", _le(1 << 255, 32)),                             # x = 0, sign: 5 is no square
        ("pallas", "no curve point", _le(_nonsquare_x("pallas"), 32)),
        ("ed377", "coordinate >= p", _le(pe, 32)),
        ("ed377", "invalid flags", _le(1 | (1 << 253), 32)),                         # an unused bit
        ("ed377", "no curve point", _le(_nonsquare_x("ed377"), 32)),
        ("ed377", "invalid flags", _le(1 | (1 << 255), 32)),                         # (0, 1) with the sign bit
    ]


@pytest.fixture(scope="module")
def planted_base():
    """2^16 valid compressed points per curve (from msm_generate_points)."""
    out = {}
    for curve in CURVES:
        ctx = _ctx(curve)
        try:
            ctx.generate_points(N_PLANT, seed=73)
            out[curve] = ctx.get_points(0, N_PLANT, compressed=True)
        finally:
            ctx.close()
    return out


def _plant(base, curve, index, enc):
    w = len(enc)
    assert len(base) == N_PLANT * w
    return base[:index * w] + enc + base[(index + 1) * w:]


@pytest.mark.parametrize("case", range(len(_refusals())))
def test_refusal(planted_base, case):
    from montgomery_amd import _lib
    from montgomery_amd.api import MsmError

    curve, reason, enc = _refusals()[case]
    with pytest.raises(ValueError, match=reason):   # the test's decoder refuses it for the same reason
        decode(curve, enc)
    ctx = _ctx(curve)
    try:
        ctx.load_points(planted_base[curve], compressed=True, validate="curve")   # the base itself loads
        data = _plant(planted_base[curve], curve, BAD_AT, enc)
        _expect_refused(ctx, lambda: ctx.load_points(data, compressed=True, validate="none"), BAD_AT, reason)
        with pytest.raises(MsmError) as e:
            ctx.run(_scalars(curve, 4, "after"))
        assert e.value.code == _lib.MSM_ERR_NO_POINTS
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_smallest_bad_index_is_reported(planted_base, curve):
    _, _, late = [r for r in _refusals() if r[0] == curve][0]
    _, reason, early = [r for r in _refusals() if r[0] == curve][-1]
    data = _plant(_plant(planted_base[curve], curve, 50000, late), curve, BAD_AT, early)
    ctx = _ctx(curve)
    try:
        _expect_refused(ctx, lambda: ctx.load_points(data, compressed=True, validate="subgroup"), BAD_AT, reason)
    finally:
        ctx.close()


# ---- 4. subgroup ------------------------------------------------------------------------------------------------------

def _random_point(curve, seed):
    C = CURVE_PARAMS[curve]
    for x in O.prng_ints(f"ingest/R/{curve}/{seed}", 200, C.p):
        y = O.sqrt_mod(x ** 3 + C.b, C.p)
        if y is not None:
            return (x, y)
    raise AssertionError


def _torsion_point(curve, ell):
    """A point of order ell, from [|E| / ell^e] R for a random curve point R (|E| = h q, ell^e the power of ell in it: the
    ell-part may be Z/ell x Z/ell, which [|E| / ell] R would always send to the identity), multiplied by ell while that
    leaves a non-identity point."""
    C = CURVE_PARAMS[curve]
    order, ell_e = C.h * C.q, 1
    while order % (ell_e * ell) == 0:
        ell_e *= ell
    for s in range(20):
        T = O.aff_scale(order // ell_e, _random_point(curve, f"{ell}/{s}"), C.p)
        if T is None:
            continue
        while O.aff_scale(ell, T, C.p) is not None:
            T = O.aff_scale(ell, T, C.p)
        return T
    raise AssertionError(f"no point of order {ell}")


def _outside_points(curve):
    """Curve points outside the prime-order subgroup, each with a name."""
    C = CURVE_PARAMS[curve]
    G = (C.gx, C.gy)
    if curve == "ed377":
        p = C.p
        i = O.sqrt_mod(p - 1, p)
        T2 = (0, p - 1)
        GT = O.te_to_affine(O.te_add(O.te_from_affine(G, C), O.te_from_affine(T2, C), C), C)
        return [("order 2", T2), ("order 4 (+)", (i, 0)), ("order 4 (-)", (p - i, 0)), ("G + T", GT)]
    if curve == "bls377":
        T2 = (C.p - 1, 0)
        out = [("order 2", T2)] + [(f"order {l}", _torsion_point(curve, l)) for l in (3, 7, 13, 499)]
        return out + [("G + T", O.aff_add(G, T2, C.p))]
    T3 = _torsion_point(curve, 3)
    out = [(f"order {l}", _torsion_point(curve, l)) for l in (3, 11, 10177, 859267, 52437899)]
    return out + [("G + T", O.aff_add(G, T3, C.p))]


@pytest.mark.parametrize("curve", ("bls377", "bls381", "ed377"))
def test_points_outside_the_subgroup(planted_base, curve):
    ctx = _ctx(curve)
    try:
        for name, T in _outside_points(curve):
            enc = encode(curve, T)
            assert decode(curve, enc) == T, name
            data = _plant(planted_base[curve], curve, BAD_AT, enc)
            ctx.load_points(data, compressed=True, validate="curve")          # on the curve: accepted
            ctx.validate_points(0, BAD_AT, level="subgroup")                  # the points before it pass
            _expect_refused(ctx, lambda: ctx.validate_points(10000, 20000, level="subgroup"), BAD_AT,
                            "not in the prime-order subgroup")
            _expect_refused(ctx, lambda: ctx.load_points(data, compressed=True), BAD_AT, "not in the prime-order subgroup")
            raw = _raw(ctx, [T])   # and through the uncompressed format
            _expect_refused(ctx, lambda: ctx.load_points(raw, validate="subgroup"), 0, "not in the prime-order subgroup")
            ctx.load_points(raw, validate="curve")
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", CURVES)
def test_valid_points_pass_and_uncompressed_refusals_have_an_index(planted_base, curve):
    ctx = _ctx(curve)
    try:
        ctx.load_points(planted_base[curve], compressed=True, validate="subgroup")
        raw = ctx.get_points(0, N_PLANT)
        ctx.validate_points()
        ctx.load_points(raw, validate="subgroup")
        # not on the curve: y + 1
        P = _points(ctx, raw[BAD_AT * 2 * ctx.coord_bytes:(BAD_AT + 1) * 2 * ctx.coord_bytes])[0]
        bad = _raw(ctx, [(P[0], (P[1] + 1) % CURVE_PARAMS[curve].p)])
        w = 2 * ctx.coord_bytes
        data = raw[:BAD_AT * w] + bad + raw[(BAD_AT + 1) * w:]
        _expect_refused(ctx, lambda: ctx.load_points(data, validate="curve"), BAD_AT, "not on curve")
        ctx.load_points(data, validate=None)   # as msm_set_points(check_curve = 0)
        _expect_refused(ctx, lambda: ctx.validate_points(level="curve"), BAD_AT, "not on curve")
        big = _le(CURVE_PARAMS[curve].p, ctx.coord_bytes) + bytes(ctx.coord_bytes)
        data = raw[:BAD_AT * w] + big + raw[(BAD_AT + 1) * w:]
        _expect_refused(ctx, lambda: ctx.load_points(data, validate=None), BAD_AT, "coordinate >= p")
    finally:
        ctx.close()


def test_pallas_every_curve_point_passes():
    ctx = _ctx("pallas")
    try:
        pts = [_random_point("pallas", s) for s in range(64)]
        ctx.load_points(b"".join(encode("pallas", P) for P in pts), compressed=True, validate="subgroup")
        assert _points(ctx, ctx.get_points(0, 64)) == pts
    finally:
        ctx.close()


# ---- 5. scale, 6. device list -----------------------------------------------------------------------------------------

def test_compressed_subgroup_load_at_2p22():
    C = O.BLS12_377
    n = 1 << 22
    ctx = _ctx("bls377")
    try:
        a = O.scalars_from_bytes(ctx.generate_points(n, seed=74, want_scalars=True))
        enc = ctx.get_points(0, n, compressed=True)
        _, sc_raw = ctx.generate_scalars(n, seed=75, to_host=True)
        s = O.scalars_from_bytes(sc_raw)
        ctx.pointset_create()
        ctx.load_points(enc, compressed=True, validate="subgroup")
        res, _ = ctx.run(sc_raw)
        k = sum(x * y for x, y in zip(s, a)) % C.q
        assert res.as_tuple() == O.aff_scale(k, (C.gx, C.gy), C.p)
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", ("bls377", "ed377"))
def test_device_list_context(planted_base, curve):
    sc = _scalars(curve, N_PLANT, "multi")
    one = _ctx(curve)
    try:
        one.load_points(planted_base[curve], compressed=True)
        want = one.run(sc)[0].as_tuple()
    finally:
        one.close()
    ctx = _ctx(curve, devices=[0, 0])
    try:
        ctx.load_points(planted_base[curve], compressed=True)
        assert ctx.run(sc)[0].as_tuple() == want
        data = _plant(planted_base[curve], curve, BAD_AT, _refusals()[[r[0] for r in _refusals()].index(curve)][2])
        _expect_refused(ctx, lambda: ctx.load_points(data, compressed=True), BAD_AT, "coordinate >= p")
    finally:
        ctx.close()
