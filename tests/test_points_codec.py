"""Compressed point encodings (msm_set_points_ex / msm_get_points_ex, include/msm_hip.h): the test-side encoder and decoder
every ingest test uses, their known answers, and the ABI 8 surface.  No GPU needed."""
import os
import re

import pytest

from oracle import msm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CURVE_PARAMS = {"bls377": O.BLS12_377, "bls381": O.BLS12_381, "pallas": O.PALLAS, "ed377": O.ED_ON_BLS12_377}
COMPRESSED_BYTES = {"bls377": 48, "bls381": 48, "pallas": 32, "ed377": 32}

# the BLS12-381 G1 generator in the ZCash serialisation
ZCASH_G1 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def encode(curve, P):
    """The compressed encoding of P: (x, y), or None for the identity of a Weierstrass curve (Edwards: (0, 1) is a point)."""
    C = CURVE_PARAMS[curve]
    if curve == "ed377":
        x, y = P
        b = bytearray(y.to_bytes(32, "little"))
        if x > (C.p - 1) // 2:
            b[31] |= 0x80
        return bytes(b)
    if curve == "bls381":
        if P is None:
            return b"\xc0" + bytes(47)
        b = bytearray(P[0].to_bytes(48, "big"))
        b[0] |= 0x80
        if P[1] > (C.p - 1) // 2:
            b[0] |= 0x20
        return bytes(b)
    if curve == "bls377":
        if P is None:
            return bytes(47) + b"\x40"
        b = bytearray(P[0].to_bytes(48, "little"))
        if P[1] > (C.p - 1) // 2:
            b[47] |= 0x80
        return bytes(b)
    if P is None:   # pallas
        return bytes(32)
    b = bytearray(P[0].to_bytes(32, "little"))
    if P[1] & 1:
        b[31] |= 0x80
    return bytes(b)


def decode(curve, b):
    """The inverse of encode; raises ValueError on every encoding the library refuses."""
    C = CURVE_PARAMS[curve]
    p = C.p
    if curve == "ed377":
        sign, y = b[31] >> 7, int.from_bytes(b, "little") & ((1 << 255) - 1)
        if y >> 253:
            raise ValueError("invalid flags")
        if y >= p:
            raise ValueError("coordinate >= p")
        x = O.sqrt_mod((y * y - 1) * pow(C.d * y * y + 1, -1, p), p)
        if x is None:
            raise ValueError("no curve point")
        if (x > (p - 1) // 2) != bool(sign):
            if x == 0:
                raise ValueError("invalid flags")
            x = p - x
        return (x, y)
    if curve == "bls381":
        fl, x = b[0] >> 5, int.from_bytes(b, "big") & ((1 << 381) - 1)
        inf, sign = bool(fl & 2), bool(fl & 1)
        if not fl & 4 or (inf and (sign or x)):
            raise ValueError("invalid flags")
    elif curve == "bls377":
        v = int.from_bytes(b, "little")
        sign, inf, x = bool(v >> 383), bool((v >> 382) & 1), v & ((1 << 377) - 1)
        if (inf and (sign or x)) or (v >> 377) & 0x1F:
            raise ValueError("invalid flags")
    else:
        v = int.from_bytes(b, "little")
        sign, x = bool(v >> 255), v & ((1 << 255) - 1)
        inf = not sign and x == 0
    if inf:
        return None
    if x >= p:
        raise ValueError("coordinate >= p")
    y = O.sqrt_mod(x ** 3 + C.b, p)
    if y is None:
        raise ValueError("no curve point")
    odd = bool(y & 1) if curve == "pallas" else y > (p - 1) // 2
    if odd != sign:
        if y == 0:
            raise ValueError("invalid flags")
        y = p - y
    return (x, y)


def test_zcash_generator_vector():
    G = (O.BLS12_381.gx, O.BLS12_381.gy)
    assert encode("bls381", G) == ZCASH_G1
    assert decode("bls381", ZCASH_G1) == G
    assert decode("bls381", b"\xc0" + bytes(47)) is None


@pytest.mark.parametrize("curve", sorted(CURVE_PARAMS))
def test_encoder_round_trip(curve):
    C = CURVE_PARAMS[curve]
    pts = []
    for k in (1, 2, 3, 12345, C.q - 1):
        if curve == "ed377":
            P = O.te_to_affine(O.te_scale(k, O.te_from_affine((C.gx, C.gy), C), C), C)
        else:
            P = O.aff_scale(k, (C.gx, C.gy), C.p)
        pts.append(P)
    if curve != "ed377":
        pts.append(None)
    for P in pts:
        b = encode(curve, P)
        assert len(b) == COMPRESSED_BYTES[curve]
        assert decode(curve, b) == P


def test_encoder_refusals():
    p377 = O.BLS12_377.p
    with pytest.raises(ValueError, match="invalid flags"):   # (p - 1, 0) with the sign of a non-zero root
        decode("bls377", bytearray((p377 - 1).to_bytes(48, "little")[:47]) + bytes([((p377 - 1) >> 376) | 0x80]))
    with pytest.raises(ValueError, match="invalid flags"):   # (0, 1) with the sign bit
        decode("ed377", (1 | (1 << 255)).to_bytes(32, "little"))
    with pytest.raises(ValueError, match="invalid flags"):   # no compression flag
        decode("bls381", bytes([ZCASH_G1[0] & 0x7F]) + ZCASH_G1[1:])
    with pytest.raises(ValueError, match="no curve point"):  # x = 0 with the sign bit: 5 is no square mod p
        decode("pallas", (1 << 255).to_bytes(32, "little"))


def test_abi_8_exports_the_ingest_entries():
    from montgomery_amd import _lib

    text = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", text).group(1)) == 8 == _lib.ABI_VERSION
    for name in ("msm_set_points_ex", "msm_validate_points", "msm_get_points_ex"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTS
    for enum, val in (("MSM_POINTS_UNCOMPRESSED", 0), ("MSM_POINTS_COMPRESSED", 1), ("MSM_VALIDATE_NONE", 0),
                      ("MSM_VALIDATE_CURVE", 1), ("MSM_VALIDATE_SUBGROUP", 2)):
        assert re.search(rf"\b{enum} = {val}\b", text), enum
    lib = _lib.load()
    assert lib.msm_abi_version() == 8
    for name in ("msm_set_points_ex", "msm_validate_points", "msm_get_points_ex"):
        assert hasattr(lib, name)


def test_addon_exports_the_ingest_entries():
    from napi_support import assert_exports

    assert_exports(("setPointsEx", "getPointsEx", "POINTS_COMPRESSED", "POINTS_UNCOMPRESSED", "VALIDATE_NONE", "VALIDATE_CURVE",
                    "VALIDATE_SUBGROUP"), facade=())
