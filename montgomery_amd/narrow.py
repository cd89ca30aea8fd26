"""Narrow scalar formats of msm_run_narrow (include/msm_hip.h), host side, pure Python / numpy.

A narrow scalar is a little-endian integer of 1, 2, 4, 8 or 16 bytes (two's complement when signed), or a 32-byte field element
holding a small value (v >= 0 as v, v < 0 as q - |v|).  `widen` writes such values in the 32-byte form msm_run takes, which is
what the tests and tools/narrow_time.py compare a narrow call against.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

WIDTHS = (1, 2, 4, 8, 16, 32)
MAX_BITS = 128

# numpy dtype -> (width in bytes, signed)
DTYPES = {
    np.dtype("uint8"): (1, False), np.dtype("uint16"): (2, False), np.dtype("uint32"): (4, False), np.dtype("uint64"): (8, False),
    np.dtype("int8"): (1, True), np.dtype("int16"): (2, True), np.dtype("int32"): (4, True), np.dtype("int64"): (8, True),
}


def dtype_format(dtype) -> Tuple[int, bool]:
    """(width, signed) of a numpy integer dtype; little-endian words are what the library reads."""
    dt = np.dtype(dtype)
    if dt.kind not in "iu" or dt.itemsize not in (1, 2, 4, 8):
        raise ValueError(f"dtype {dt} is not a narrow scalar format (uint8/16/32/64, int8/16/32/64)")
    if dt.itemsize > 1 and dt.newbyteorder("<") != dt:
        raise ValueError("narrow scalars are little-endian")
    return dt.itemsize, dt.kind == "i"


def full_bits(width: int, signed: bool) -> int:
    """Magnitude bits a width holds: 8 w unsigned, 8 w - 1 signed, 128 for the 32-byte form."""
    if width not in WIDTHS:
        raise ValueError(f"width must be one of {WIDTHS}, got {width}")
    return MAX_BITS if width == 32 else 8 * width - (1 if signed else 0)


def resolve_bits(width: int, bits: Optional[int], signed: bool) -> int:
    """The `bits` a call runs under: None / 0 = all the width gives (not allowed for width 32); else 1 .. min(full, 128)."""
    full = full_bits(width, signed)
    if not bits:
        if width == 32:
            raise ValueError("32-byte scalars need bits (1 .. 128)")
        return full
    if bits < 0 or bits > full:
        raise ValueError(f"bits = {bits} is beyond what {width}-byte {'signed' if signed else 'unsigned'} scalars hold ({full})")
    return int(bits)


def value_range(bits: int, signed: bool) -> Tuple[int, int]:
    """[lo, hi) of the values a call with `bits` accepts: [0, 2^bits) unsigned, [-2^bits, 2^bits) signed."""
    return (-(1 << bits) if signed else 0), 1 << bits


def pack(values: Iterable[int], width: int, signed: bool, q: Optional[int] = None) -> bytes:
    """Python integers -> n x width bytes in the narrow format (width 32 needs q for the negatives)."""
    if width not in WIDTHS:
        raise ValueError(f"width must be one of {WIDTHS}, got {width}")
    if width == 32:
        if q is None:
            raise ValueError("the 32-byte form needs the group order q")
        return widen(values, q)
    return b"".join(int(v).to_bytes(width, "little", signed=signed) for v in values)


def unpack(data: Union[bytes, bytearray, memoryview, np.ndarray], width: int, signed: bool, q: Optional[int] = None) -> List[int]:
    """n x width bytes in the narrow format -> Python integers (width 32, signed: values above q / 2 are negative)."""
    raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    if len(raw) % width:
        raise ValueError(f"buffer length {len(raw)} is not a multiple of {width}")
    out = []
    for i in range(0, len(raw), width):
        if width == 32:
            v = int.from_bytes(raw[i:i + 32], "little")
            if signed and q is not None and v > q // 2:
                v -= q
        else:
            v = int.from_bytes(raw[i:i + width], "little", signed=signed)
        out.append(v)
    return out


def widen(values: Union[Iterable[int], np.ndarray], q: int) -> bytes:
    """Narrow values as the 32-byte scalars msm_run takes: v >= 0 as v, v < 0 as q - |v| (n x 32 bytes, little-endian)."""
    if isinstance(values, np.ndarray):
        dtype_format(values.dtype)   # (refuses anything but the integer formats)
        values = values.ravel().tolist()
    out = bytearray()
    for v in values:
        v = int(v)
        if not -q < v < q:
            raise ValueError("value outside (-q, q)")
        out += (v if v >= 0 else q + v).to_bytes(32, "little")
    return bytes(out)


def bits_needed(values: Sequence[int]) -> Tuple[int, int]:
    """(unsigned, signed) magnitude bits a set of integers needs, as msm_scalar_bits counts them: the smallest `bits` with every
    value in [0, 2^bits) resp. [-2^bits, 2^bits); 0 for an all-zero set.  Unsigned is 255 if a value is negative."""
    ub = sb = 0
    for v in values:
        v = int(v)
        ub = max(ub, v.bit_length() if v >= 0 else 255)
        sb = max(sb, v.bit_length() if v >= 0 else (-v - 1).bit_length())
    return ub, sb
