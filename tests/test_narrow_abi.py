"""Narrow-scalar MSM at the C ABI and in the Python binding, without a GPU: the four symbols, the formats, the widening helper."""
import ctypes

import numpy as np
import pytest

from abi_surface import assert_abi_frozen, assert_names_declared

NAMES = ("msm_run_narrow", "msm_run_batch_narrow", "msm_plan_narrow", "msm_scalar_bits")
Q377 = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001


def test_header_binding_and_library_have_the_narrow_entries():
    assert_names_declared(NAMES)


def test_abi_version_and_struct_sizes_did_not_move():
    from montgomery_amd import _lib

    assert_abi_frozen(_lib.load())


def test_null_context_is_an_argument_error():
    from montgomery_amd import _lib
    from montgomery_amd._lib import MsmOpts, MsmResult

    lib = _lib.load()
    s = (ctypes.c_uint8 * 64)()
    res, o = (MsmResult * 1)(), MsmOpts()
    arr = (ctypes.c_void_p * 1)(ctypes.cast(s, ctypes.c_void_p))
    c, k = ctypes.c_int32(), ctypes.c_int32()
    assert lib.msm_run_narrow(None, s, 8, 0, 8, 0, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG
    assert lib.msm_run_batch_narrow(None, arr, 1, 8, 0, 8, 0, 0, ctypes.byref(o), res) == _lib.MSM_ERR_ARG
    assert lib.msm_plan_narrow(None, 1024, 64, None, ctypes.byref(c), ctypes.byref(k)) == _lib.MSM_ERR_ARG
    assert lib.msm_scalar_bits(None, s, 2, 0, ctypes.byref(c), ctypes.byref(k)) == _lib.MSM_ERR_ARG


def test_python_api_has_the_narrow_entries():
    from montgomery_amd import api

    for name in ("run_narrow", "run_narrow_device", "run_batch_narrow", "run_batch_narrow_device", "plan_narrow", "scalar_bits"):
        assert callable(getattr(api.MsmContext, name))
    assert callable(api._Parallel.msmNarrow)


@pytest.mark.parametrize("name,width,signed", [("uint8", 1, False), ("uint16", 2, False), ("uint32", 4, False), ("uint64", 8, False),
                                                ("int8", 1, True), ("int16", 2, True), ("int32", 4, True), ("int64", 8, True)])
def test_dtype_to_format(name, width, signed):
    from montgomery_amd import narrow as N

    assert N.dtype_format(np.dtype(name)) == (width, signed)
    assert N.dtype_format(np.zeros(3, dtype=name).dtype) == (width, signed)
    assert N.full_bits(width, signed) == 8 * width - (1 if signed else 0)


def test_dtype_refusals():
    from montgomery_amd import narrow as N

    for bad in ("float32", "float64", "complex64", "bool", ">u4", ">i8"):
        with pytest.raises(ValueError):
            N.dtype_format(np.dtype(bad))
    assert N.dtype_format(np.dtype("<u4")) == (4, False)


def test_bits_validation():
    from montgomery_amd import narrow as N

    for w in (1, 2, 4, 8, 16):
        for sg in (False, True):
            full = 8 * w - (1 if sg else 0)
            assert N.resolve_bits(w, None, sg) == full and N.resolve_bits(w, 0, sg) == full
            assert N.resolve_bits(w, 1, sg) == 1 and N.resolve_bits(w, full, sg) == full
            with pytest.raises(ValueError):
                N.resolve_bits(w, full + 1, sg)
            with pytest.raises(ValueError):
                N.resolve_bits(w, -1, sg)
    assert N.full_bits(16, False) == 128 and N.full_bits(32, True) == 128
    assert N.resolve_bits(32, 128, True) == 128 and N.resolve_bits(32, 1, False) == 1
    for bad in (None, 0, 129, 255):
        with pytest.raises(ValueError):
            N.resolve_bits(32, bad, False)
    with pytest.raises(ValueError):
        N.full_bits(3, False)
    assert N.value_range(7, True) == (-128, 128) and N.value_range(8, False) == (0, 256)


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("signed", [False, True])
def test_widen_against_python_integers(width, signed):
    """pack -> unpack is the identity and widen writes v resp. q - |v|, at the extremes 0, 2^bits - 1 and -2^bits too."""
    from montgomery_amd import narrow as N

    q = Q377
    bits = N.full_bits(width, signed)
    lo, hi = N.value_range(bits, signed)
    rng = np.random.default_rng(width * 2 + signed)
    vals = [0, 1, hi - 1, hi // 2, lo] + [int(x) % (hi - lo) + lo for x in rng.integers(0, 1 << 62, size=40).tolist()]
    if signed:
        vals += [-1, lo + 1]
    raw = N.pack(vals, width, signed, q)
    assert len(raw) == width * len(vals)
    assert N.unpack(raw, width, signed, q) == vals
    wide = N.widen(vals, q)
    assert len(wide) == 32 * len(vals)
    got = [int.from_bytes(wide[32 * i:32 * i + 32], "little") for i in range(len(vals))]
    assert got == [v % q for v in vals]
    assert all(g < q for g in got)
    if width <= 8:   # numpy arrays take the same road
        arr = np.array(vals, dtype=np.dtype(f"{'i' if signed else 'u'}{width}"))
        assert arr.tobytes() == raw and N.widen(arr, q) == wide


def test_widen_refuses_what_does_not_fit():
    from montgomery_amd import narrow as N

    with pytest.raises(ValueError):
        N.widen([Q377], Q377)
    with pytest.raises(ValueError):
        N.widen([-Q377], Q377)
    with pytest.raises(ValueError):
        N.widen(np.zeros(2, dtype=np.float32), Q377)
    with pytest.raises(OverflowError):
        N.pack([256], 1, False)
    with pytest.raises(OverflowError):
        N.pack([-129], 1, True)


def test_bits_needed_bookkeeping():
    from montgomery_amd import narrow as N

    assert N.bits_needed([0, 0]) == (0, 0)
    assert N.bits_needed([1]) == (1, 1)
    assert N.bits_needed([255, 3]) == (8, 8)
    assert N.bits_needed([-1]) == (255, 0)
    assert N.bits_needed([-128, 127]) == (255, 7)
    assert N.bits_needed([-129]) == (255, 8)
    assert N.bits_needed([(1 << 128) - 1, -(1 << 128)]) == (255, 128)
