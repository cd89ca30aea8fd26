"""Indexed (sparse) MSM at the C ABI and in the Python binding, without a GPU: the two symbols, the host-side input checks of the
facade, and sparse_from_dense / dense_from_sparse."""
import ctypes

import numpy as np
import pytest

from abi_surface import abi_history, assert_abi_frozen, assert_names_declared

NAMES = ("msm_run_indexed", "msm_run_indexed_narrow")
Q377 = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001


def test_header_binding_and_library_have_the_indexed_entries():
    assert_names_declared(NAMES)


def test_abi_version_and_struct_sizes_did_not_move():
    from montgomery_amd import _lib

    assert "msm_run_indexed" in abi_history()                                     # the ABI-history comment says so
    assert_abi_frozen(_lib.load())


def test_null_context_is_an_argument_error():
    from montgomery_amd import _lib
    from montgomery_amd._lib import MsmOpts, MsmResult

    lib = _lib.load()
    s = (ctypes.c_uint8 * 64)()
    idx = (ctypes.c_uint32 * 2)(0, 1)
    res, o = MsmResult(), MsmOpts()
    assert lib.msm_run_indexed(None, s, idx, 2, 0, ctypes.byref(o), ctypes.byref(res)) == _lib.MSM_ERR_ARG
    assert lib.msm_run_indexed_narrow(None, s, idx, 2, 0, 8, 0, 0, ctypes.byref(o), ctypes.byref(res)) == _lib.MSM_ERR_ARG


def test_python_api_has_the_indexed_entries():
    from montgomery_amd import api

    for name in ("msm_indexed", "msm_indexed_device", "msm_indexed_narrow", "msm_indexed_narrow_device"):
        assert callable(getattr(api.MsmContext, name))
    assert callable(api._Parallel.msmIndexed) and callable(api._Parallel.msmIndexedNarrow)
    assert callable(api.sparse_from_dense) and callable(api.dense_from_sparse)


def test_index_arrays_are_checked_on_the_host():
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    for good in (np.array([3, 0, 3], dtype=np.uint32), np.array([3, 0, 3], dtype=np.int64), [3, 0, 3], (3, 0, 3),
                 np.array([3, 0, 3], dtype=">u4"), np.arange(6, dtype=np.uint16)[::2] * 0 + np.array([3, 0, 3], dtype=np.uint16)):
        out = api._index_array(good, 3)
        assert out.dtype == np.dtype("<u4") and out.flags["C_CONTIGUOUS"] and out.tolist() == [3, 0, 3]
    assert api._index_array(np.zeros(0, dtype=np.int32), 0).size == 0
    assert api._index_array(np.array([(1 << 32) - 1], dtype=np.uint64)).tolist() == [(1 << 32) - 1]
    bad = (
        np.array([0.0, 1.0]),                          # wrong dtype
        np.array([True, False]),
        np.array(["1", "2"]),
        [0, 1.5],
        np.zeros((2, 2), dtype=np.uint32),             # wrong shape
        np.array([0, -1], dtype=np.int64),             # negative
        [5, -3],
        np.array([0, 1 << 32], dtype=np.uint64),       # beyond 32 bits
        [1 << 32, 0],
    )
    for b in bad:
        with pytest.raises(MsmError) as e:
            api._index_array(b)
        assert e.value.code == MSM_ERR_ARG
    with pytest.raises(MsmError) as e:                 # wrong length
        api._index_array(np.arange(4, dtype=np.uint32), 3)
    assert e.value.code == MSM_ERR_ARG


def test_wide_scalars_are_checked_on_the_host():
    from montgomery_amd import api
    from montgomery_amd._lib import MsmError

    raw = bytes(range(64))
    assert api._wide_scalar_bytes(raw) == raw
    assert api._wide_scalar_bytes(bytearray(raw)) == raw
    assert api._wide_scalar_bytes(np.frombuffer(raw, dtype=np.uint8).reshape(2, 32)) == raw
    assert api._wide_scalar_bytes(np.frombuffer(raw, dtype=np.uint8)) == raw
    for b in (raw[:33], np.zeros((2, 31), dtype=np.uint8), np.zeros((2, 32), dtype=np.uint16), np.zeros((2, 32), dtype=np.float32),
              np.zeros((1, 2, 32), dtype=np.uint8)):
        with pytest.raises(MsmError):
            api._wide_scalar_bytes(b)


def test_torch_tensors_are_taken():
    torch = pytest.importorskip("torch")
    from montgomery_amd import api
    from montgomery_amd._lib import MsmError

    assert api._index_array(torch.tensor([4, 1, 4], dtype=torch.int64), 3).tolist() == [4, 1, 4]
    assert api._index_array(torch.tensor([4, 1], dtype=torch.int32)).dtype == np.dtype("<u4")
    with pytest.raises(MsmError):
        api._index_array(torch.tensor([1, -1]))
    with pytest.raises(MsmError):
        api._index_array(torch.tensor([1.0, 2.0]))
    t = torch.arange(64, dtype=torch.uint8).reshape(2, 32)
    assert api._wide_scalar_bytes(t) == bytes(range(64))
    idx, nz = api.sparse_from_dense(torch.tensor([0, 7, 0, 9], dtype=torch.int32))
    assert idx.tolist() == [1, 3] and nz.tolist() == [7, 9]


def test_facade_refuses_before_it_reaches_the_library():
    """The checks run before the context handle is touched: an object without one is enough to see them."""
    from montgomery_amd import api
    from montgomery_amd._lib import MSM_ERR_ARG, MsmError

    ctx = api.MsmContext.__new__(api.MsmContext)   # no library call can succeed on this object
    ctx._h, ctx._lib, ctx.coord_bytes = None, None, 48
    sc = bytes(64)
    for scalars, indices in ((sc, [0]), (sc, [0, 1, 2]), (sc, [0, -1]), (sc, np.array([0.5, 1.0])), (sc[:40], [0, 1]),
                             (np.zeros((2, 32), dtype=np.int8), [0, 1]), (sc, np.zeros((1, 2), dtype=np.uint32))):
        with pytest.raises(MsmError) as e:
            ctx.msm_indexed(scalars, indices)
        assert e.value.code == MSM_ERR_ARG
    for scalars, indices, kw in ((np.zeros(3, dtype=np.uint64), [0, 1], {}), (np.zeros(2, dtype=np.int32), [0, -1], {}),
                                 (np.zeros(2, dtype=np.float32), [0, 1], {}), (bytes(8), [0], {}), (bytes(9), [0], {"width": 8}),
                                 (np.zeros(2, dtype=np.int16), [0, 1], {"width": 4}), (np.zeros(2, dtype=np.int16), [[0, 1]], {})):
        with pytest.raises((MsmError, ValueError)):
            ctx.msm_indexed_narrow(scalars, indices, **kw)


@pytest.mark.parametrize("n,density", [(0, 0.5), (1, 1.0), (1, 0.0), (257, 0.1), (1000, 0.6), (64, 1.0), (64, 0.0)])
def test_sparse_from_dense_round_trips(n, density):
    from montgomery_amd import api

    rng = np.random.default_rng(n * 7 + int(density * 10))
    rows = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    rows[:, 31] &= 0x0F                                       # below q
    rows[rng.random(n) >= density] = 0
    if n >= 64 and density not in (0.0, 1.0):
        rows[5] = 0
        rows[5, 31] = 1                                        # non-zero in the last byte only
        rows[6] = 0
        rows[6, 0] = 1                                         # and in the first
    dense = rows.tobytes()
    idx, nz = api.sparse_from_dense(dense)
    assert idx.dtype == np.dtype("<u4") and len(nz) == 32 * idx.size
    assert idx.tolist() == [i for i in range(n) if any(dense[32 * i:32 * i + 32])]
    assert all(any(nz[32 * j:32 * j + 32]) for j in range(idx.size))
    assert api.dense_from_sparse(idx, nz, n, Q377) == dense
    idx2, nz2 = api.sparse_from_dense(rows)                   # the (n, 32) array form
    assert idx2.tolist() == idx.tolist() and nz2 == nz


def test_sparse_from_dense_on_narrow_arrays():
    from montgomery_amd import api
    from montgomery_amd._lib import MsmError

    for dt in ("uint8", "int16", "uint32", "int64"):
        a = np.array([0, 5, 0, 0, 1, 0, 3], dtype=dt)
        if np.dtype(dt).kind == "i":
            a[4] = -1
        idx, nz = api.sparse_from_dense(a)
        assert idx.tolist() == [1, 4, 6] and nz.dtype == a.dtype and nz.tolist() == a[[1, 4, 6]].tolist()
        back = np.zeros_like(a)
        back[idx] = nz
        assert back.tolist() == a.tolist()
    with pytest.raises(MsmError):
        api.sparse_from_dense(np.zeros(4, dtype=np.float64))
    with pytest.raises(MsmError):
        api.sparse_from_dense(np.zeros((2, 2), dtype=np.int32))


def test_dense_from_sparse_adds_repeats_mod_q():
    from montgomery_amd import api
    from montgomery_amd._lib import MsmError

    q = Q377
    sc = [5, q - 5, 7, q - 1, 2, 9]
    idx = [2, 2, 0, 3, 3, 0]
    raw = b"".join(s.to_bytes(32, "little") for s in sc)
    dense = api.dense_from_sparse(idx, raw, 5, q)
    got = [int.from_bytes(dense[32 * i:32 * i + 32], "little") for i in range(5)]
    assert got == [16, 0, 0, 1, 0]
    with pytest.raises(MsmError):
        api.dense_from_sparse([5], raw[:32], 5, q)
    with pytest.raises(MsmError):
        api.dense_from_sparse([0, 1], raw[:32], 5, q)
