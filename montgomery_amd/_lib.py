"""ctypes binding of libmsm_hip.so (the C ABI in include/msm_hip.h).

There is no CPU fallback: if the HIP extension is missing or no GPU is usable, loading / creating
a context raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSM_HIP_LIB: A/B experiments with alternative builds of the same extension (tools/ab_time.py)
LIB_PATH = os.environ.get("MSM_HIP_LIB") or os.path.join(_HERE, "libmsm_hip.so")

MSM_OK, MSM_ERR_ARG, MSM_ERR_HIP, MSM_ERR_POINT, MSM_ERR_NO_POINTS, MSM_ERR_NO_DEVICE, MSM_ERR_SCALAR, MSM_ERR_INTERNAL = range(8)
CURVE_BLS12_377_G1 = 0
CURVE_ED_ON_BLS12_377 = 1
CURVE_BLS12_381_G1 = 2
CURVE_PALLAS = 3
CURVE_BN254_G1 = 4   # the two curve cycles: 32-byte coordinates like Pallas
CURVE_GRUMPKIN = 5
CURVE_VESTA = 6
CURVES_32_BYTE = (CURVE_ED_ON_BLS12_377, CURVE_PALLAS, CURVE_BN254_G1, CURVE_GRUMPKIN, CURVE_VESTA)   # 9 limbs / 8 words
ABI_VERSION = 8   # MSM_ABI_VERSION of the include/msm_hip.h this binding was written against
N_PHASES = 8
SORT_PATH_NAMES = ("one_level", "radix", "slots", "pairs")   # MSM_SORT_* of include/msm_hip.h
PHASE_NAMES = ("total", "upload", "digits", "sort", "accumulate", "reduce", "final", "accumulate_round1")

POINTS_UNCOMPRESSED, POINTS_COMPRESSED = 0, 1
VALIDATE_NONE, VALIDATE_CURVE, VALIDATE_SUBGROUP = 0, 1, 2
NO_BAD_INDEX = (1 << 64) - 1   # *bad_index_out when every point passed

SCAN_SUM, SCAN_PRODUCT = 0, 1   # op of msm_scalars_scan
SCAN_EXCLUSIVE = 1              # its flags
SUMCHECK_PROD, SUMCHECK_R1CS = 0, 1   # shape of msm_scalars_sumcheck_round
MATRIX_TRANSPOSE = 1            # flags of msm_matrix_create
MATVEC_ACCUMULATE = 1           # flags of msm_scalars_matvec

OP_MUL, OP_SQR, OP_ADD, OP_SUB, OP_INV, OP_TO_MONT, OP_FROM_MONT, OP_INV_FERMAT, OP_INV_KALISKI, OP_INV_WORDSLICED = range(10)

# every symbol include/msm_hip.h declares
EXPORTS = (
    "msm_ctx_create", "msm_ctx_destroy", "msm_last_error", "msm_set_points", "msm_run", "msm_window_sums",
    "msm_combine", "msm_combine_curve", "msm_plan", "msm_generate_points", "msm_generate_scalars", "msm_get_points", "msm_test_fp",
    "msm_test_glv", "msm_test_batch_add", "msm_test_batch_inverse",
    "msm_ctx_create_multi", "msm_ctx_device_count", "msm_pointset_create", "msm_pointset_select", "msm_pointset_destroy",
    "msm_device_alloc", "msm_device_free", "msm_device_upload",
    "msm_test_fp_raw", "msm_test_curve_op", "msm_test_batch_add_mode",
    "msm_run_placed", "msm_combine_groups", "msm_test_bucket_reduce", "msm_set_workspace_limit",
    "msm_precompute", "msm_tables_info", "msm_tables_range", "msm_set_tables_limit", "msm_reserve",
    "msm_abi_version", "msm_abi_struct_bytes", "msm_run_batch",
    "msm_set_points_ex", "msm_validate_points", "msm_get_points_ex",
    "msm_run_narrow", "msm_run_batch_narrow", "msm_plan_narrow", "msm_scalar_bits",
    "msm_run_indexed", "msm_run_indexed_narrow",
    "msm_points_lincomb", "msm_pointset_size",
    "msm_device_download", "msm_scalars_lincomb", "msm_scalars_mul", "msm_scalars_inner", "msm_scalars_powers",
    "msm_test_bucket_sums", "msm_test_set_chunk_rows_log", "msm_test_last_sort_paths", "msm_test_digits",
    "msm_scalars_ntt", "msm_scalars_root_of_unity", "msm_scalars_ntt_max_log2n", "msm_test_set_ntt_tile_log", "msm_test_last_ntt_plan",
    "msm_test_tree_sums",
    "msm_scalars_scan", "msm_scalars_inverse", "msm_scalars_div_linear", "msm_test_set_scan_tile_log", "msm_test_last_scan_plan",
    "msm_points_mul", "msm_points_mul_base", "msm_test_set_points_mul_grid", "msm_test_set_points_mul_base_path",
    "msm_test_last_points_mul",
    "msm_points_ntt", "msm_test_set_points_ntt_grid", "msm_test_last_points_ntt",
    "msm_scalars_sumcheck_round", "msm_scalars_bind", "msm_scalars_eq", "msm_test_set_sumcheck_grid", "msm_test_last_sumcheck",
    "msm_matrix_create", "msm_matrix_destroy", "msm_matrix_info", "msm_scalars_matvec", "msm_test_set_matvec_geometry",
    "msm_test_last_matvec",
    "msm_test_live_buffers",
)


class MsmOpts(C.Structure):
    _fields_ = [("c", C.c_int32), ("unsafe", C.c_int32), ("k_lo", C.c_int32), ("k_hi", C.c_int32), ("serial", C.c_int32),
                ("no_glv", C.c_int32), ("strict", C.c_int32), ("point_lo", C.c_uint32), ("by_window", C.c_int32), ("no_tables", C.c_int32),
                ("bucket_shard", C.c_int32), ("bucket_shards", C.c_int32), ("merged_sums", C.c_int32), ("reserved_", C.c_int32)]


class MsmResult(C.Structure):
    _fields_ = [
        ("x", C.c_uint8 * 48),
        ("y", C.c_uint8 * 48),
        ("is_infinity", C.c_int32),
        ("c", C.c_int32),
        ("K", C.c_int32),
        ("rounds", C.c_int32),
        ("phase_ms", C.c_float * N_PHASES),
        ("n_pairs", C.c_uint64),
        ("max_bucket", C.c_uint64),
        ("n_pairs_algo", C.c_uint64),
        ("tables", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class MsmError(RuntimeError):
    """code: MSM_ERR_*; bad_index: the index of the first refused point (msm_set_points_ex / msm_validate_points), else None."""

    def __init__(self, code: int, message: str, bad_index=None):
        super().__init__(f"msm error {code}: {message}")
        self.code = code
        self.bad_index = bad_index


_lib = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process, whichever of torch and this package is imported first.

    The ROCm wheels of torch bundle their own libamdhip64.so (SONAME libamdhip64.so.7, found through the RPATH of torch's
    libraries under the name `libamdhip64.so`); libmsm_hip.so asks for `libamdhip64.so.7`.  With torch imported first the
    dynamic loader hands this library the runtime torch has already mapped (same SONAME).  The other way round it would map
    the system runtime for this library and then, for torch, the bundled file as a SECOND runtime -- and torch reports
    "No HIP GPUs are available".  So if a torch installation with a bundled runtime exists and is not loaded yet, that runtime
    is mapped here first: this library binds to it by SONAME, and a later `import torch` finds the very file already loaded.
    torch itself is never imported by this package."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        try:
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
        except OSError:
            pass   # the library then binds to the system runtime, as a process without torch does


def load() -> C.CDLL:
    """Load the HIP extension; raises if it has not been built (python __graft_entry__.py / make)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int32
    # a library built from another version of include/msm_hip.h keeps its symbol names but not its struct layouts
    if not hasattr(lib, "msm_abi_version"):
        raise ImportError(f"{LIB_PATH} predates msm_abi_version(): rebuild it (`make`)")
    lib.msm_abi_version.restype = C.c_uint32
    lib.msm_abi_struct_bytes.argtypes = [C.c_int]
    lib.msm_abi_struct_bytes.restype = C.c_uint32
    got = (lib.msm_abi_version(), lib.msm_abi_struct_bytes(0), lib.msm_abi_struct_bytes(1))
    want = (ABI_VERSION, C.sizeof(MsmOpts), C.sizeof(MsmResult))
    if got != want:
        raise ImportError(f"{LIB_PATH}: ABI (version, sizeof msm_opts, sizeof msm_result) = {got}, this binding expects {want}; "
                          "rebuild the library and the binding from the same include/msm_hip.h")
    lib.msm_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.msm_ctx_create.restype = C.c_int
    lib.msm_ctx_destroy.argtypes = [vp]
    lib.msm_ctx_destroy.restype = None
    lib.msm_last_error.argtypes = [vp]
    lib.msm_last_error.restype = C.c_char_p
    lib.msm_set_points.argtypes = [vp, vp, u64, C.c_int, C.c_int]
    lib.msm_run.argtypes = [vp, vp, u64, C.c_int, C.POINTER(MsmOpts), C.POINTER(MsmResult)]
    lib.msm_window_sums.argtypes = [vp, vp, u64, C.c_int, C.POINTER(MsmOpts), vp, C.POINTER(MsmResult)]
    lib.msm_combine.argtypes = [vp, vp, i32, i32, C.POINTER(MsmResult)]
    lib.msm_combine_curve.argtypes = [i32, vp, i32, i32, C.POINTER(MsmResult)]
    lib.msm_combine_curve.restype = i32
    lib.msm_combine_groups.argtypes = [i32, vp, i32, i32, i32, C.POINTER(MsmResult)]
    lib.msm_run_batch.argtypes = [vp, C.POINTER(vp), C.c_uint32, u64, C.c_int, C.POINTER(MsmOpts), C.POINTER(MsmResult)]
    # narrow scalars: new symbols under ABI 8 (a library without msm_run_narrow predates them)
    if not hasattr(lib, "msm_run_narrow"):
        raise ImportError(f"{LIB_PATH} predates msm_run_narrow: rebuild it (`make`)")
    lib.msm_run_narrow.argtypes = [vp, vp, u64, C.c_int, i32, i32, i32, C.POINTER(MsmOpts), C.POINTER(MsmResult)]
    lib.msm_run_batch_narrow.argtypes = [vp, C.POINTER(vp), C.c_uint32, u64, C.c_int, i32, i32, i32, C.POINTER(MsmOpts),
                                         C.POINTER(MsmResult)]
    lib.msm_plan_narrow.argtypes = [vp, u64, i32, C.POINTER(MsmOpts), C.POINTER(i32), C.POINTER(i32)]
    lib.msm_scalar_bits.argtypes = [vp, vp, u64, C.c_int, C.POINTER(i32), C.POINTER(i32)]
    # indexed (sparse) MSM: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_run_indexed"):
        raise ImportError(f"{LIB_PATH} predates msm_run_indexed: rebuild it (`make`)")
    lib.msm_run_indexed.argtypes = [vp, vp, C.POINTER(C.c_uint32), u64, C.c_int, C.POINTER(MsmOpts), C.POINTER(MsmResult)]
    lib.msm_run_indexed_narrow.argtypes = [vp, vp, C.POINTER(C.c_uint32), u64, C.c_int, i32, i32, i32, C.POINTER(MsmOpts),
                                           C.POINTER(MsmResult)]
    # point-set linear combinations: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_points_lincomb"):
        raise ImportError(f"{LIB_PATH} predates msm_points_lincomb: rebuild it (`make`)")
    lib.msm_points_lincomb.argtypes = [vp, i32, u64, vp, i32, u64, vp, u64, i32]
    lib.msm_pointset_size.argtypes = [vp, i32, C.POINTER(u64)]
    # resident scalar-vector operations and the download: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_scalars_lincomb"):
        raise ImportError(f"{LIB_PATH} predates msm_scalars_lincomb: rebuild it (`make`)")
    lib.msm_device_download.argtypes = [vp, vp, vp, u64]
    lib.msm_scalars_lincomb.argtypes = [vp, vp, vp, vp, vp, vp, u64]
    lib.msm_scalars_mul.argtypes = [vp, vp, vp, vp, u64]
    lib.msm_scalars_inner.argtypes = [vp, vp, vp, u64, vp]
    lib.msm_scalars_powers.argtypes = [vp, vp, vp, vp, u64]
    lib.msm_run_placed.argtypes = [vp, C.POINTER(vp), u64, C.POINTER(MsmOpts), C.POINTER(MsmResult)]
    lib.msm_plan.argtypes = [vp, u64, C.POINTER(MsmOpts), C.POINTER(i32), C.POINTER(i32)]
    lib.msm_generate_points.argtypes = [vp, u64, u64, vp]
    lib.msm_generate_scalars.argtypes = [vp, u64, u64, vp, vp]
    lib.msm_get_points.argtypes = [vp, u64, u64, vp]
    lib.msm_set_points_ex.argtypes = [vp, vp, u64, C.c_int, C.c_int, C.c_int, C.POINTER(u64)]
    lib.msm_validate_points.argtypes = [vp, u64, u64, C.c_int, C.POINTER(u64)]
    lib.msm_get_points_ex.argtypes = [vp, u64, u64, C.c_int, vp]
    lib.msm_test_fp.argtypes = [vp, C.c_int, vp, vp, vp, u64]
    lib.msm_test_glv.argtypes = [vp, vp, vp, u64]
    lib.msm_test_batch_add.argtypes = [vp, vp, vp, vp, u64]
    lib.msm_test_batch_inverse.argtypes = [vp, vp, vp, u64, C.c_uint32]
    lib.msm_ctx_create_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(i32), i32]
    lib.msm_ctx_device_count.argtypes = [vp]
    lib.msm_pointset_create.argtypes = [vp, C.POINTER(i32)]
    lib.msm_pointset_select.argtypes = [vp, i32]
    lib.msm_pointset_destroy.argtypes = [vp, i32]
    lib.msm_device_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    lib.msm_device_free.argtypes = [vp, vp]
    lib.msm_device_upload.argtypes = [vp, vp, vp, u64]
    lib.msm_set_workspace_limit.argtypes = [vp, u64]
    lib.msm_precompute.argtypes = [vp, u64, C.POINTER(MsmOpts)]
    lib.msm_tables_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]
    lib.msm_tables_range.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.msm_set_tables_limit.argtypes = [vp, u64]
    lib.msm_reserve.argtypes = [vp, u64, C.POINTER(MsmOpts)]
    lib.msm_test_fp_raw.argtypes = [vp, C.c_int, vp, vp, vp, u64]
    lib.msm_test_curve_op.argtypes = [vp, C.c_int, vp, vp, vp, u64]
    lib.msm_test_batch_add_mode.argtypes = [vp, vp, vp, vp, u64, C.c_int, C.c_uint32]
    lib.msm_test_bucket_reduce.argtypes = [vp, vp, i32, C.c_uint32, C.c_int, C.c_int, vp, C.POINTER(C.c_float)]
    # the bucket finish and reduction on crafted buckets: a new test symbol under ABI 8
    if not hasattr(lib, "msm_test_bucket_sums"):
        raise ImportError(f"{LIB_PATH} predates msm_test_bucket_sums: rebuild it (`make`)")
    lib.msm_test_bucket_sums.argtypes = [vp, vp, u64, vp, vp, i32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, vp, vp]
    # the pair-form threshold and the sort-path report: new test symbols under ABI 8
    if not hasattr(lib, "msm_test_last_sort_paths"):
        raise ImportError(f"{LIB_PATH} predates msm_test_last_sort_paths: rebuild it (`make`)")
    lib.msm_test_set_chunk_rows_log.argtypes = [vp, i32]
    lib.msm_test_last_sort_paths.argtypes = [vp, C.POINTER(i32), C.c_int]
    # the digit kernels alone: a new test symbol under ABI 8
    if not hasattr(lib, "msm_test_digits"):
        raise ImportError(f"{LIB_PATH} predates msm_test_digits: rebuild it (`make`)")
    lib.msm_test_digits.argtypes = [vp, C.POINTER(vp), C.c_uint32, u64, u64, u64, i32, i32, i32, C.POINTER(MsmOpts), i32, i32, vp,
                                    C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    # the resident NTT over scalar vectors, with its test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_scalars_ntt"):
        raise ImportError(f"{LIB_PATH} predates msm_scalars_ntt: rebuild it (`make`)")
    lib.msm_scalars_ntt.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int]
    lib.msm_scalars_root_of_unity.argtypes = [vp, C.c_uint32, vp]
    lib.msm_scalars_ntt_max_log2n.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.msm_test_set_ntt_tile_log.argtypes = [vp, i32]
    lib.msm_test_last_ntt_plan.argtypes = [vp, C.POINTER(i32), C.c_int]
    # the scans, the round plan and the tree rounds on crafted buckets: a new test symbol under ABI 8
    if not hasattr(lib, "msm_test_tree_sums"):
        raise ImportError(f"{LIB_PATH} predates msm_test_tree_sums: rebuild it (`make`)")
    lib.msm_test_tree_sums.argtypes = [vp, vp, u64, vp, vp, vp, i32, C.c_uint32, i32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32,
                                       vp, C.c_uint32]
    # the resident scans, the batch inverse and the division by X - z, with their test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_scalars_scan"):
        raise ImportError(f"{LIB_PATH} predates msm_scalars_scan: rebuild it (`make`)")
    lib.msm_scalars_scan.argtypes = [vp, vp, vp, u64, C.c_int, C.c_uint32, vp, vp]
    lib.msm_scalars_inverse.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    lib.msm_scalars_div_linear.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.msm_test_set_scan_tile_log.argtypes = [vp, i32]
    lib.msm_test_last_scan_plan.argtypes = [vp, C.POINTER(i32), C.c_int]
    # per-row scalar multiplication of point sets, with its test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_points_mul"):
        raise ImportError(f"{LIB_PATH} predates msm_points_mul: rebuild it (`make`)")
    lib.msm_points_mul.argtypes = [vp, i32, u64, vp, C.c_int, u64, i32]
    lib.msm_points_mul_base.argtypes = [vp, vp, vp, C.c_int, u64, i32]
    lib.msm_test_set_points_mul_grid.argtypes = [vp, i32]
    lib.msm_test_set_points_mul_base_path.argtypes = [vp, i32]
    lib.msm_test_last_points_mul.argtypes = [vp, C.POINTER(i32), C.c_int]
    # the transform over point sets, with its test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_points_ntt"):
        raise ImportError(f"{LIB_PATH} predates msm_points_ntt: rebuild it (`make`)")
    lib.msm_points_ntt.argtypes = [vp, i32, u64, C.c_uint32, vp, vp, C.c_int, i32]
    lib.msm_test_set_points_ntt_grid.argtypes = [vp, i32]
    lib.msm_test_last_points_ntt.argtypes = [vp, C.POINTER(i32), C.c_int]
    # the resident sumcheck (round sums, variable binding, eq tables), with its test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_scalars_sumcheck_round"):
        raise ImportError(f"{LIB_PATH} predates msm_scalars_sumcheck_round: rebuild it (`make`)")
    lib.msm_scalars_sumcheck_round.argtypes = [vp, C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp]
    lib.msm_scalars_bind.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_uint32, vp]
    lib.msm_scalars_eq.argtypes = [vp, vp, vp, C.c_uint32, vp]
    lib.msm_test_set_sumcheck_grid.argtypes = [vp, i32]
    lib.msm_test_last_sumcheck.argtypes = [vp, C.POINTER(i32), C.c_int]
    # resident sparse matrices and the matrix-vector product, with their test surface: new symbols under ABI 8 as well
    if not hasattr(lib, "msm_scalars_matvec"):
        raise ImportError(f"{LIB_PATH} predates msm_scalars_matvec: rebuild it (`make`)")
    lib.msm_matrix_create.argtypes = [vp, u64, u64, u64, vp, vp, vp, C.c_int, C.c_uint32, C.POINTER(i32)]
    lib.msm_matrix_destroy.argtypes = [vp, i32]
    lib.msm_matrix_info.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.msm_scalars_matvec.argtypes = [vp, i32, vp, vp, vp, C.c_uint32]
    lib.msm_test_set_matvec_geometry.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.msm_test_last_matvec.argtypes = [vp, C.POINTER(i32), C.c_int]
    # the count of live device buffers: a new test symbol under ABI 8
    if not hasattr(lib, "msm_test_live_buffers"):
        raise ImportError(f"{LIB_PATH} predates msm_test_live_buffers: rebuild it (`make`)")
    lib.msm_test_live_buffers.argtypes = [C.POINTER(u64), C.POINTER(u64)]
    for name in EXPORTS:
        if name not in ("msm_ctx_destroy", "msm_last_error", "msm_abi_version", "msm_abi_struct_bytes"):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib
