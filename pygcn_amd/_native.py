"""ctypes binding of the C-ABI in include/gcn_spmm.h (pygcn_amd/csrc/libgcn_spmm.so).

There is NO fallback: if the HIP library is missing or does not load, every product call raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GCN_SPMM_LIB: an experiment build of the same ABI — tools/build_gemm_variant.sh; never set in product use)
LIB_PATH = os.environ.get("GCN_SPMM_LIB") or os.path.join(_HERE, "csrc", "libgcn_spmm.so")

GCN_ABI_VERSION = 26
GCN_REDUCE_SUM = 0
GCN_REDUCE_MAX = 1
GCN_DEFAULT_ITEM_COST = 64
GCN_DEFAULT_LONG_THRESH = 256
GCN_DTYPE_F32 = 0
GCN_DTYPE_BF16 = 1
GCN_DENSE_NONZERO = 0
GCN_DENSE_GREATER = 1
GCN_DENSE_SWEEP_ROWS = 8192
GCN_SAMPLE_UNIFORM = 0
GCN_SAMPLE_WEIGHT = 1
GCN_SAMPLE_STRONGEST = 2
GCN_SAMPLE_RESCALE_NONE = 0
GCN_SAMPLE_RESCALE_SUM = 1
GCN_SAMPLE_WAVE_ROW_MAX = 253
GCN_SAMPLE_WAVE_SWEEP_ROWS = 65536

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_f32p = ctypes.POINTER(ctypes.c_float)


class GcnCsrPlan(ctypes.Structure):
    """Mirror of `struct gcn_csr_plan` (include/gcn_spmm.h).  Pointers are device addresses."""
    _fields_ = [
        ("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("rowptr", ctypes.c_void_p), ("rowptr_is64", ctypes.c_int32),
        ("long_thresh", ctypes.c_int32),
        ("col", ctypes.c_void_p), ("val", ctypes.c_void_p),
        ("n_items", ctypes.c_int64), ("items", ctypes.c_void_p),
        ("n_chunks", ctypes.c_int64), ("chunk_row", ctypes.c_void_p),
        ("chunk_e0", ctypes.c_void_p),
        ("n_long", ctypes.c_int64), ("long_row", ctypes.c_void_p),
        ("long_chunk0", ctypes.c_void_p),
    ]


class GcnEpilogue(ctypes.Structure):
    """Mirror of `struct gcn_epilogue` (include/gcn_spmm.h)."""
    _fields_ = [("bias", ctypes.c_void_p), ("relu", ctypes.c_int32),
                ("dropout_p", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("b_row_nonzero", ctypes.c_void_p), ("b_nnz_rows", ctypes.c_void_p),
                ("b2", ctypes.c_void_p), ("ldb2", ctypes.c_int64), ("b_split", ctypes.c_int64),
                ("c_row_nonzero", ctypes.c_void_p), ("log_softmax", ctypes.c_int32),
                ("seed_dev", ctypes.c_void_p), ("c_row_select", ctypes.c_void_p),
                ("c_skip_zero_rows", ctypes.c_int32), ("drop_row_base", ctypes.c_int64),
                ("c_absmax", ctypes.c_void_p)]


class GcnGemmEpilogue(ctypes.Structure):
    """Mirror of `struct gcn_gemm_epilogue` (include/gcn_spmm.h)."""
    _fields_ = [("bias", ctypes.c_void_p), ("relu", ctypes.c_int32), ("dropout_p", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("seed_dev", ctypes.c_void_p),
                ("mask_src", ctypes.c_void_p), ("ld_mask", ctypes.c_int64),
                ("mask_scale", ctypes.c_float), ("mask_rows", ctypes.c_void_p),
                ("drop_row_base", ctypes.c_int64), ("keep_bits_out", ctypes.c_void_p),
                ("mask_bits", ctypes.c_void_p)]


# every symbol include/gcn_spmm.h declares: name -> (restype, [argtypes]).  The ONE statement of the
# C-ABI on the Python side: lib() binds exactly this, tests hold names and parameter counts against
# the header (and check that the library exports all of them).
i, i64, sz, f32, p = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_void_p
plan_p, ep_p = ctypes.POINTER(GcnCsrPlan), ctypes.POINTER(GcnEpilogue)
gemm_ep_p = ctypes.POINTER(GcnGemmEpilogue)
SIGNATURES = {
    "gcn_abi_version": (i, []),
    "gcn_last_error": (ctypes.c_char_p, []),
    "gcn_plan_count_host": (i, [p, i, i64, i, i, c_i64p, c_i64p, c_i64p]),
    "gcn_plan_fill_host": (i, [p, i, i64, i, i, p, i64, p, p, i64, p, p, i64]),
    "gcn_plan_device_workspace_bytes": (sz, [i64]),
    "gcn_plan_count_device": (i, [p, i, i64, i, i, p, sz, p, p]),
    "gcn_plan_fill_device": (i, [p, i, i64, i, p, sz, p, i64, p, p, i64, p, p, i64, p]),
    "gcn_spmm_workspace_bytes": (sz, [plan_p, i64]),
    "gcn_spmm_csr": (i, [plan_p, i, p, i64, p, i64, i64, p, i, p, sz, p]),
    "gcn_spmm_csr_ep": (i, [plan_p, i, p, i64, p, i64, i64, ep_p, p, sz, p]),
    "gcn_relu_dropout_backward": (i, [i, p, p, p, i64, f32, p]),
    "gcn_bwd_colsum_workspace_bytes": (sz, [i64, i64, i]),
    "gcn_log_softmax_backward_colsum": (i, [i, p, p, p, p, i64, i64, p, p, i, p, sz, p]),
    "gcn_relu_dropout_backward_colsum": (i, [i, p, p, p, p, i64, i64, f32, p, p, i, p, sz, p]),
    "gcn_nll_log_softmax_backward_colsum": (i, [i, p, p, p, p, p, i64, i64, p, sz, p]),
    "gcn_sddmm_csr": (i, [plan_p, i, p, i64, p, i64, i64, p, p]),
    "gcn_csr_transpose_host": (i, [p, i, p, p, i64, i64, p, p, p]),
    "gcn_csr_transpose_workspace_bytes": (sz, [i64, i64, i64]),
    "gcn_csr_transpose_device": (i, [p, i, p, p, i64, i64, i64, p, p, p, p, sz, p]),
    "gcn_coo_to_csr_workspace_bytes": (sz, [i64, i64, i64]),
    "gcn_coo_to_csr_device": (i, [p, p, p, i64, i64, i64, i, p, i, p, p, p, p, sz, p]),
    "gcn_row_normalize_device": (i, [p, i, p, i64, p]),
    "gcn_gemm_xw256_workspace_bytes": (sz, []),
    "gcn_gemm_xw256_f32": (i, [p, i64, p, i64, p, i64, i64, p, sz, p]),
    "gcn_gemm_xw256_h2_workspace_bytes": (sz, []),
    "gcn_gemm_xw256_f32_h2": (i, [p, i64, p, p, i64, p, i64, i64, p, p, gemm_ep_p, p, sz, p]),
    "gcn_gemm_xw256_b3_workspace_bytes": (sz, []),
    "gcn_gemm_xw256_f32_b3": (i, [p, i64, p, p, i64, p, i64, i64, p, gemm_ep_p, p, sz, p]),
    "gcn_gemm_xw256_f32_b3_logsoftmax": (i, [p, i64, p, i64, p, p, i64, i64, p, sz, p]),
    "gcn_gemm_bf16_workspace_bytes": (sz, [i64, i64]),
    "gcn_gemm_xw_bf16": (i, [p, i64, p, i64, p, i64, i64, i64, i64, gemm_ep_p, p, sz, p]),
    "gcn_gemm_atg256_workspace_bytes": (sz, [i64]),
    "gcn_gemm_atg256_f32": (i, [p, i64, p, p, i64, p, i64, p, p, p, i64, p, sz, p]),
    "gcn_gemm_atg256_f32_b3": (i, [p, i64, p, p, i64, p, i64, p, i64, p, sz, p]),
    "gcn_gemm_atg256_f32_b3_colsum": (i, [p, i64, p, p, i64, p, i64, p, i64, p, p, sz, p]),
    "gcn_gemm_atg_bf16_workspace_bytes": (sz, [i64, i64, i64]),
    "gcn_gemm_atg_bf16": (i, [p, i64, p, p, i64, p, i64, i64, i64, p, i64, p, sz, p]),
    "gcn_rows_pack_count": (i, [i, p, i64, p, i64, i64, p, p, p]),
    "gcn_rows_pack_values": (i, [i, p, i64, p, i64, i64, p, p, p]),
    "gcn_rows_unpack": (i, [i, p, p, p, i64, i64, p, i64, p]),
    "gcn_bits_row_counts": (i, [p, i64, i64, p, p]),
    "gcn_rows_pack512": (i, [p, i64, i64, p, p]),
    "gcn_spmm_csr_packed": (i, [plan_p, p, p, i64, p, i64, p, sz, p]),
    "gcn_rows_pack384": (i, [p, i64, i64, p, p]),
    "gcn_spmm_csr_packed384": (i, [plan_p, p, p, i64, p, i64, p, sz, p]),
    "gcn_bn_workspace_bytes": (sz, [i64, i64, i]),
    "gcn_bn_stats": (i, [i, p, i64, i64, i, f32, p, p, p, p, sz, p]),
    "gcn_bn_apply": (i, [i, p, p, i64, i64, i, p, p, p, p, p]),
    "gcn_bn_backward_sums": (i, [i, p, p, i64, i64, i, f32, p, p, p, p, p, sz, p]),
    "gcn_bn_backward_apply": (i, [i, p, p, p, i64, i64, i, p, p, p]),
    "gcn_bn_batched_workspace_bytes": (sz, [i64, i64, i64, i]),
    "gcn_bn_stats_batched": (i, [i, p, i64, i64, i64, i, f32, p, p, p, p, sz, p]),
    "gcn_bn_apply_batched": (i, [i, p, p, i64, i64, i64, i, p, p, p, p, p]),
    "gcn_bn_backward_sums_batched": (i, [i, p, p, i64, i64, i64, i, f32, p, p, p, p, p, sz, p]),
    "gcn_bn_backward_apply_batched": (i, [i, p, p, p, i64, i64, i64, i, p, p, p]),
    "gcn_pool_workspace_bytes": (sz, [i64, i64, i64, i]),
    "gcn_masked_colsum": (i, [i, p, p, i64, i64, i64, p, p, sz, p]),
    "gcn_masked_broadcast": (i, [i, p, p, p, i64, i64, i64, p]),
    "gcn_attn_workspace_bytes": (sz, [i64, i64, i64, i]),
    "gcn_attn_scores": (i, [i, p, p, i64, i64, i64, p, p, p, sz, p]),
    "gcn_attn_normalize": (i, [p, p, p, i64, i64, p]),
    "gcn_attn_backward": (i, [i, p, p, p, p, p, i64, i64, i64, p, sz, p]),
    "gcn_select_workspace_bytes": (sz, [i64, i64]),
    "gcn_select_kth": (i, [p, i64, i64, i64, p, p, p, sz, p]),
    "gcn_select_indices": (i, [p, i64, i64, i64, p, p, p, p, sz, p]),
    "gcn_topk_flag": (i, [p, i64, i64, p, p, p]),
    "gcn_race_keys": (i, [p, i64, i64, ctypes.c_uint64, p, p]),
    "gcn_race_keys_dev": (i, [p, i64, i64, p, p, p]),
    "gcn_eval_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "gcn_eval_ingest": (i, [p, p, i64, i64, i64, i64, p, p, p, p, p, sz, p]),
    "gcn_eval_ingest_backward": (i, [p, p, p, p, p, i64, i64, i64, i64, p, p, p]),
    "gcn_vmlp_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "gcn_vmlp_forward": (i, [p, p, i64, i64, i64, i64, i64, p, p, i64, p, p, i64, p, p, i, p, p, p, p, p, sz, p]),
    "gcn_vmlp_backward": (i, [p, p, i64, i64, i64, i64, i64, p, p, i64, p, p, i64, p, p, i, p, p,
                              p, p, p, p, p, p, p, p, sz, p]),
    "gcn_dropout_rows": (i, [i, p, i64, p, i64, i64, f32, ctypes.c_uint64, p, i64, p]),
    "gcn_csr_take_rows": (i, [p, i, p, p, p, i64, p, p, i, p, p, p, p]),
    "gcn_bn_linear_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "gcn_bn_linear_forward": (i, [p, p, p, p, p, i64, i64, i64, i64, i, p]),
    "gcn_bn_linear_backward_sums": (i, [p, p, p, p, p, i64, i64, i64, i64, i, f32, p, p, p, sz, p]),
    "gcn_bn_linear_backward_apply": (i, [p, p, p, p, p, i64, i64, i64, i64, i, p]),
    "gcn_sym_normalize_workspace_bytes": (sz, [i64]),
    "gcn_sym_normalize_device": (i, [p, i, p, p, i64, p, sz, p]),
    "gcn_csr_mirror_device": (i, [p, p, p, i64, i64, p, p, p]),
    "gcn_gather_f32": (i, [p, p, i64, i64, p, p]),
    "gcn_agg_linear_partial_rows": (i64, [i64, i64, i64, i64]),
    "gcn_agg_linear_forward": (i, [p, p, p, p, i64, i64, i64, i64, i, p]),
    "gcn_agg_linear_backward": (i, [p, p, p, i64, i64, i64, i64, i, p, p, p, i64, p]),
    "gcn_dense_to_csr_count": (i, [p, i64, i64, i64, i, f32, p, p, i64, p, p]),
    "gcn_dense_to_csr_fill": (i, [p, i64, i64, i64, i, f32, p, p, i64, p, i, p, p, p]),
    "gcn_csr_sample_rows": (i, [p, i, p, p, p, i64, i64, i, ctypes.c_uint64, ctypes.c_uint32, i, i, p, i, p, p, p]),
}
EXPORTS = tuple(SIGNATURES)

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m pygcn_amd.build` "
            "(hipcc --offload-arch=gfx950). pygcn_amd has no CPU or PyTorch fallback.")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:   # e.g. libamdhip64 not found
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    bound = []
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:      # (entry points were added without moving the ABI number)
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}: a library older than this package; "
                                     "rebuild with `python -m pygcn_amd.build`") from None
        bound.append((fn, restype, argtypes))
    for fn, restype, argtypes in bound:
        fn.restype, fn.argtypes = restype, argtypes
    if L.gcn_abi_version() != GCN_ABI_VERSION:
        raise NativeLibraryError(f"{LIB_PATH}: ABI version {L.gcn_abi_version()} != "
                                 f"{GCN_ABI_VERSION}; rebuild with `python -m pygcn_amd.build`")
    _lib = L
    return L


def check(rc, what):
    """Non-zero C-ABI return -> RuntimeError (PyTorch's convention for the ops it replaces)."""
    if rc != 0:
        msg = lib().gcn_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def launch(name, device, *args, workspace=None):
    """Call the launching entry point `name` with `args` on `device`'s current stream and raise if it
    fails.  The header's rule this relies on: `void *stream` is the LAST parameter of every entry
    point that launches, and those with a workspace end in `void *workspace, size_t workspace_bytes,
    void *stream` — `workspace=n` (the answer of the entry point's *_workspace_bytes query) allocates
    n bytes on `device` and passes them there, NULL when n is 0."""
    with torch.cuda.device(device):
        if workspace is not None:
            ws = torch.empty(workspace, dtype=torch.uint8, device=device) if workspace else None
            args += (ws.data_ptr() if workspace else None, workspace)
        check(getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)
