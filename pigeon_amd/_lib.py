"""ctypes binding of libpigeon_hip.so (include/pigeon_hip.h).  The product path has NO fallback: if the HIP
library is missing or there is no GPU, importing/using the ops raises -- loudly (see `require_gpu`)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PIGEON_HIP_LIB lets a developer A/B two builds of the library in one process launch (tools/); default = in-tree build
LIB_PATH = os.environ.get("PIGEON_HIP_LIB") or os.path.join(_HERE, "libpigeon_hip.so")

PG_DTYPE_F32, PG_DTYPE_BF16, PG_DTYPE_F16, PG_DTYPE_F64, PG_DTYPE_U8 = 0, 1, 2, 3, 4
EPI_QKV, EPI_GELU, EPI_RESID, EPI_PATCH, EPI_F32, EPI_RESID_STAT, EPI_QKV_LN, EPI_GELU_LN, EPI_GELU_X3 = 0, 1, 2, 3, 4, 5, 6, 7, 8
PROF_CLASSES = ["gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "gemm_patch", "attention", "layernorm",
                "im2col", "token_mean"]


class PigeonHipError(RuntimeError):
    pass


class VitCfg(C.Structure):
    _fields_ = [("layers", C.c_int32), ("image_size", C.c_int32), ("patch", C.c_int32), ("hidden", C.c_int32),
                ("heads", C.c_int32), ("mlp", C.c_int32), ("ln_eps", C.c_float), ("max_chunk", C.c_int32),
                ("mma_dtype", C.c_int32), ("precise", C.c_int32)]


class Bank(C.Structure):
    _fields_ = [("proto_emb", C.c_void_p), ("cell_off", C.c_void_p), ("proto_lnglat", C.c_void_p),
                ("proto_count", C.c_void_p), ("member_off", C.c_void_p), ("member_idx", C.c_void_p),
                ("train_emb", C.c_void_p), ("train_lnglat", C.c_void_p),
                ("num_cells", C.c_int64), ("num_protos", C.c_int64), ("num_train", C.c_int64)]


class KnnBank(C.Structure):
    """pg_knn_bank (include/pigeon_hip.h): the fp32 bank, pg_knn_prepare's three arrays, the row count."""
    _fields_ = [("x", C.c_void_p), ("x16", C.c_void_p), ("hn", C.c_void_p), ("stats", C.c_void_p), ("n", C.c_int64)]


class RegionBankStruct(C.Structure):
    """pg_region_bank (include/pigeon_hip.h): five device arrays, the host copies of the two offset arrays, three counts."""
    _fields_ = [("region_off", C.c_void_p), ("ring_off", C.c_void_p), ("xy", C.c_void_p), ("ring_bbox", C.c_void_p),
                ("region_bbox", C.c_void_p), ("region_off_host", C.c_void_p), ("ring_off_host", C.c_void_p),
                ("num_regions", C.c_int64), ("num_rings", C.c_int64), ("num_vertices", C.c_int64)]


class PrepItem(C.Structure):
    """pg_prep_item (include/pigeon_hip.h): one image of a ragged preprocessing batch, PREP_ITEM_BYTES bytes."""
    _fields_ = [("src_off", C.c_uint64), ("in_h", C.c_int32), ("in_w", C.c_int32), ("new_h", C.c_int32), ("new_w", C.c_int32),
                ("top", C.c_int32), ("left", C.c_int32), ("ksize_h", C.c_int32), ("ksize_v", C.c_int32), ("row0", C.c_int32),
                ("nrows", C.c_int32), ("tmp_row", C.c_int32), ("bounds_h_off", C.c_uint32), ("kk_h_off", C.c_uint32),
                ("bounds_v_off", C.c_uint32), ("kk_v_off", C.c_uint32), ("reserved", C.c_int32 * 3)]


PREP_ITEM_BYTES = 80
assert C.sizeof(PrepItem) == PREP_ITEM_BYTES


class JpegInfo(C.Structure):
    """pg_jpeg_info (include/pigeon_hip.h): what pg_jpeg_probe reads from a file's header; reason 0 = decoded on the GPU."""
    _fields_ = [("reason", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32),
                ("vs", C.c_int32), ("reserved", C.c_int32 * 2)]


class JpegItem(C.Structure):
    """pg_jpeg_item (include/pigeon_hip.h): one image of a JPEG batch, JPEG_ITEM_BYTES bytes."""
    _fields_ = [("rgb_off", C.c_uint64), ("coef_off", C.c_uint64 * 3), ("plane_off", C.c_uint64 * 3), ("height", C.c_int32),
                ("width", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32), ("bw", C.c_int32 * 3),
                ("bh", C.c_int32 * 3), ("qsel", C.c_int32 * 3), ("reserved", C.c_int32 * 4), ("qt", (C.c_uint16 * 64) * 4)]


JPEG_ITEM_BYTES = 640
assert C.sizeof(JpegItem) == JPEG_ITEM_BYTES and C.sizeof(JpegInfo) == 32
JPEG_REASONS = ("ok", "not_jpeg", "progressive", "lossless", "hierarchical", "arithmetic", "precision", "components", "colorspace",
                "sampling", "multiscan", "dnl", "size", "malformed")          # PG_JPEG_R_*: index = code


class EqView(C.Structure):
    """pg_eq_view (include/pigeon_hip.h): what the caller knows of one view of a panorama, the input of pg_equirect_plan."""
    _fields_ = [("src_h", C.c_int32), ("src_w", C.c_int32), ("src_index", C.c_int32), ("size", C.c_int32), ("rot", C.c_double * 9),
                ("inv_f", C.c_double)]


class EqItem(C.Structure):
    """pg_eq_item (include/pigeon_hip.h): one view of an equirectangular batch, EQ_ITEM_BYTES bytes."""
    _fields_ = [("src_off", C.c_uint64), ("dst_off", C.c_uint64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("size", C.c_int32),
                ("reserved0", C.c_int32), ("rot", C.c_double * 9), ("inv_f", C.c_double), ("reserved", C.c_int32 * 4)]


EQ_ITEM_BYTES = 128
assert C.sizeof(EqItem) == EQ_ITEM_BYTES and C.sizeof(EqView) == 96


# name -> (restype, argtypes); must list EVERY symbol declared in include/pigeon_hip.h (tests check this)
_P, _I, _I64, _F, _D, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
SIGNATURES = {
    "pg_last_error": (C.c_char_p, []),
    "pg_abi_version": (_I, []),
    "pg_device_count": (_I, []),
    "pg_vit_create": (_I, [C.POINTER(_P), _I, C.POINTER(VitCfg)]),
    "pg_vit_load_weight": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_I64), _I]),
    "pg_vit_finalize": (_I, [_P]),
    "pg_vit_workspace_bytes": (_I, [_P, _I, C.POINTER(_SZ)]),
    "pg_vit_forward": (_I, [_P, _P, _I, _I, _P, _P, _SZ, _P]),
    "pg_vit_forward_hidden": (_I, [_P, _P, _I, _I, _P, _P, _P, _SZ, _P]),
    "pg_vit_precise_workspace_bytes": (_I, [_P, _I, C.POINTER(_SZ)]),
    "pg_vit_forward_precise": (_I, [_P, _P, _I, _I, _P, _P, _P, _SZ, _P]),
    "pg_vit_graph": (_I, [_P, _I, C.POINTER(_I64), C.POINTER(_I64)]),
    "pg_vit_destroy": (_I, [_P]),
    "pg_vit_mma_dtype": (_I, [_P]),
    "pg_fingerprint": (_I, [_P, _SZ, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "pg_vit_fingerprint": (_I, [_P, C.POINTER(C.c_uint64)]),
    "pg_vit_param_read": (_I, [_P, _I, _I, _P, _SZ, C.POINTER(_SZ)]),
    "pg_vit_profile_enable": (_I, [_P, _I]),
    "pg_vit_profile_read": (_I, [_P, C.POINTER(_I64), C.POINTER(_D)]),
    "pg_vit_profile_reset": (_I, [_P]),
    "pg_tune_gemm_stagger": (_I, [_F]),
    "pg_tune_gemm_tail_rows": (_I, [_I]),
    "pg_tune_gemm_tail_shape": (_I, [_I, _I]),
    "pg_tune_gemm_raster": (_I, [_I]),
    "pg_tune_gemm_mid": (_I, [_I]),
    "pg_tune_exact_attention": (_I, [_I]),
    "pg_tune_exact_products": (_I, [_I]),
    "pg_tune_exact_fusion": (_I, [_I]),
    "pg_gemm_plan": (_I, [_I, _I, _I, _I, _I, _P, _P, _P]),
    "pg_vit_saturation_check": (_I, [_P, _I]),
    "pg_vit_saturation_read": (_I, [_P, C.POINTER(_I64), _I]),
    "pg_vit_range_alarm_read": (_I, [_P, C.POINTER(_I64), _I]),
    "pg_comm_unique_id": (_I, [_P]),
    "pg_comm_init_rank": (_I, [C.POINTER(_P), _I, _P, _I]),
    "pg_comm_count": (_I, [_P, C.POINTER(_I)]),
    "pg_allgather": (_I, [_P, _P, _P, _SZ, _P]),
    "pg_allgather_many": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(_SZ), _P]),
    "pg_comm_destroy": (_I, [_P]),
    "pg_comm_rccl_version": (_I, []),
    "pg_prep_create": (_I, [C.POINTER(_P), _I, _I, _I]),
    "pg_prep_destroy": (_I, [_P]),
    "pg_prep_geometry": (_I, [_P, C.POINTER(C.c_int32)]),
    "pg_prep_workspace_bytes": (_I, [_P, _I, C.POINTER(_SZ)]),
    "pg_prep_norm_lut": (_I, [C.POINTER(_F)]),
    "pg_prep_forward": (_I, [_P, _P, _I, _P, _I, _P, _SZ, _P]),
    "pg_prep_ragged_plan": (_I, [_I, C.POINTER(C.c_int32), C.POINTER(PrepItem), C.POINTER(_SZ), C.POINTER(_SZ)]),
    "pg_prep_ragged_create": (_I, [C.POINTER(_P), _I]),
    "pg_prep_ragged_destroy": (_I, [_P]),
    "pg_prep_ragged_forward": (_I, [_P, _P, _SZ, C.POINTER(PrepItem), _I, _P, _I, _P, _SZ, _P]),
    "pg_jpeg_probe": (_I, [_P, _SZ, C.POINTER(JpegInfo)]),
    "pg_jpeg_reason": (C.c_char_p, [_I]),
    "pg_jpeg_plan": (_I, [_I, C.POINTER(JpegInfo), C.POINTER(JpegItem), C.POINTER(PrepItem), C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ),
                          C.POINTER(_SZ)]),
    "pg_jpeg_entropy_decode": (_I, [_I, C.POINTER(_P), C.POINTER(_SZ), C.POINTER(JpegItem), _P, _SZ, _I, C.POINTER(_I)]),
    "pg_jpeg_forward": (_I, [_P, _SZ, C.POINTER(JpegItem), C.POINTER(PrepItem), _I, _P, _SZ, _P, _SZ, _P]),
    "pg_equirect_plan": (_I, [_I, C.POINTER(EqView), _I, C.POINTER(C.c_uint64), C.POINTER(EqItem), C.POINTER(PrepItem), C.POINTER(_SZ),
                              C.POINTER(_SZ)]),
    "pg_equirect_forward": (_I, [_P, _SZ, C.POINTER(EqItem), C.POINTER(PrepItem), _I, _P, _SZ, _P]),
    "pg_proto_build": (_I, [_P, _I, _I64, _P, _P, _I64, _P, _P]),
    "pg_haversine_matrix": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "pg_haversine_pairs": (_I, [_P, _P, _I, _I64, _P, _P]),
    "pg_smooth_labels": (_I, [_P, _I, _I, _D, _P, _P]),
    "pg_guess_spread": (_I, [_P, _I, _I, _P, _P, _P, _I, C.POINTER(_D), _I, _P, _P, _P, _P]),
    "pg_guess_spread_plan": (_I, [_I, C.POINTER(C.c_int32)]),
    "pg_score_table": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "pg_guess_best": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "pg_guess_best_plan": (_I, [_I, _I, _I, C.POINTER(C.c_int32)]),
    "pg_temper_stats": (_I, [_P, _I64, _I, _P, C.POINTER(_D), _I, _P, _P, _P, _P, _P, _P]),
    "pg_temper_logits": (_I, [_P, _I64, _I, _D, _P, _P]),
    "pg_temper_plan": (_I, [_I64, _I, _I, C.POINTER(C.c_int32)]),
    "pg_bootstrap_indices": (_I, [_I64, C.c_uint64, _I64, _I64, _I64, _P, _P]),
    "pg_bootstrap_means": (_I, [_P, _I, _I64, _I64, C.c_uint64, _P, _P]),
    "pg_bootstrap_quantiles": (_I, [_P, _P, _I, _I64, _I64, C.c_uint64, C.POINTER(_D), _I, _P, _P]),
    "pg_bootstrap_plan": (_I, [_I64, _I64, _I, _I, C.POINTER(C.c_int32)]),
    "pg_refine_sweep": (_I, [_P, _I, _I, _I, _P, _I, _P, C.POINTER(C.c_int32), _I, C.POINTER(_F), _I, C.POINTER(_D), _I, _P, _P, _P]),
    "pg_refine_sweep_totals": (_I, [_P, _I64, _I, _I, _P, _I, _P, _P]),
    "pg_refine_sweep_plan": (_I, [_I, _I, _I64, _I, C.POINTER(_I64)]),
    "pg_knn_prepare": (_I, [_P, _I64, _P, _P, _P, _P]),
    "pg_knn_workspace_bytes": (_I, [_I64, _I, _I, C.POINTER(_SZ)]),
    "pg_knn_search": (_I, [C.POINTER(KnnBank), _P, _I, _I, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "pg_knn_plan": (_I, [_I64, _I, _I, C.POINTER(C.c_int32)]),
    "pg_tune_knn_spans": (_I, [_I]),
    "pg_haversine_blocks": (_I, [_P, _P, _P, _I, _D, _P, _P]),
    "pg_optics_graph": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "pg_optics_plan": (_I, [_I64, _I, C.POINTER(C.c_int32)]),
    "pg_tune_optics_lds_points": (_I, [_I]),
    "pg_region_locate": (_I, [C.POINTER(RegionBankStruct), _P, _P, _I64, _P, _P, _P]),
    "pg_region_classify": (_I, [C.POINTER(RegionBankStruct), _P, _P, _I64, _P, _P]),
    "pg_region_nearest": (_I, [C.POINTER(RegionBankStruct), _P, _I64, _P, _P, _P]),
    "pg_region_plan": (_I, [C.POINTER(RegionBankStruct), C.POINTER(C.c_int32)]),
    "pg_tune_region_wave_edges": (_I, [_I]),
    "pg_head_forward": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "pg_head_train_loss": (_I, [_P, _I, _I, _P, _P, _P, _I, _P, _P, _D, _D, _P, _P, _P, _P, _P]),
    "pg_head_train_update": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I64, _D, _D, _D, _D, _D, _P, _P, _P]),
    "pg_head_train_plan": (_I, [_I, C.POINTER(C.c_int32)]),
    "pg_head_margin": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "pg_head_certainty": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "pg_aux_heads_forward": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "pg_refine_forward": (_I, [C.POINTER(Bank), _P, _I, _I, _P, _P, _P, _I, _I, _F, _D, _P, _P, _P, _P, _P]),
    "pg_refine_forward_ex": (_I, [C.POINTER(Bank), _P, _I, _I, _P, _P, _P, _I, _I, _I, _F, _D, _P, _P, _P, _P, _P, _P]),
    "pg_refine_certainty": (_I, [C.POINTER(Bank), _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _F, _P, _P, _P, _P, _P]),
    "pg_refine_certainty_bank": (_I, [C.POINTER(Bank), _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _F, _P, _P, _P, _P, _F, _P]),
    "pg_requeue_append": (_I, [_P, _P, _P, _I, _F, _I, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P]),
    "pg_rows_to_slots": (_I, [_P, _I64, _P, _I, _P, _P]),
    "pg_requeue_take": (_I, [_P, _I64, _I64, _I, _I, _P, _P]),
    "pg_scatter_rows": (_I, [_P, _I64, _P, _I, _P, _I64, _I64, _I64, _I64, _P]),
    "pg_head_wstats": (_I, [_P, _I, _P, _P, _P]),
    "pg_embedding_debias": (_I, [_P, _I64, _I, _P, _P]),
    "pg_token_attribution": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _P]),
    "pg_op_gemm16": (_I, [_I, _P, _I64, _P, _P, _P, _I64, _I, _I, _I, _I, _F, _I, _P, _I, _P]),
    "pg_op_gemm16_ld": (_I, [_I, _P, _I64, _P, _I64, _P, _P, _I64, _I, _I, _I, _I, _F, _I, _P, _I, _P]),
    "pg_op_rowstat_cast": (_I, [_P, _P, _I, _P, _I64, _F, _P]),
    "pg_op_gemm16_resid_stat": (_I, [_I, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _I, _I, _I, _I, _P]),
    "pg_op_rowstat_finalize": (_I, [_P, _I, _P, _I64, _F, _P]),
    "pg_op_gemm16_ln": (_I, [_I, _P, _I64, _P, _I64, _P, _P, _P, _P, _I64, _I, _I, _I, _I, _F, _I, _I, _P]),
    "pg_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I64, _F, _P]),
    "pg_op_attention": (_I, [_I, _P, _P, _I, _P]),
    "pg_op_im2col": (_I, [_P, _I, _P, _I, _I, _P]),
    "pg_op_token_mean": (_I, [_P, _P, _I, _P]),
    "pg_op_cast_f32": (_I, [_P, _P, _I, _I64, _P]),
    "pg_op_gemm16_parts": (_I, [_I, _P, _I64, _P, _I64, _P, _P, _I, _I, _I, _I, _P]),
    "pg_op_x3_split": (_I, [_P, _P, _I64, _I, _I, _P]),
    "pg_op_x3_layernorm": (_I, [_P, _P, _P, _P, _I64, _F, _P]),
    "pg_op_attention_f32": (_I, [_P, _P, _I, _P]),
    "pg_op_attention_x3": (_I, [_P, _P, _I, _P]),
    "pg_op_x3_im2col": (_I, [_P, _I, _P, _I, _P]),
    "pg_op_sum_parts": (_I, [_P, _I, _I64, _P, _I64, _I, _P]),
    "pg_op_preln": (_I, [_P, _P, _P, _P, _P, _I64, _F, _P, _I, _P, _P]),
    "pg_vit_precise_plan": (_I, [_I, C.POINTER(C.c_int32)]),
}

_lib = None


def load():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PigeonHipError(
            f"{LIB_PATH} not found: build it with `python -m pigeon_amd.build` (hipcc, gfx950). "
            "pigeon_amd has no CPU/PyTorch fallback for its hot path.")
    # One HIP runtime per process: the library receives torch's streams and device pointers, so it must bind to the libamdhip64
    # torch has loaded (torch ships its own copy).  Loaded FIRST, libpigeon_hip.so would pull /opt/rocm's runtime in under the same
    # soname and torch would then find "No HIP GPUs" (seen when build() and smoke() ran in one process).  Importing torch here makes
    # the order irrelevant; it is the tensor container of every caller of this module anyway.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().pg_last_error()
        raise PigeonHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def require_gpu():
    """Fail loudly when the HIP path cannot run (missing library or no device)."""
    lib = load()
    n = lib.pg_device_count()
    if n <= 0:
        raise PigeonHipError("pigeon_amd needs an AMD GPU (gfx950) visible to HIP; found none. "
                             "There is no CPU fallback for the hot path.")
    return n
