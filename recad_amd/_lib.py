"""ctypes binding of librecad_hip.so (include/recad_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails this
module raises.  Pointers are taken from torch tensors with ``data_ptr()``; torch is only
the owner of device memory and streams here.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product reads no environment variable.  A/B work against a variant build of the same ABI (scripts/ only) calls
# load(path) explicitly BEFORE anything else touches the library.
LIB_PATH = os.path.join(_HERE, "lib", "librecad_hip.so")
RK_LOSS_PARTIALS = 256
RK_MAX_GRAPH_STEPS = 64
ABI_VERSION = 11
RK_LDS_SYNC_WORDS = 2560
RK_PCA_GRAM_BLOCKS = 256
RK_RANK_MAX_NK = 8   # cut-offs per rk_rank_metrics call
RK_KNN_MAX_K, RK_KNN_MAX_BAND = 128, 38720
RK_KNN_RULES = {1: "a value that is not an integer in 1..127", 2: "column ids not strictly ascending inside [0, n_items)",
                3: "a squared norm of 2^31 or more", 4: "row pointers that decrease or are negative"}
RK_CS_MAX_CELLS, RK_CS_MAX_ITEMS = 8192, 1 << 26
RK_CS_RULES = {17: "a negative deg_item or reach, or reach 0 at a rated item", 18: "more than RK_CS_MAX_CELLS cells"}
RK_CS_FORM_AUTO, RK_CS_FORM_WAVE, RK_CS_FORM_WORKGROUP = 0, 1, 2
RK_CS_SCORE_SYNC, RK_CS_SCORE_NORMALITY, RK_CS_SCORE_RESIDUAL = 0, 1, 2
RK_FD_MAX_NODES, RK_FD_MAX_NNZ, RK_FD_WEIGHT_ONE, RK_FD_STEPS_PER_LAUNCH = 1 << 19, 1 << 29, 1 << 24, 4096
RK_FD_RULES = {19: "a weight-table entry outside 1..2^24", 20: "a column length outside 0..n_users"}
RK_ITEMKNN_MAX_BAND, RK_ITEMKNN_MAX_ITEMS, RK_ITEMKNN_MAX_USER_BLOCK = 39872, 163776, 16
RK_RP3_MAX_BAND, RK_RP3_MAX_USERS = 19904, 1 << 23
RK_USERKNN_MAX_BAND = 19904
RK_EASE_MAX_ITEMS, RK_EASE_BLOCK_SMALL, RK_EASE_BLOCK_LARGE = 65536, 32, 64
RK_EASE_BAD_GRAM, RK_EASE_NOT_SPD = 5, 6
RK_IALS_MAX_DIM, RK_IALS_CHUNK, RK_IALS_GRAM_ROWS, RK_IALS_NOT_SPD = 128, 64, 256, 7
RK_PGA_MAX_TARGETS = 64
RK_SLIM_MAX_ITEMS, RK_SLIM_BAD_DIAG = 20464, 8
RK_APR_MAX_DIM, RK_APR_MAX_BATCH = 256, 65536
RK_APR_MAX_GROUP = 64     # members of one rk_apr_train_epoch_group call
RK_APR_RULES = {9: "a user id outside [0, n_users)", 10: "a positive item id outside [0, n_items)",
                11: "a negative item id outside [0, n_items)"}


class HipLibraryMissing(RuntimeError):
    pass


class HipCallError(RuntimeError):
    pass


class LdsInfo(C.Structure):
    """rk_lds_info (include/recad_hip.h)."""

    _fields_ = [
        ("n_wg", C.c_int32), ("lds_bytes", C.c_int32), ("lpa", C.c_int32), ("lpb", C.c_int32),
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32), ("lsu", C.c_int32), ("lsi", C.c_int32),
        ("chunk", C.c_int32), ("wgx_ofs", C.c_int32), ("dinv_ofs", C.c_int32), ("perm0_ofs", C.c_int32), ("perm1_ofs", C.c_int32),
        ("mq_ofs", C.c_int32), ("reserved", C.c_int32),
    ]


class LdsEpilogue(C.Structure):
    """rk_lds_epilogue (include/recad_hip.h)."""

    _fields_ = [
        ("add", C.c_void_p), ("y", C.c_void_p), ("sum_in", C.c_void_p), ("sum_out", C.c_void_p),
        ("sum_scale", C.c_float), ("y_row_major", C.c_int32), ("sum_out_row_major", C.c_int32), ("adam_t", C.c_int32),
        ("zero1", C.c_void_p), ("zero2", C.c_void_p),
        ("adam_p", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("adam_shadow", C.c_void_p), ("coef_scratch", C.c_void_p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("stamps", C.c_void_p),
    ]


class LightGCNDesc(C.Structure):
    """rk_lightgcn_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32), ("n_layers", C.c_int32),
        ("lam", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("reserved0", C.c_int32),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("wave_desc", C.c_void_p),
        ("n_blocks", C.c_int32), ("reserved1", C.c_int32),
        ("user_emb", C.c_void_p), ("item_emb", C.c_void_p),
        ("m_user", C.c_void_p), ("v_user", C.c_void_p), ("m_item", C.c_void_p), ("v_item", C.c_void_p),
        ("buf_a", C.c_void_p), ("buf_b", C.c_void_p), ("light", C.c_void_p), ("gprop", C.c_void_p), ("gego", C.c_void_p),
        ("grad", C.c_void_p), ("state", C.c_void_p), ("coef", C.c_void_p),
        ("spmm_scratch", C.c_void_p),
        ("row_bits", C.c_void_p),
        ("keep_prob", C.c_float), ("reserved3", C.c_int32), ("drop_seed", C.c_uint64), ("tpos", C.c_void_p),
        ("lds_plan", C.c_void_p), ("lds_info", LdsInfo), ("lsum", C.c_void_p), ("e0s", C.c_void_p), ("ms", C.c_void_p), ("vs", C.c_void_p), ("cnt", C.c_void_p),
        ("row_blocks", C.c_void_p), ("row_blocks_extra", C.c_int32), ("reserved4", C.c_int32),
        ("lds_sync", C.c_void_p),
    ]


class ScorePlan(C.Structure):
    """rk_score_plan (include/recad_hip.h): the scoring path and its shape knobs as an ARGUMENT of rk_score_topk"""

    _fields_ = [
        ("path", C.c_int32), ("panel_rows", C.c_int32), ("panel_ntw", C.c_int32), ("panel_safe", C.c_int32),
        ("nb", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32), ("K", C.c_int32), ("n_targets", C.c_int32),
        ("ld_scores", C.c_int32), ("reserved", C.c_int32 * 2), ("scratch_floats", C.c_int64),
    ]


RK_SCORE_AUTO, RK_SCORE_GEMM, RK_SCORE_PANEL = 0, 1, 2


class SpmmEpilogue(C.Structure):
    """rk_spmm_epilogue (include/recad_hip.h)."""

    _fields_ = [
        ("add", C.c_void_p), ("y", C.c_void_p), ("sum_in", C.c_void_p), ("sum_out", C.c_void_p),
        ("sum_scale", C.c_float), ("adam_t", C.c_int32), ("zero1", C.c_void_p), ("zero2", C.c_void_p),
        ("adam_p", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("coef_scratch", C.c_void_p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("src_filter", C.c_void_p),
    ]


class NCFDesc(C.Structure):
    """rk_ncf_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("factor", C.c_int32), ("n_layers", C.c_int32),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("ug", C.c_void_p), ("ig", C.c_void_p), ("um", C.c_void_p), ("im", C.c_void_p),
        ("W", C.c_void_p * 8), ("b", C.c_void_p * 8), ("pw", C.c_void_p), ("pb", C.c_void_p),
        ("grad", C.c_void_p * 24), ("m", C.c_void_p * 24), ("v", C.c_void_p * 24),
        ("acts", C.c_void_p), ("dacts", C.c_void_p), ("d0", C.c_void_p),
        ("max_batch", C.c_int32), ("reserved", C.c_int32),
        ("gemm_scratch", C.c_void_p), ("gemm_scratch_floats", C.c_int64), ("wgrad_part", C.c_void_p),
        ("mode", C.c_int32), ("dropout", C.c_float), ("drop_seed", C.c_uint64), ("drop_call", C.c_int32), ("reserved2", C.c_int32),
    ]


class GemmDesc(C.Structure):
    """rk_gemm_desc (include/recad_hip.h): one request of rk_gemm_f32, the test and diagnostic entry of the fp32 MFMA GEMM."""

    _fields_ = [
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("policy", C.c_int32),
        ("A", C.c_void_p), ("a_rs", C.c_int64), ("a_cs", C.c_int64),
        ("a_ridx", C.c_void_p), ("a_rmod", C.c_int32), ("a_roff", C.c_int32),
        ("acc_init", C.c_void_p), ("ld_init", C.c_int32), ("init_base", C.c_int32),
        ("B", C.c_void_p), ("b_rs", C.c_int64), ("b_cs", C.c_int64),
        ("C", C.c_void_p), ("ldc", C.c_int32), ("reserved0", C.c_int32),
        ("col_bias", C.c_void_p), ("row_bias", C.c_void_p),
        ("const_add", C.c_float), ("relu", C.c_int32), ("sigmoid", C.c_int32),
        ("drop_thresh24", C.c_uint32), ("drop_scale", C.c_float), ("reserved1", C.c_int32), ("drop_seed", C.c_uint64),
        ("mask", C.c_void_p), ("ldmask", C.c_int32), ("reserved2", C.c_int32),
        ("sk_part", C.c_void_p), ("sk_stride", C.c_int64), ("split_k", C.c_int32), ("reserved3", C.c_int32),
        ("scratch", C.c_void_p), ("scratch_floats", C.c_int64),
    ]


# RK_GEMM_* (include/recad_hip.h): the kernel instantiation rk_gemm_f32 reports, by value
RK_GEMM_FORMS = ("none", "skinny", "deep<1,1,64>", "deep<1,2,64>", "deep<2,2,64>", "deep<1,1,32>", "deep<1,2,32>", "deep<2,2,32>",
                 "wide<1,1>", "wide<1,2>", "wide<1,1,PLAIN>", "wide<1,1,PLAIN,GROUPED>", "tile128", "tile128<GATHER>",
                 "tile128<GATHER,PLAIN>", "tuning-variant")
RK_GEMM_POLICY_LAUNCH, RK_GEMM_POLICY_AUTO, RK_GEMM_POLICY_FWD_BLOCKED = 0, 1, 2


class AushDesc(C.Structure):
    """rk_aush_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("filler_num", C.c_int32), ("n_sel", C.c_int32), ("batch", C.c_int32),
        ("reserved", C.c_int32),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("sel", C.c_void_p),
        ("g_w1t", C.c_void_p), ("g_b1", C.c_void_p), ("g_w2", C.c_void_p), ("g_b2", C.c_void_p),
        ("d_param", C.c_void_p), ("d_m", C.c_void_p), ("d_v", C.c_void_p),
        ("touched", C.c_void_p), ("touched_list", C.c_void_p), ("n_touched", C.c_void_p), ("gslot", C.c_void_p),
        ("work", C.c_void_p), ("work_bytes", C.c_int64),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
    ]


class AiaDesc(C.Structure):
    """rk_aia_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_rows", C.c_int32), ("n_real", C.c_int32), ("n_items", C.c_int32), ("dpad", C.c_int32), ("batch", C.c_int32),
        ("n_fake_nz", C.c_int32), ("nnz_real", C.c_int64),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("x", C.c_void_p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("wd", C.c_float), ("w_pos", C.c_float),
    ]


class AprLayout(C.Structure):
    """rk_apr_layout (include/recad_hip.h): byte offsets of the workspace's areas."""

    AREAS = ("keys", "keys_in", "sort_tmp", "sort_tmp_bytes", "run", "x", "c", "slot_of", "gamma", "norm", "delta", "x_adv", "c_adv",
             "part", "grad")
    _fields_ = [("bytes", C.c_int64)] + [(k, C.c_int64) for k in AREAS] + [
        ("run_stride", C.c_int32), ("part_blocks", C.c_int32), ("max_rows", C.c_int32), ("n_steps", C.c_int32)]


class AprDesc(C.Structure):
    """rk_apr_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32), ("reserved0", C.c_int32),
        ("table", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p),
        ("lam", C.c_float), ("eps", C.c_float), ("adv_reg", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
        ("adam_eps", C.c_float), ("reserved1", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class MvaeLayout(C.Structure):
    """rk_mvae_layout (include/recad_hip.h): byte offsets of the workspace's areas, element offsets of the parameters."""

    AREAS = ("brp", "keep", "keys", "keys_in", "t_ptr", "t_row", "c", "a", "pre1", "h1", "ml", "eps", "z", "kl",
             "pre2", "h2", "logits", "lse", "nll", "dh2", "dp2", "dz", "dml", "dh1", "dp1", "grad")
    PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
    _fields_ = [("bytes", C.c_int64)] + [(k, C.c_int64) for k in AREAS] + [(k, C.c_int64) for k in PARAMS] + [
        ("n_params", C.c_int64), ("nnz_cap", C.c_int64), ("batch", C.c_int32), ("reserved", C.c_int32)]


class MvaeDesc(C.Structure):
    """rk_mvae_desc (include/recad_hip.h)."""

    _fields_ = [
        ("n_users", C.c_int32), ("n_items", C.c_int32), ("hidden", C.c_int32), ("latent", C.c_int32),
        ("rowptr", C.c_void_p), ("col", C.c_void_p),
        ("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p), ("logits_out", C.c_void_p),
        ("dropout", C.c_float), ("anneal_cap", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
        ("adam_eps", C.c_float),
        ("total_anneal_steps", C.c_int64), ("seed", C.c_uint64), ("ws_nnz_cap", C.c_int64),
        ("ws_batch", C.c_int32), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


RK_MVAE_MAX_HIDDEN, RK_MVAE_MAX_LATENT, RK_MVAE_MAX_BATCH, RK_MVAE_MAX_ITEMS = 1024, 512, 4096, 262144
RK_MVAE_RULES = {12: "a user id outside [0, n_users)", 13: "a row whose item ids are not strictly ascending inside [0, n_items)",
                 14: "a user without a train item", 15: "a step with more entries than the workspace's nnz_cap",
                 16: "an item id outside [0, n_items)"}
RK_AIA_MAX_BATCH = 256
RK_AUSH_HG, RK_AUSH_HD = 128, 150
RK_AUSH_MAX_FILLER, RK_AUSH_MAX_SELECT, RK_AUSH_MAX_PAIRS = 256, 16, 4096
RK_HEUR_MAX_FILLER, RK_HEUR_MAX_TARGETS, RK_HEUR_MAX_SELECT = 256, 64, 64
RK_HEUR_GLOBAL, RK_HEUR_ITEM, RK_HEUR_ONES = 0, 1, 2
RK_UBA_MAX_BUDGET, RK_UBA_MAX_TARGETS, RK_UBA_TRIALS, RK_UBA_TOPN, RK_UBA_LDS_USERS = 16, 64, 10, 10, 8000
RK_UBA_ELEMENTWISE, RK_UBA_MATRIX = 0, 1
RK_UBA_PATH_AUTO, RK_UBA_PATH_LDS, RK_UBA_PATH_WORK = 0, 1, 2
RK_AP_HG, RK_AP_HG_REAL, RK_AP_HD1, RK_AP_HD2 = 128, 125, 512, 128
RK_AP_D_WORK_PER_ROW = 2 * RK_AP_HD1 + 2 * RK_AP_HD2 + 3

_lib = None

# name -> argtypes (restype is always int unless listed in _RESTYPES)
_P, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
_SIGNATURES = {
    "rk_abi_version": [],
    "rk_last_error": [],
    "rk_device_info": [C.c_char_p, _I32, C.POINTER(_I32)],
    "rk_coo_to_csr": [_I32, _I64, _P, _P, _P, _P, _P, _P, _P],
    "rk_csr_schedule_build": [_I32, _P, _I32, _I32, _P, C.POINTER(_P), C.POINTER(_I32), C.POINTER(_I64), C.POINTER(_I64)],
    "rk_csr_schedule_build_host": [_I32, _P, _I32, _I32, C.POINTER(_P), C.POINTER(_I32), C.POINTER(_I64), C.POINTER(_I64)],
    "rk_csr_schedule_build_host_ex": [_I32, _P, _I32, _I32, _I32, _I32, _I32, C.POINTER(_P), C.POINTER(_I32), C.POINTER(_I64), C.POINTER(_I64)],
    "rk_csr_schedule_words": [_P, _P],
    "rk_csr_schedule_upload": [_P, _P, _P],
    "rk_csr_schedule_destroy": [_P],
    "rk_build_norm_adj": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P],
    "rk_spmm_csr": [_I32, _P, _P, _P, _P, _I32, _P, _I32, _P, _P, _P, _P],
    "rk_spmm_csr_ex": [_I32, _P, _P, _P, _P, _I32, _P, _I32, _P, _I64, C.POINTER(SpmmEpilogue), _P],
    "rk_lds_plan_build": [_I32, _I32, _P, _P, _P, _I32, _P, C.POINTER(_P), C.POINTER(_I64), C.POINTER(LdsInfo)],
    "rk_lds_plan_build_host": [_I32, _I32, _P, _P, _P, _I32, _I32, C.POINTER(_P), C.POINTER(_I64), C.POINTER(LdsInfo)],
    "rk_lds_plan_build_host_ex": [_I32, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, C.POINTER(_P), C.POINTER(_I64), C.POINTER(LdsInfo)],
    "rk_lds_plan_words": [_P, _P],
    "rk_lds_plan_upload": [_P, _P, _P],
    "rk_lds_plan_destroy": [_P],
    "rk_lds_pack": [C.POINTER(LdsInfo), _P, _P, _I32, _I64, _P],
    "rk_lds_unpack": [C.POINTER(LdsInfo), _P, _P, _I32, _I64, _P],
    "rk_spmm_lds": [C.POINTER(LdsInfo), _P, _P, C.POINTER(LdsEpilogue), _P],
    "rk_rows_gather_masked": [_I32, _P, _P, _P, _I64, _P, _P],
    "rk_rows_zero": [_I32, _P, _P, _P, _I64, _P],
    "rk_rows_mark_bits": [_P, _P, _I64, _I32, _P],
    "rk_adam_coef_advance": [_P, _P, _F, _F, _F, _P],
    "rk_bpr_rows": [_I32, _I32, _F, _P, _I32, _P, _P, _P, _P, _P, _P, _I32, _P, _P],
    "rk_bpr_rows_ordered": [_I32, _I32, _F, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P],
    "rk_lightgcn_create": [C.POINTER(LightGCNDesc), C.POINTER(_P)],
    "rk_lightgcn_destroy": [_P],
    "rk_lightgcn_sync_status": [_P, C.POINTER(_I32), _P],
    "rk_lightgcn_propagate": [_P, _P],
    "rk_lightgcn_propagate_dropout": [_P, C.c_uint64, _P],
    "rk_lightgcn_train_epoch": [_P, _P, _P, _P, _I64, _I32, _I32, _P, _I32, _I32, _P],
    "rk_lightgcn_prepare": [_P, _I64, _I32, _I32, _I32, _P],
    "rk_lightgcn_set_deterministic": [_P, _I32],
    "rk_pair_scores": [_I32, _P, _P, _P, _P, _F, _P, _P, _I64, _P, _F, C.c_uint64, _P],
    "rk_score_matrix": [_I32, _P, _I32, _P, _P, _I32, _P, _P, _F, _F, C.c_uint64, _P, _P],
    "rk_adam_step": [_I64, _P, _P, _P, _P, _I32, _F, _F, _F, _F, _P],
    "rk_adam_step_dev": [_I64, _P, _P, _P, _P, _P, _F, _F, _F, _P],
    "rk_score_topk_plan": [_I32, _I32, _I32, _I32, _I32, C.POINTER(ScorePlan), C.POINTER(ScorePlan)],
    "rk_score_topk": [_I32, _P, _I32, _P, _P, _I32, _P, _P, _F, _P, _P, _I32, _P, _P, _P, _I32, _P, _P, C.POINTER(ScorePlan), _P, _P],
    "rk_bpr_sample": [_I32, _I32, _P, _P, _I64, C.c_uint64, _P, _P, _P, _P, _P],
    "rk_pointwise_sample": [_I32, _I32, _P, _P, _I64, _I32, C.c_uint64, _P, _P, _P, _P],
    "rk_topk_rows": [_P, _I32, _I32, _P, _P, _P, _I32, _P, _P, _P, _I32, _P, _P, _P],
    "rk_hit_counts": [_P, _I64, _I32, _P, _I32, _P, _P],
    "rk_eligible_users": [_I32, _P, _P, _P, _I32, _P, _P, _P, _P],
    "rk_pred_shift": [_P, _P, _I64, _P, _P],
    "rk_rank_metrics": [_P, _I64, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P],
    "rk_users_rating": [_I32, _P, _I32, _P, _P, _I32, _P, _P],
    "rk_ncf_forward": [C.POINTER(NCFDesc), _P, _P, _P, _I32, _I64, _P, _P],
    "rk_ncf_train_epoch": [C.POINTER(NCFDesc), _P, _P, _P, _I64, _I32, _I32, _P, _I32, _P],
    "rk_gemm_f32": [C.POINTER(GemmDesc), C.POINTER(_I32), C.POINTER(_I32), _P],
    "rk_mf_train_epoch": [_I32, _I32, _I32, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _F, _F,
                          _F, _P, _I32, _F, C.c_uint64, _P],
    "rk_pca_transpose": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P],
    "rk_pca_col_scale": [_I32, _I32, _P, _P, _P, _P, _P],
    "rk_pca_spmm": [_I32, _P, _P, _P, _P, _P, _I32, _P, _P, _P],
    "rk_pca_sq_spmv": [_I32, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P],
    "rk_pca_gram": [_I64, _P, _I32, _P, _I32, _P, _P, _P],
    "rk_pca_update": [_I64, _P, _I32, _P, _I32, _P, _P],
    "rk_pca_select": [_I32, _P, _I32, _P, _P],
    "rk_knn_norms": [_I32, _I32, _P, _P, _P, _P, _P, _P],
    "rk_knn_degsim": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "rk_knn_select": [_I32, _P, _I32, _I32, _P, _P],
    "rk_cs_features": [_I32, _I32, _P, _P, _P, _P, _P, _P],
    "rk_cs_cells": [_I32, _P, _P, _I32, _P, _P, _P, _P, _P],
    "rk_cs_user_sums": [_I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "rk_cs_scores": [_I32, _P, _P, _P, _P, _I32, _I32, _P, _P],
    "rk_fd_init": [_I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rk_fd_peel_ex": [_I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _P],
    "rk_fd_peel": [_I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rk_itemknn_neighbors": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "rk_itemknn_scores": [_I32, _I32, _P, _P, _P, _P, _P, _I32, _P, _I32, _P, _P],
    "rk_itemknn_pair_scores": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P],
    "rk_rp3_steps": [_I32, _P, _P, C.c_double, _P, _P, _P],
    "rk_rp3_factors": [_I32, _P, C.c_double, C.c_double, _P, _P, _P],
    "rk_rp3_neighbors": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P],
    "rk_rp3_scores": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _P, _I32, _P, _P],
    "rk_rp3_pair_scores": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P],
    "rk_userknn_scores": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _P, _I32, _I32, _P, _P],
    "rk_userknn_pair_scores": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P, _P],
    "rk_ease_gram": [_I32, _I32, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P],
    "rk_ease_invert": [_I32, _P, _P, _I64, _I32, _P, _P],
    "rk_ease_weights": [_I32, _P, _P, _P],
    "rk_ease_scores": [_I32, _P, _P, _P, _P, _I32, _P, _P, _P],
    "rk_ease_pair_scores": [_I32, _I32, _P, _P, _P, _P, _P, _P, _I64, _P, _P],
    "rk_ials_gram": [_I32, _I32, _P, _F, _P, _P, _I64, _P],
    "rk_ials_gram64": [_I32, _I32, _P, _P, _P],
    "rk_ials_system": [_I32, _I32, _P, _P, _P, _P, _F, _P, _I32, _P, _P, _P, _P],
    "rk_ials_half_sweep": [_I32, _I32, _I32, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P],
    "rk_ials_objective": [_I32, _I32, _I32, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P],
    "rk_ials_solve_rhs": [_I32, _I32, _I32, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P],
    "rk_pga_loss": [_I32, _I32, _P, _P, _P, _I32, _I32, _P, C.c_double, _P, _P],
    "rk_pga_loss_sum": [_I64, _P, _P, _P],
    "rk_pga_add_blocks": [_I64, _I32, _P, _P, _P],
    "rk_pga_user_adjoint": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _F, _P, _P],
    "rk_pga_grad": [_I32, _I32, _I32, _P, _P, _P, _P, _P, _F, _P, _P, _P],
    "rk_pga_step": [_I32, _I32, _P, _P, _P, _F, _I32, _P, _I32, _P, _P],
    "rk_slim_fit": [_I32, _P, _F, _I32, _P, _P, _P, _P, _P],
    "rk_apr_workspace": [_I32, _I32, _I32, _I64, _I32, C.POINTER(AprLayout)],
    "rk_apr_train_epoch": [C.POINTER(AprDesc), _P, _P, _P, _I64, _I32, _I32, _I32, _P, _P, _P],
    # host arrays: descs [n_rep], users / pos / neg / losses (n_rep device pointers each), n (int64 [n_rep]), adam_t0 (int32 [n_rep])
    "rk_apr_train_epoch_group": [_I32, C.POINTER(AprDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_int64), _I32, C.POINTER(C.c_int32), _I32, C.POINTER(C.c_void_p), _P, _P],
    "rk_mvae_workspace": [_I32, _I32, _I32, _I32, _I64, C.POINTER(MvaeLayout)],
    "rk_mvae_train_epoch": [C.POINTER(MvaeDesc), _P, _I64, _I32, _I64, _I32, _P, _P, _P],
    "rk_mvae_scores": [C.POINTER(MvaeDesc), _P, _I32, _P, _I64, _P],
    "rk_mvae_pair_scores": [C.POINTER(MvaeDesc), _P, _P, _I64, _P, _P],
    "rk_aush_workspace_bytes": [_I32, _I32, _I32, C.POINTER(_I64)],
    "rk_aush_eligible": [_I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, C.POINTER(_I32), _P],
    "rk_aush_permute": [_I32, _P, C.c_uint64, C.c_uint64, _P, _P],
    "rk_aush_sample": [_I32, _P, _I32, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, _I64, _P, _I32, _P, _P, _P, _P, _P],
    "rk_aush_zr": [_I32, _I32, _I32, _P, C.c_double, C.c_uint64, C.c_uint64, _P, _P],
    "rk_aush_gen": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P],
    "rk_aush_d_step": [C.POINTER(AushDesc), _I32, _P, _P, _P, _P, _P, _P, _I32, _P, _P],
    "rk_aush_train_epoch": [C.POINTER(AushDesc), _P, _I32, _P, _P, C.c_uint64, C.c_uint64, C.c_double, _I32, _P, _P, _P, _P, _P, _P,
                            _P, _P, _P],
    "rk_aush_fake_assemble": [_I32, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _I32, _P, _P, _P],
    "rk_heur_item_stats": [_I32, _I64, _P, _P, _P, _P, _P, _P, _P],
    "rk_heur_popular": [_I32, _P, _I32, _P, _P, C.POINTER(_I32), _P],
    "rk_heur_generate": [_I32, _I32, _I32, _P, _I32, _P, _I32, _I32, C.c_double, C.c_double, _P, _P, _P, _P, C.c_uint64, C.c_uint64,
                         _P, _P],
    "rk_uba_workspace_bytes": [_I32, _I32, _I32, _I32, _I32, C.POINTER(_I64)],
    "rk_uba_redraw": [_I32, _I32, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _P, C.c_uint64, _I32, _P, _P, _P, _P, _P],
    "rk_uba_scores": [_I32, _I32, _I64, _P, _P, _P, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P],
    "rk_uba_prob": [_I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, C.c_uint64, _I32, _P, C.POINTER(_I32), _P],
    "rk_aia_project": [_I32, _P, _P, _P],
    "rk_aia_forward": [C.POINTER(AiaDesc), _P, _P, _I32, _I32, _I32, _P, _I32, _I32, _P],
    "rk_aia_reverse": [C.POINTER(AiaDesc), _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P],
    "rk_aia_attack_loss": [C.POINTER(AiaDesc), _I32, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rk_aia_g_step": [_I32, _P, _P, _P, _P, _I32, _F, _F, _F, _F, _P],
    "rk_ap_g_forward": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rk_ap_g_backward": [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _F, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "rk_ap_d_step": [_I32, _I32, _P, _P, _P, _F, _I32, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P],
}
_RESTYPES = {"rk_last_error": C.c_char_p}
EXPORTS = tuple(_SIGNATURES)


def load(path):
    """Tuning scripts only: bind a variant build of the same ABI (e.g. lib/librecad_hip_tuning.so, or its bare file name
    under recad_amd/lib/) instead of the product library.  Must be called before the first lib(); the product never calls it."""
    global _lib, LIB_PATH
    if _lib is not None:
        raise HipCallError(f"_lib.load({path!r}): {LIB_PATH} is already loaded")
    LIB_PATH = path if os.path.isabs(path) or os.path.exists(path) else os.path.join(_HERE, "lib", path)
    return lib()


def lib():
    """Load librecad_hip.so once; raise HipLibraryMissing when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  recad_amd has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, argtypes in _SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
        if handle.rk_abi_version() != ABI_VERSION:
            raise HipLibraryMissing(f"{LIB_PATH} has ABI {handle.rk_abi_version()}, expected {ABI_VERSION}; rebuild it")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().rk_last_error()
        raise HipCallError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: no CPU fallback."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipCallError("recad_amd kernels need tensors on a HIP device (got a CPU tensor); "
                           "move the model/dataset to 'cuda' first -- there is no CPU fallback")
    if not t.is_contiguous():
        raise HipCallError("recad_amd kernels need contiguous tensors")
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device=None):
    """The current HIP stream of `device` (default: the current device) as a pointer argument.  Through torch's raw accessor when it
    exists (0.3 us; torch.cuda.current_stream() builds a Stream object and resolves the device index in Python: 4 us, on every call
    of the C ABI)."""
    if _raw_stream is not None:
        if device is None:
            idx = torch.cuda.current_device()
        else:
            idx = device if isinstance(device, int) else torch.device(device).index
            if idx is None:
                idx = torch.cuda.current_device()
        return C.c_void_p(_raw_stream(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu():
    if not torch.cuda.is_available():
        raise HipCallError("no HIP device visible: recad_amd's hot path only runs on an MI355X (gfx950)")
