"""ctypes binding of libtlod.so (the C ABI declared in include/tlod.h).

This is the ONLY way the Python host side reaches the MI355X kernels.  There is no CPU
fallback anywhere in the product path: if the library is missing, or a tensor is not on
the GPU, calls raise.  (The CPU restatement under ``oracle/`` is test infrastructure and
is never imported from here.)
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libtlod.so")
# os.environ's own bytes mapping: the hot-path switches (math mode, fusion toggles) are read
# per conv / GEMM call, and os.environ.get's per-call key encode + value decode cost ~1 us
# each (~1.3k reads per ATF-R101 step; the A/B was step-neutral, profiles/r05/host_env_ab.txt).
# A plain dict lookup on the same mapping sees exported and monkeypatched values alike.
_ENV_DATA = getattr(os.environ, "_data", None)
_ENV_KEYS = {}
# CPython-private layout (POSIX: a dict of fsencoded bytes keys and values); anything else —
# Windows' upper-cased str keys, a future _Environ — takes os.environ.get (round-5 advisor)
if not (os.name == "posix" and type(_ENV_DATA) is dict
        and all(isinstance(k, bytes) and isinstance(v, bytes) for k, v in _ENV_DATA.items())
        and os.environ.get("PATH") == (os.fsdecode(_ENV_DATA[b"PATH"]) if b"PATH" in _ENV_DATA
                                       else None)):
    _ENV_DATA = None


def env(name, default=None):
    """os.environ.get(name, default), without the per-call encode / decode."""
    if _ENV_DATA is None:
        return os.environ.get(name, default)
    k = _ENV_KEYS.get(name)
    if k is None:
        k = _ENV_KEYS[name] = os.fsencode(name)
    v = _ENV_DATA.get(k)
    return default if v is None else os.fsdecode(v)


if os.environ.get("TLOD_LIB"):  # tuning builds (tools/build_variants.sh); same ABI
    LIB_PATH = os.environ["TLOD_LIB"]

c_int, c_float, c_double = ctypes.c_int, ctypes.c_float, ctypes.c_double
c_size_t, c_void_p, c_uint64 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64
P = c_void_p  # every device pointer / stream crosses as void*


class RpnCfg(ctypes.Structure):
    """tlod_rpn_cfg (include/tlod.h)."""
    _fields_ = [("pos_overlap", c_float), ("neg_overlap", c_float), ("fg_fraction", c_float),
                ("batch_size", c_int), ("clobber_positives", c_int),
                ("inside_weight", c_float), ("allowed_border", c_int)]


class RcnnCfg(ctypes.Structure):
    """tlod_rcnn_cfg (include/tlod.h)."""
    _fields_ = [("batch_size", c_int), ("fg_fraction", c_float), ("fg_thresh", c_float),
                ("bg_thresh_hi", c_float), ("bg_thresh_lo", c_float),
                ("means", c_float * 4), ("stds", c_float * 4), ("inside_weight", c_float * 4)]


# name -> (restype, argtypes)
SIGNATURES = {
    "tlod_abi_version": (c_int, []),
    "tlod_last_error": (ctypes.c_char_p, []),
    "tlod_set_cu_reserve": (c_int, [c_int]),
    "tlod_nms_workspace_bytes": (c_size_t, [c_int]),
    "tlod_nms_f32": (c_int, [P, c_int, c_int, c_float, c_int, P, P, P, c_size_t, P]),
    "tlod_roi_align_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int,
                                       c_float, P, P]),
    "tlod_roi_align_bwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int,
                                       c_float, P, P]),
    "tlod_roi_align_avg_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int,
                                           c_float, P, P]),
    "tlod_roi_align_avg_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "tlod_roi_align_avg_bwd_gather_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int,
                                                                 c_int, c_int]),
    "tlod_roi_align_avg_bwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int,
                                           c_float, P, P, c_size_t, P]),
    "tlod_roi_align_avg_s2_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                         c_int]),
    "tlod_roi_align_avg_s2_nhwc_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                                   c_int, c_float, P, P, c_size_t, P]),
    "tlod_roi_align_avg_s2_nhwc_bwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                                   c_int, c_float, P, P, c_size_t, P]),
    "tlod_roi_pool_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int,
                                      c_float, P, P, P]),
    "tlod_roi_pool_bwd_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_roi_crop_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, P, P]),
    "tlod_roi_crop_bwd_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P,
                                      P]),
    "tlod_roi_crop_pool_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                           c_float, c_int, P, P, P]),
    "tlod_roi_crop_pool_bwd_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                           c_float, c_int, P, P]),
    "tlod_proposal_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "tlod_proposal_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_float, P, P, P, c_size_t, P]),
    "tlod_anchor_target_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "tlod_anchor_target_label_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P,
                                             ctypes.POINTER(RpnCfg), P, P, c_size_t, P]),
    "tlod_anchor_target_sample_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                              ctypes.POINTER(RpnCfg), P, P, c_uint64, P, P, P, P,
                                              P, c_size_t, P]),
    "tlod_anchor_target_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P,
                                       ctypes.POINTER(RpnCfg), c_uint64, P, P, P, P, P, P,
                                       c_size_t, P]),
    "tlod_proposal_target_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "tlod_proposal_target_count_f32": (c_int, [P, c_int, c_int, P, c_int, ctypes.POINTER(RcnnCfg),
                                               P, P, c_size_t, P]),
    "tlod_proposal_target_sample_f32": (c_int, [P, c_int, c_int, P, c_int, ctypes.POINTER(RcnnCfg),
                                                P, P, P, P, c_uint64, P, P, P, P, P, P,
                                                c_size_t, P]),
    "tlod_proposal_target_f32": (c_int, [P, c_int, c_int, P, c_int, ctypes.POINTER(RcnnCfg),
                                         c_uint64, P, P, P, P, P, P, P, c_size_t, P]),
    "tlod_conv_pack_fwd_f32": (c_int, [P, c_int, c_int, c_int, P, P]),
    "tlod_conv_pack_dgrad_f32": (c_int, [P, c_int, c_int, c_int, P, P]),
    "tlod_conv_fwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "tlod_conv_dgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "tlod_conv_fwd_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P,
                                  c_size_t, P]),
    "tlod_conv_dgrad_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t,
                                    P]),
    "tlod_conv_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "tlod_conv_wgrad_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P,
                                    c_size_t, P]),
    "tlod_relu_bwd_bias_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    "tlod_sgd_clip_f32": (c_int, [P, c_int, c_float, c_float, c_float, P, P, P]),
    "tlod_sgd_clip_pack_f32": (c_int, [P, c_int, c_int, P, c_int, c_float, c_float, c_float, P, P, P]),
    "tlod_adam_clip_f32": (c_int, [P, c_int, P, c_int, c_float, c_double, c_double, c_double,
                                   c_float, P, P, P]),
    "tlod_adam_clip_pack_f32": (c_int, [P, c_int, c_int, P, c_int, P, c_int, c_float, c_double,
                                        c_double, c_double, c_float, P, P, P]),
    "tlod_conv_fwd_ex_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_int, P, c_size_t, P]),
    "tlod_relu_bwd_ex_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, P]),
    "tlod_conv_pack_bs_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "tlod_conv_pack_bs": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_conv_pack_bs_ex": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_conv_fwd_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                    c_int]),
    "tlod_conv_fwd_bs_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_int, P, c_size_t, P]),
    "tlod_conv_wgrad_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                      c_int]),
    "tlod_conv_wgrad_bs_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, P, c_size_t, P]),
    "tlod_conv_wgrad_bs_ex_f32": (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int,
                                          c_int, c_int, c_int, P, c_size_t, P]),
    "tlod_conv3x3_direct_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "tlod_conv_dgrad_bs_mask_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                            P, c_size_t, P]),
    "tlod_gemm_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "tlod_gemm_bs_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P,
                                 c_size_t, P]),
    "tlod_gemm_bs_ex_f32": (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int,
                                    c_int, P, c_size_t, P]),
    "tlod_gemm_bs_mask_f32": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                      P, c_size_t, P]),
    "tlod_conv3x3_gemm_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                        c_int]),
    "tlod_conv3x3_gemm_bs_f32": (c_int, [P, P, c_int, P, P, P, P, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, P, c_size_t, P]),
    "tlod_conv1x1_gemm_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                        c_int]),
    "tlod_conv1x1_gemm_bs_f32": (c_int, [P, P, c_int, P, P, P, P, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, P, c_size_t, P]),
    "tlod_conv1x1_gemm_bs_ex_f32": (c_int, [P, P, c_int, P, P, P, P, P, P, c_int, c_int, c_int,
                                            c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "tlod_conv1x1_small_fwd_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_int, P, P]),
    "tlod_conv1x1_small_dgrad_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, P]),
    "tlod_conv1x1_small_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "tlod_conv1x1_small_wgrad_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, P,
                                             c_size_t, P]),
    "tlod_maxpool2x2_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_maxpool2x2_relu_bwd_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, P]),
    "tlod_conv_fwd_bs_pool_f32": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_int, c_int, P]),
    "tlod_stem_conv7x7s2_f32": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "tlod_subsample2_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_upsample2_zero_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_im2col3x3_nhwc_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_gemm_nhwc3_bs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                      c_int]),
    "tlod_gemm_nhwc3_bs_f32": (c_int, [c_int, P, P, P, P, P, c_int, P, c_int, c_int, c_int, c_int,
                                       c_int, c_int, P, c_size_t, P]),
    "tlod_col2im3x3_nhwc_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_col2im3x3_nhwc_mask_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P]),
    "tlod_image_blob_u8": (c_int, [P, c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_int, P, P]),
    "tlod_detect_f32": (c_int, [P, P, P, c_int, c_int, c_int, P, P, c_float, c_float, c_float,
                                c_float, c_float, P, P, P, P]),
    "tlod_space_to_depth_f32": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "tlod_depth_to_space_f32": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "tlod_drm_fwd_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t,
                                 P]),
    "tlod_drm_relu_bwd_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "tlod_relu_dropout_f32": (c_int, [P, P, ctypes.c_longlong, c_float, c_uint64, P]),
    "tlod_relu_dropout_bwd_f32": (c_int, [P, P, P, ctypes.c_longlong, c_float, P]),
    "tlod_rpn_loss_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P, P,
                                  P]),
    "tlod_rpn_loss_bwd_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int,
                                      c_float, P, P, P, P, P]),
    "tlod_rcnn_loss_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_float, P, P, P, P]),
    "tlod_rcnn_loss_bwd_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P,
                                       P, P, P]),
    "tlod_da_loss_f32": (c_int, [P, P, P, P, P, P] + [c_int] * 8 + [P, P, P]),
    "tlod_da_loss_bwd_f32": (c_int, [P, P, P, P, P, P] + [c_int] * 8 + [P, P, P, P, P, P, P]),
    "tlod_fgbg_maps_f32": (c_int, [P, c_int, c_int, c_int, c_int, c_float, c_float, P, P, P, P]),
    "tlod_masked_nll2_f32": (c_int, [P, P, c_int, P, c_int, c_int, c_int, P, P, P]),
    "tlod_masked_nll2_bwd_f32": (c_int, [P, P, c_int, P, c_int, c_int, c_int, P, P, P, P]),
    "tlod_kd_kl_f32": (c_int, [P, P, P, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong,
                               c_int, c_float, P, P]),
    "tlod_kd_kl_bwd_f32": (c_int, [P, P, P, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong,
                                   c_int, c_float, P, P, P, P]),
    "tlod_gt_cell_mask_f32": (c_int, [P, P, c_int, c_int, c_int, P, P]),
    "tlod_roi_scale_labels_f32": (c_int, [P, c_int, P, P]),
    "tlod_us_daf_loss_f32": (c_int, [P] * 8 + [c_int] * 8 + [P] * 8),
    "tlod_us_daf_loss_bwd_f32": (c_int, [P] * 8 + [c_int] * 8 + [P] * 6),
}

# include/tlod_idf.h: the IDF extension of the ABI, bound by lib() like SIGNATURES (its own
# table and header, so the main header's ledger stays what it is)
EXT_SIGNATURES = {
    "tlod_idf_dam_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "tlod_idf_dam_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "tlod_idf_sep_fwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "tlod_idf_sep_fwd_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P,
                                     c_size_t, P]),
    "tlod_idf_sep_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P,
                                     P]),
    "tlod_idf_domain_loss_f32": (c_int, [P, c_int, c_int, P, c_int, c_int, c_float, P, P]),
    "tlod_idf_domain_loss_bwd_f32": (c_int, [P, c_int, c_int, P, c_int, c_int, c_float, P, P, P,
                                             P]),
}

# include/tlod_pa_atf.h: the PA-ATF extension (strided conv im2col / col2im, channel gate,
# prototype pooling), a third table with its own header and ledger (tests/test_pa_atf_cpu.py)
PA_ATF_SIGNATURES = {
    "tlod_im2col_f32": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "tlod_col2im_f32": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "tlod_pa_gate_f32": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P]),
    "tlod_pa_gate_bwd_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P]),
    "tlod_pa_proto_pool_fwd_f32": (c_int, [P, c_int, c_int, c_int, P, c_int, c_float, P, P, P, P,
                                           P, P]),
    "tlod_pa_proto_pool_bwd_f32": (c_int, [P, P, P, P, P, P, c_int, c_float, c_int, c_int, c_int,
                                           c_float, P, P]),
    "tlod_pa_atf_loss_f32": (c_int, [P, P, P, P, P]),
    "tlod_pa_atf_loss_bwd_f32": (c_int, [P, P, P, P, P, P]),
    "tlod_proposal_keep_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_float, P, P, P, c_size_t, P]),
    "tlod_proposal_pick_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, c_uint64, P, P]),
    "tlod_proposal_subsample_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "tlod_proposal_subsample_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_int, c_float, c_uint64, P, P, c_size_t, P]),
}

# include/tlod_roi.h: the RoIPool backward with the reference gather's membership tests, a
# fourth table with its own header (ledger: tests/test_abi.py, guard case in
# tests/test_abi_guard_gpu.py)
ROI_SIGNATURES = {
    "tlod_roi_pool_bwd_gather_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                             c_int, c_float, P, P]),
}

# include/tlod_selftrain.h: the IDF self-training extension (pseudo ground truth packed from the
# detections, the domain losses with EFocalLoss), a fifth table with its own header (ledger and
# guard cases: tests/test_selftrain_cpu.py, tests/test_selftrain_gpu.py)
SELFTRAIN_SIGNATURES = {
    "tlod_pseudo_gt_f32": (c_int, [P, P, c_int, c_int, c_double, c_int, c_uint64, P, P, P]),
    "tlod_idf_domain_loss_ef_f32": (c_int, [P, c_int, c_int, P, c_int, c_int, c_float, P, P]),
    "tlod_idf_domain_loss_ef_bwd_f32": (c_int, [P, c_int, c_int, P, c_int, c_int, c_float, P, P,
                                                P, P]),
}

# include/tlod_plan.h: host-only queries of a kernel's plan (no GPU), a sixth table with its own
# header (ledger: tests/test_wide_epilogue_cpu.py)
PLAN_SIGNATURES = {
    "tlod_conv_ws_store_map": (c_int, [c_int, c_int, c_int, P, P, P, P]),
}

_lib = None


def lib():
    """Load libtlod.so once; raise (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libtlod.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(EXT_SIGNATURES.items())
                                  + list(PA_ATF_SIGNATURES.items())
                                  + list(ROI_SIGNATURES.items())
                                  + list(SELFTRAIN_SIGNATURES.items())
                                  + list(PLAN_SIGNATURES.items())):
            if os.environ.get("TLOD_LIB") and not hasattr(L, name):
                continue  # an older tuning build (A/B timing) may predate an entry point
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what=""):
    if status != 0:
        msg = lib().tlod_last_error().decode(errors="replace")
        raise RuntimeError(f"tlod {what} failed (status {status}): {msg}")


def ptr(t):
    """Device pointer of a CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    return c_void_p(t.data_ptr())


_raw_stream = torch._C._cuda_getCurrentRawStream  # hipStream_t of a device's current stream


def _dev_index(device=None):
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, torch.device):
        return device.index if device.index is not None else torch.cuda.current_device()
    return torch.device(device).index if torch.device(device).index is not None else \
        torch.cuda.current_device()


def stream_of(t=None):
    """The current stream of t's device (hipStream_t).  (The raw accessor: the Stream object
    of torch.cuda.current_stream costs ~4 us of host time per launch, and a ResNet101 step
    makes ~270 launches through here.)"""
    return c_void_p(_raw_stream(t.get_device() if t is not None else torch.cuda.current_device()))



def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("tlod ops run on the MI355X only: got a CPU tensor "
                               "(the reference's CPU kernels are not part of this path)")


_ws_cache = {}


def workspace(nbytes, device, name):
    """Grow-only scratch buffer per (op name, device, stream) for the C ABI's
    caller-provided workspace.  Distinct names keep two-phase ops (anchor target,
    proposal target) from sharing scratch with ops launched between their phases."""
    if env("TLOD_WS_GUARD", "0") != "0":
        return _guarded_workspace(nbytes, device, name)
    key = (name, str(device), _raw_stream(_dev_index(device)))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# TLOD_WS_GUARD=1 (a test mode): no cache — every call gets a view of exactly the queried
# length inside a fresh buffer with canaries on both sides, so a kernel runs with the
# workspace its *_workspace_bytes query promised and a store past it is seen.
WS_CANARY_BYTES = 64 << 10
WS_CANARY = 0xC7
_ws_guarded = []  # (op name, whole buffer, view length), until check_workspace_guards()


def _guarded_workspace(nbytes, device, name):
    n = max(int(nbytes), 256)
    buf = torch.full((2 * WS_CANARY_BYTES + n,), WS_CANARY, dtype=torch.uint8, device=device)
    _ws_guarded.append((name, buf, n))
    return buf[WS_CANARY_BYTES:WS_CANARY_BYTES + n]


def check_workspace_guards():
    """Synchronise, verify the canaries of every workspace handed out under TLOD_WS_GUARD
    since the last check (RuntimeError naming the op on damage) and forget the buffers.
    Returns how many were checked."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    held, bad = list(_ws_guarded), []
    del _ws_guarded[:]
    for name, buf, n in held:
        front = buf[:WS_CANARY_BYTES] != WS_CANARY
        back = buf[WS_CANARY_BYTES + n:] != WS_CANARY
        nf, nb = int(front.sum()), int(back.sum())
        if nf or nb:
            bad.append(f"{name} ({n} B): {nf} bytes before, {nb} bytes past the workspace")
    if bad:
        raise RuntimeError("workspace canaries damaged: " + "; ".join(bad))
    return len(held)
