"""ctypes binding of the gfx950 C ABI (include/lfvdm_hip.h).

PyTorch is used for device memory and streams only: every call passes raw device pointers,
integer shapes and the current HIP stream.  There is NO fallback: if ``liblfvdm_hip.so`` is
missing, importing the product on a GPU path raises immediately (build it with
``python latent-flexible-video-diffusion-modeling_amd/build.py``).
"""
import atexit
import ctypes as C
import json
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFVDM_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "liblfvdm_hip.so")   # override: A/B builds

ACT_NONE, ACT_SILU = 0, 1
OUT_ROWS, OUT_NCHW = 0, 1

_lib = None

c_fp = C.c_void_p
c_i = C.c_int


class ConvArgs(C.Structure):
    _fields_ = [
        ("src0", c_fp), ("src1", c_fp), ("C0", C.c_int32), ("C1", C.c_int32), ("N", C.c_int32),
        ("Hs", C.c_int32), ("Ws", C.c_int32), ("up", C.c_int32), ("stride", C.c_int32), ("ksize", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32), ("coefA", c_fp), ("coefB", c_fp), ("act", C.c_int32),
        ("W", c_fp), ("bias", c_fp), ("Cout", C.c_int32),
        ("s2src0", c_fp), ("s2src1", c_fp), ("s2C0", C.c_int32), ("s2C1", C.c_int32), ("W2", c_fp), ("bias2", c_fp),
        ("res", c_fp), ("ldr", C.c_int32), ("resA", c_fp), ("resB", c_fp),
        ("out", c_fp), ("ldo", C.c_int32), ("out_mode", C.c_int32), ("tune", C.c_int32),
        ("splitk_ws", c_fp), ("splitk_cnt", c_fp), ("splitk_ws_floats", C.c_int64), ("splitk_cnt_ints", C.c_int64),
        ("gn_gamma", c_fp), ("gn_beta", c_fp), ("gn_film", c_fp), ("gn_out", c_fp), ("gn_film_ld", C.c_int32),
        ("gn_film_div", C.c_int32), ("gn_act", C.c_int32), ("gn_skip_raw", C.c_int32), ("gn_eps", C.c_float),
        ("gn_general", C.c_int32), ("gn_gw", C.c_int32), ("gn_ld", C.c_int32),
    ]


class GnArgs(C.Structure):
    _fields_ = [("src0", c_fp), ("src1", c_fp), ("C0", C.c_int32), ("C1", C.c_int32), ("N", C.c_int32), ("P", C.c_int32),
                ("gamma", c_fp), ("beta", c_fp), ("film", c_fp), ("film_div", C.c_int32), ("film_ld", C.c_int32),
                ("eps", C.c_float), ("act", C.c_int32), ("out", c_fp), ("cg", C.c_int32), ("ldo", C.c_int32), ("out_base", c_fp),
                ("out_col", C.c_int32), ("pad_", C.c_int32)]


class GnBwdArgs(C.Structure):
    """lfvdm_gn_bwd_args (include/lfvdm_hip.h): the fused spatial GroupNorm backward."""
    _fields_ = ([(n, c_fp) for n in ("da", "src0", "src1", "coefA", "coefB", "stats", "out0", "out1", "add", "add2", "gamma", "beta",
                                     "film", "dgamma", "dbeta", "dfilm", "sums_out", "ws")] + [("ws_floats", C.c_int64)]
                + [(n, C.c_int32) for n in ("C0", "C1", "N", "P", "act", "add_ld", "add2_ld", "film_ld", "T", "dfilm_ld")])


class ChainStage(C.Structure):
    """lfvdm_chain_stage (include/lfvdm_hip.h): one stage of a persistent level chain."""
    _fields_ = [("kind", C.c_int32), ("n_items", C.c_int32), ("flag_base", C.c_int32), ("n_flags", C.c_int32),
                ("dep_base", C.c_int32), ("dep_stride", C.c_int32), ("cfg", C.c_int32), ("kz", C.c_int32), ("nt2", C.c_int32),
                ("wg_off", C.c_int32), ("side", C.c_int32), ("wg_lo", C.c_int32), ("wg_count", C.c_int32), ("ws_off", C.c_int64), ("cnt_off", C.c_int64), ("conv", ConvArgs), ("gn", GnArgs)]


CHAIN_CONV, CHAIN_GN, CHAIN_LOCAL = 0, 1, 2
CHAIN_CTL_EPOCH, CHAIN_CTL_EXIT, CHAIN_CTL_ABORT, CHAIN_CTL_INTS = 0, 32, 64, 96


class AdamWArgs(C.Structure):
    _fields_ = [("p", c_fp), ("g", c_fp), ("m", c_fp), ("v", c_fp), ("ema", c_fp * 4), ("ema_rate", C.c_float * 4),
                ("n_ema", C.c_int32), ("n", C.c_int64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("bias_corr1", C.c_float), ("bias_corr2_sqrt", C.c_float),
                ("grad_scale", C.c_float), ("grad_sqsum", c_fp), ("skip_flag", c_fp), ("skip_flag2", c_fp)]


class RowdotJob(C.Structure):
    _fields_ = [("W", c_fp), ("b", c_fp), ("inp", c_fp), ("out", c_fp), ("K", C.c_int32), ("O", C.c_int32),
                ("M", C.c_int32), ("ldin", C.c_int32), ("ldout", C.c_int32), ("in_mode", C.c_int32),
                ("row0", C.c_int32), ("pad_", C.c_int32)]


class RowdotBwdJob(C.Structure):
    _fields_ = [("W", c_fp), ("inp", c_fp), ("dout", c_fp), ("dW", c_fp), ("db", c_fp), ("din", c_fp), ("K", C.c_int32),
                ("O", C.c_int32), ("M", C.c_int32), ("ldin", C.c_int32), ("lddout", C.c_int32), ("lddin", C.c_int32),
                ("in_mode", C.c_int32), ("task0", C.c_int32)]


class PackJob(C.Structure):
    _fields_ = [("src", c_fp), ("dst", c_fp), ("Cout", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32),
                ("transposed", C.c_int32), ("blk0", C.c_int32), ("ld", C.c_int32)]


# bumped by code that rewrites parameters through raw pointers (the fused AdamW): cached packed weights are stale
param_epoch = [0]


class UnpackJob(C.Structure):
    _fields_ = [("gp", c_fp), ("g", c_fp), ("Cout", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32), ("row0", C.c_int32),
                ("ldp", C.c_int32), ("pad_", C.c_int32)]


class RpeJob(C.Structure):
    _fields_ = [("tproj", c_fp), ("Wd", c_fp), ("bd", c_fp), ("Wout", c_fp), ("bout", c_fp), ("R", c_fp),
                ("C", C.c_int32), ("tile0", C.c_int32), ("tproj_ld", C.c_int32), ("pad_", C.c_int32), ("act", c_fp)]


class RpeBwdJob(C.Structure):
    _fields_ = [("tproj", c_fp), ("Wd", c_fp), ("bd", c_fp), ("Wout_t", c_fp), ("dR", c_fp), ("dtproj", c_fp),
                ("dWd", c_fp), ("dbd", c_fp), ("C", C.c_int32), ("tile0", C.c_int32), ("tproj_ld", C.c_int32),
                ("dtproj_ld", C.c_int32)]


class WgradJob(C.Structure):
    _fields_ = [("a", ConvArgs), ("msplit", C.c_int32), ("task0", C.c_int32)]


_SIGS = {
    "lfvdm_abi_version": ([], c_i),
    "lfvdm_conv_igemm": ([C.POINTER(ConvArgs), c_fp], c_i),
    "lfvdm_conv_igemm_config": ([C.POINTER(ConvArgs), C.POINTER(c_i), C.POINTER(c_i)], c_i),
    "lfvdm_conv_igemm_candidates": ([C.POINTER(ConvArgs), C.POINTER(c_i), c_i], c_i),
    "lfvdm_pack_conv_weight": ([c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_pack_conv_weight_up2x": ([c_fp, c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_conv_wgrad": ([C.POINTER(ConvArgs), c_fp], c_i),
    "lfvdm_pack_conv_weight_t": ([c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_unpack_conv_grad": ([c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_unpack_conv_grads": ([c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_pack_conv_weights": ([c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_conv_in": ([c_fp] * 6 + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_gn_coef": ([c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_i, C.c_float, c_fp, c_fp, c_fp], c_i),
    "lfvdm_gn_coef_stats": ([c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_i, C.c_float, c_fp, c_fp, c_fp, c_fp], c_i),
    "lfvdm_gn_apply": ([c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_i, C.c_float, c_i, c_fp, c_fp, c_fp, c_fp, c_fp], c_i),
    "lfvdm_gn_apply_part": ([c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, C.c_float, c_i, c_fp, c_i, c_fp], c_i),
    "lfvdm_gn_apply_ws_floats": ([c_i, c_i, c_i], C.c_long),
    "lfvdm_gn_apply_ws": ([c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_i, C.c_float, c_i, c_fp, c_fp, c_fp, c_fp, c_fp,
                           C.c_long, c_fp], c_i),
    "lfvdm_compose_rows": ([c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_conv_in_tick": ([c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_fp, c_i, c_fp, c_i,
                            c_fp], c_i),
    "lfvdm_conv_out_psample_ok": ([c_i] * 5, c_i),
    "lfvdm_update_x0": ([c_fp] * 9 + [c_i, c_i, c_i] + [c_fp] * 3 + [c_i, c_i, c_fp], c_i),
    "lfvdm_update_rng_x0": ([c_fp] * 9 + [c_i, c_i, c_i] + [c_fp] * 3 + [c_i, c_i, c_fp, c_fp], c_i),
    "lfvdm_conv_out_update_x0": ([c_fp] * 13 + [c_i, c_i, c_i] + [c_fp] * 3 + [c_i] * 6 + [c_fp, c_fp], c_i),
    "lfvdm_update_ms_x0": ([c_fp] * 9 + [c_i, c_i] + [c_fp] * 2 + [c_i, c_i, c_fp], c_i),
    "lfvdm_conv_out_update_ms_x0": ([c_fp] * 12 + [c_i, c_i] + [c_fp] * 2 + [c_i] * 6 + [c_fp], c_i),
    "lfvdm_known_blend": ([c_fp] * 9 + [c_i] * 4 + [c_fp], c_i),
    "lfvdm_renoise": ([c_fp] * 6 + [c_i, c_i, c_fp], c_i),
    "lfvdm_dyn_threshold_workspace": ([c_i, C.c_int64, C.POINTER(C.c_size_t)], c_i),
    "lfvdm_dyn_threshold": ([c_fp] * 5 + [c_i, c_i, c_fp, c_i, c_i, C.c_int64, C.c_double, C.c_float] + [c_fp] * 4, c_i),
    "lfvdm_cfg_workspace": ([c_i, C.c_int64, C.POINTER(C.c_size_t)], c_i),
    "lfvdm_cfg_combine": ([c_fp] * 5 + [c_i, c_i, c_fp, C.c_float, C.c_float] + [c_fp] * 3 + [c_i, c_i, C.c_int64, c_fp], c_i),
    "lfvdm_noise_prior_factor": ([c_fp, C.c_double, C.c_double, C.c_double, c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_noise_prior_fill": ([c_fp] * 5 + [c_i, c_i, C.c_int64, c_fp], c_i),
    "lfvdm_masked_mse_bwd": ([c_fp, c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_vb_terms": ([c_fp] * 12 + [c_i, c_i] + [c_fp] * 4 + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_vb_terms_bwd": ([c_fp] * 11 + [c_i, c_i, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_frame_metrics": ([c_fp, c_fp, c_i, C.c_float, C.c_float] + [c_i] * 5 + [c_fp, c_fp, c_fp, C.c_long, c_fp], c_i),
    "lfvdm_frame_metrics_workspace": ([c_i] * 5, C.c_long),
    "lfvdm_frame_dist_rows": ([c_fp] + [c_i] * 6 + [c_fp, c_i, c_fp, c_i, c_fp, c_fp], c_i),
    "lfvdm_fps_select": ([c_fp, c_i, c_i, c_fp, c_i, c_fp, c_i, c_i, c_fp, c_fp], c_i),
    "lfvdm_gn_bwd_stats": ([c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_fp, c_fp], c_i),
    "lfvdm_gn_bwd_apply": ([c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_fp, c_i, c_fp, c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_gn_bwd_apply_params": ([c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp, c_fp, c_fp, c_fp, c_i, c_fp, c_fp, c_i, c_i,
                                   c_fp, c_fp, c_fp, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_fp, c_i, c_fp], c_i),
    "lfvdm_gn_bwd_ws_floats": ([c_i, c_i, c_i], C.c_long),
    "lfvdm_gn_bwd": ([C.POINTER(GnBwdArgs), c_fp], c_i),
    "lfvdm_gn_param_grads": ([c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_rowdot_bwd": ([c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_gn_temporal_bwd": ([c_fp, c_fp, c_fp, C.c_float, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_gn_temporal": ([c_fp, c_fp, c_fp, C.c_float, c_fp, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_gn_temporal_qkv_ok": ([c_i, c_i, c_i, c_i], c_i),
    "lfvdm_proj_gn_ok": ([c_i, c_i, c_i], c_i),
    "lfvdm_proj_gn": ([c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_float, c_i, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_gn_temporal_qkv": ([c_fp, c_fp, c_fp, C.c_float, c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_rowdot": ([c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_silu": ([c_fp, c_fp, C.c_int64, c_fp], c_i),
    "lfvdm_rpe_nets": ([c_fp, c_i, c_i, c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_rpe_nets_maxc": ([c_fp, c_i, c_i, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_rpe_nets_bwd": ([c_fp, c_i, c_i, c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_conv_wgrad_grouped": ([c_fp, c_i, c_i, c_fp], c_i),
    "lfvdm_attn_spatial": ([c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_attn_spatial_fused_ok": ([c_i, c_i, c_i, c_i], c_i),
    "lfvdm_attn_spatial_fused": ([c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_det_reduce": ([c_fp, c_fp, C.c_long, C.c_long, c_fp], c_i),
    "lfvdm_gn_temporal_bwd_det": ([c_fp, c_fp, c_fp, C.c_float, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_fp, C.c_int64, c_fp], c_i),
    "lfvdm_rowdot_bwd_det": ([c_fp, c_i, c_i, c_fp, C.c_int64, c_fp, C.c_int64, c_fp], c_i),
    "lfvdm_rpe_nets_bwd_det": ([c_fp, c_i, c_i, c_fp, c_i, c_i, c_fp, C.c_int64, c_fp], c_i),
    "lfvdm_rpe_front": ([c_fp, c_i, c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_rpe_front_bwd": ([c_fp, c_i, c_fp, c_fp, c_fp, c_fp, c_fp, c_i, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_sampler_tick": ([c_fp, c_fp, c_fp, c_i, c_fp], c_i),
    "lfvdm_sampler_tick_fetch": ([c_fp, c_fp, c_fp, c_i, c_fp, c_i, c_fp, c_i, c_fp], c_i),
    "lfvdm_attn_temporal_sel": ([c_fp] * 7 + [c_i] * 5 + [c_fp, c_fp], c_i),
    "lfvdm_attn_temporal_ring": ([c_fp] * 7 + [c_i] * 5 + [c_fp, c_i, c_fp], c_i),
    "lfvdm_attn_temporal_bwd": ([c_fp] * 12 + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_attn_spatial_bwd": ([c_fp] * 6 + [c_i, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_attn_temporal": ([c_fp] * 7 + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_adamw_ema": ([C.POINTER(AdamWArgs), c_fp], c_i),
    "lfvdm_grad_norm_nparts": ([C.c_int64], c_i),
    "lfvdm_grad_norm_partials": ([c_fp, C.c_int64, C.c_float, c_fp, c_i, c_fp], c_i),
    "lfvdm_grad_norm_finalize": ([c_fp, c_i, C.c_float, c_fp, c_fp], c_i),
    "lfvdm_adamw_ema_clip": ([C.POINTER(AdamWArgs), c_fp, c_fp], c_i),
    "lfvdm_q_sample": ([c_fp] * 6 + [c_i, c_i, c_fp], c_i),
    "lfvdm_masked_mse": ([c_fp] * 4 + [c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_train_loss": ([c_fp] * 6 + [c_i] + [c_fp] * 3 + [c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_train_loss_bwd": ([c_fp] * 5 + [c_i, c_fp, c_fp, c_i, c_i, c_i, c_fp], c_i),
    "lfvdm_prepare_batch": ([c_fp] * 6 + [c_i] * 4 + [c_fp], c_i),
    "lfvdm_wavelet_encode": ([c_fp, c_i, C.c_float, C.c_float, c_fp, c_fp, c_fp] + [c_i] * 6 + [c_fp], c_i),
    "lfvdm_wavelet_decode": ([c_fp, c_fp, c_fp, c_fp] + [c_i] * 7 + [c_fp], c_i),
    "lfvdm_prepare_batch_wavelet": ([c_fp, c_i, C.c_float, C.c_float] + [c_fp] * 7 + [c_i] * 8 + [c_fp], c_i),
    "lfvdm_shapes_trajectories": ([c_fp, c_fp, c_fp, C.c_uint64] + [c_i] * 7 + [c_fp], c_i),
    "lfvdm_shapes_render": ([c_fp] * 5 + [c_i] + [c_fp] * 3 + [c_i] * 7 + [c_fp], c_i),
    "lfvdm_search_assemble": ([c_fp] * 9 + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_search_noise_qsample": ([c_fp] * 10 + [c_i] * 4 + [c_fp], c_i),
    "lfvdm_search_noise_fill": ([c_fp, C.c_uint64, c_i, c_i, c_fp] + [c_i] * 4 + [c_fp], c_i),
    "lfvdm_search_scores": ([c_fp, c_fp, c_fp] + [c_i] * 5 + [c_fp], c_i),
    "lfvdm_chain_plan": ([C.POINTER(ChainStage), c_i, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)], c_i),
    "lfvdm_chain_conv_ok": ([C.POINTER(ConvArgs)], c_i),
    "lfvdm_chain_gn_ok": ([c_i, c_i, c_i, c_i], c_i),
    "lfvdm_chain_local_ok": ([C.POINTER(ConvArgs), c_i], c_i),
    "lfvdm_chain_capacity": ([c_i], c_i),
    "lfvdm_level_chain": ([c_fp, c_i, c_fp, c_fp, c_fp, c_i, c_i, C.c_double, c_fp], c_i),
    "lfvdm_flag_add": ([c_fp, c_fp], c_i),
    "lfvdm_flag_wait": ([c_fp, c_i, C.c_double, c_fp, c_fp], c_i),
    "lfvdm_flag_wait2": ([c_fp, c_i, C.c_double, c_fp, c_fp, c_fp], c_i),
}

EXPORTS = tuple(_SIGS)

# Positional layouts (without the stream) of the spatial GroupNorm forward entries, by GnArgs field name where one exists.
# The one place that knows the order: gn_fwd_call builds calls and plan steps from it, _chains.chain_stage reads plan
# steps back by it, bench.py reads the same tuples by position.
GN_APPLY_ARGS = ("src0", "src1", "C0", "C1", "N", "P", "gamma", "beta", "film", "film_div", "film_ld", "eps", "act", "out",
                 "coefA", "coefB", "stats")                       # lfvdm_gn_apply; lfvdm_gn_apply_ws: + ("ws", "ws_floats")
GN_APPLY_PART_ARGS = ("src0", "C0", "N", "P", "cg", "gamma", "beta", "eps", "act", "out", "ldo")      # lfvdm_gn_apply_part


def gn_fwd_call(alloc_ws=None, **kw):
    """-> (entry, its arguments without the stream) for keywords named as in GN_APPLY_ARGS (raw pointers or None; src1,
    film and the three optional outputs default to absent).  No ``out``: lfvdm_gn_coef_stats, whose layout is the same
    without act / out.  Otherwise lfvdm_gn_apply, or on a large map lfvdm_gn_apply_ws with ``alloc_ws(floats)`` -> pointer."""
    L = lib()
    kw = dict(dict(src1=None, C1=0, film=None, film_div=1, film_ld=0, act=ACT_NONE, out=None, coefA=None, coefB=None,
                   stats=None), **kw)
    if kw["out"] is None:
        return L.lfvdm_gn_coef_stats, tuple(kw[k] for k in GN_APPLY_ARGS if k not in ("act", "out"))
    args = tuple(kw[k] for k in GN_APPLY_ARGS)
    need = int(L.lfvdm_gn_apply_ws_floats(kw["C0"] + kw["C1"], kw["N"], kw["P"]))
    return (L.lfvdm_gn_apply_ws, args + (alloc_ws(need), need)) if need else (L.lfvdm_gn_apply, args)


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"native library {LIB_PATH} is missing - build it with "
                "`python latent-flexible-video-diffusion-modeling_amd/build.py` (there is no fallback path)")
        L = C.CDLL(LIB_PATH)
        for name, (argt, rest) in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = rest
        _lib = L
    return _lib


_ERR = {1: "invalid shape", 2: "HIP launch error", 3: "unsupported configuration"}


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {_ERR.get(rc, rc)}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("native ops need device (HIP) tensors; the product has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    return t.data_ptr()


# ------------------------------------------------------------------------------ thin wrappers
def conv_igemm(**kw):
    """Fill an lfvdm_conv_args from keyword tensors/ints (see fill_conv_args) and launch.  Required: src0, C0, N, Hs,
    Ws, Ho, Wo, W, Cout, out.  Everything else defaults to 'absent'."""
    a = fill_conv_args(**kw)
    ws, cnt = splitk_workspace(kw["out"].device)
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = ws.data_ptr(), cnt.data_ptr(), ws.numel(), cnt.numel()
    a.tune = tuned_code(a)
    check(lib().lfvdm_conv_igemm(C.byref(a), stream()), "lfvdm_conv_igemm")


_splitk = {}


def splitk_workspace(device):
    """Per-device split-K workspace shared by all eager launches (they are stream-ordered): 8 MiB of slabs and
    zero-initialised, self-cleaning arrival tickets."""
    ent = _splitk.get(device)
    if ent is None:
        ent = _splitk[device] = (torch.empty(2 * 1024 * 1024, device=device, dtype=torch.float32),
                                 torch.zeros(4096, device=device, dtype=torch.int32))
    return ent


# ------------------------------------------------------------------------------------------- launch tuning
# Launch shape -> tile/K-chunk/split-K code (lfvdm_conv_args.tune), measured on the device the first time a
# shape is launched outside of stream capture.  LFVDM_TUNE_CACHE names a JSON table that is loaded READ-ONLY
# (entries are only valid for the library ABI version they were measured with; the committed
# profiles/tune_cache_mi355x.json is used this way by bench.py and the profiling tools, so ordinary runs never modify a
# tracked file).  Newly measured entries are written at exit only if LFVDM_TUNE_CACHE_OUT names a file (may equal
# LFVDM_TUNE_CACHE to refresh it in place - tools/refresh_profiles.sh does), and only by rank 0 of a multi-process job.
_tune = None
_tune_saved = 0


# markers appended to a launch-shape key (integers: the table is stored as JSON lists of ints): the fastest code among the
# variants the persistent level chain holds, measured per launch / measured inside its chain
TUNE_CHAIN, TUNE_IN_CHAIN, TUNE_LOCAL_RT = -101, -102, -103      # (-103: row tiles per item of a sample-local chain stage)


def tune_key(a):
    return (a.N, a.Hs, a.Ws, a.up, a.stride, a.ksize, a.Ho, a.Wo, a.C0, a.C1, a.Cout, a.s2C0, a.s2C1, bool(a.coefA), a.act,
            bool(a.res), bool(a.resA), a.out_mode, bool(a.splitk_ws),
            (1 + bool(a.gn_film) + 2 * bool(a.gn_skip_raw) + 4 * bool(a.gn_gw)) if a.gn_out else 0)


def tune_cache():
    global _tune, _tune_saved
    if _tune is None:
        _tune = {}
        for path in (os.environ.get("LFVDM_TUNE_CACHE", ""), os.environ.get("LFVDM_TUNE_CACHE_OUT", "")):
            if path and os.path.exists(path):
                try:
                    with open(path) as f:
                        blob = json.load(f)
                    if blob.get("abi") == int(lib().lfvdm_abi_version()):
                        _tune.update({tuple(json.loads(k)): int(v) for k, v in blob["entries"].items()})
                except (OSError, ValueError, KeyError):
                    pass
        _tune_saved = len(_tune)
        atexit.register(tune_cache_save)
    return _tune


def tune_cache_save():
    global _tune_saved
    path = os.environ.get("LFVDM_TUNE_CACHE_OUT", "")
    if not path or _tune is None or len(_tune) == _tune_saved or os.environ.get("RANK", "0") != "0":
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump({"abi": int(lib().lfvdm_abi_version()),
                       "entries": {json.dumps([int(x) for x in k]): int(v) for k, v in sorted(_tune.items())}}, f, indent=0)
        os.replace(tmp, path)
        _tune_saved = len(_tune)
    except OSError:
        pass


def autotune_launch(a, rounds=3, reps=6, chain_only=False):
    """Time every legal variant of this implicit-GEMM launch (the launch is idempotent) and return the fastest
    code.  Must not be called while the stream is capturing.  LFVDM_TUNE_REPS / LFVDM_TUNE_ROUNDS: longer measurements
    (what the committed table was made with: 20 x 5).  chain_only: only the variants the persistent level chain holds
    (lfvdm_chain_conv_ok: 4-wave tiles, 32-channel chunks, plain split-K); 0 if there is none."""
    rounds = int(os.environ.get("LFVDM_TUNE_ROUNDS", rounds))
    reps = int(os.environ.get("LFVDM_TUNE_REPS", reps))
    L, s = lib(), stream()
    codes = (C.c_int * 256)()
    n = L.lfvdm_conv_igemm_candidates(C.byref(a), codes, 256)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, best_t = 0, float("inf")
    for code in ([] if chain_only else [0]) + [codes[i] for i in range(n)]:
        a.tune = code
        if chain_only and L.lfvdm_chain_conv_ok(C.byref(a)) != 0:
            continue
        if L.lfvdm_conv_igemm(C.byref(a), s) != 0:
            continue
        t_min = float("inf")
        for _ in range(rounds):
            ev0.record()
            for _ in range(reps):
                L.lfvdm_conv_igemm(C.byref(a), s)
            ev1.record()
            ev1.synchronize()
            t_min = min(t_min, ev0.elapsed_time(ev1))
        if t_min < best_t * 0.98:      # prefer earlier (simpler) candidates on ties
            best, best_t = code, t_min
    a.tune = best
    return best


def tuned_code(a):
    """Cached code for this launch shape; measures it on first sight unless LFVDM_AUTOTUNE=0 or capturing."""
    cache = tune_cache()
    key = tune_key(a)
    code = cache.get(key)
    if code is None:
        if os.environ.get("LFVDM_AUTOTUNE", "1") == "0" or torch.cuda.is_current_stream_capturing():
            return 0
        code = cache[key] = autotune_launch(a)
    return code


def fill_conv_args(**kw):
    """ConvArgs from keyword tensors/ints (same keys as conv_igemm)."""
    a = ConvArgs()
    g = kw.get
    a.src0 = ptr(kw["src0"]); a.src1 = ptr(g("src1")); a.C0 = kw["C0"]; a.C1 = g("C1", 0)
    a.N = kw["N"]; a.Hs = kw["Hs"]; a.Ws = kw["Ws"]; a.up = g("up", 0); a.stride = g("stride", 1)
    a.ksize = g("ksize", 3); a.Ho = kw["Ho"]; a.Wo = kw["Wo"]
    a.coefA = ptr(g("coefA")); a.coefB = ptr(g("coefB")); a.act = g("act", ACT_NONE)
    a.W = ptr(g("W")); a.bias = ptr(g("bias")); a.Cout = kw["Cout"]
    a.s2src0 = ptr(g("s2src0")); a.s2src1 = ptr(g("s2src1")); a.s2C0 = g("s2C0", 0); a.s2C1 = g("s2C1", 0)
    a.W2 = ptr(g("W2")); a.bias2 = ptr(g("bias2"))
    a.res = ptr(g("res")); a.ldr = g("ldr", kw["Cout"]); a.resA = ptr(g("resA")); a.resB = ptr(g("resB"))
    a.out = ptr(kw["out"]); a.ldo = g("ldo", kw["Cout"]); a.out_mode = g("out_mode", OUT_ROWS)
    if g("gn_out") is not None:     # fused GroupNorm(+FiLM)(+activation) of the output (see lfvdm_conv_args)
        film = g("gn_film")
        a.gn_gamma = ptr(kw["gn_gamma"]); a.gn_beta = ptr(kw["gn_beta"]); a.gn_out = ptr(kw["gn_out"])
        a.gn_film = film.data_ptr() if film is not None else None
        a.gn_film_ld = film.stride(0) if film is not None else 0
        a.gn_film_div = g("gn_film_div", 1); a.gn_act = g("gn_act", ACT_NONE); a.gn_skip_raw = int(g("gn_skip_raw", 0))
        a.gn_eps = g("gn_eps", 1e-5)
    return a


# ------------------------------------------------------------------------------------------- deterministic gradients
def deterministic():
    """LFVDM_DETERMINISTIC=1: partial gradient sums go through ordered slabs instead of float atomics (include/lfvdm_hip.h,
    "Deterministic gradients"): bitwise reproducible training steps, at the price of the slab traffic."""
    return os.environ.get("LFVDM_DETERMINISTIC", "0") == "1"


_det_ws = {}


def det_workspace(device):
    """The per-device slab workspace of the deterministic mode (LFVDM_DET_WS_MB, default 1024 MiB; launches are stream-ordered,
    one workspace serves all of them).  Allocated on first use, outside of stream capture."""
    ws = _det_ws.get(device)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("deterministic workspace missing under stream capture: run the step eagerly once first")
        ws = _det_ws[device] = torch.empty(int(os.environ.get("LFVDM_DET_WS_MB", "1024")) * 2 ** 18, device=device, dtype=torch.float32)
    return ws


def _wgrad_codes(a):
    """Candidate launch codes of lfvdm_conv_wgrad for this layer shape (1 + tile + 4 * stages + 16 * M slices; tile 1 / 2 / 3 =
    64 x 64 / 128 x 64 / 128 x 128 filters x channels, stages 1 / 2 / 3 = two / three stages / two stages of 64-row chunks)."""
    Cin, M = a.C0 + a.C1, a.N * a.Ho * a.Wo
    if Cin % 64 or a.C0 % 64 or a.Cout < 64 or a.coefA:
        return []
    nchunks = (M + 31) // 32
    codes = []
    for tile, cot in ((1, 2), (2, 4), (3, 4)):
        if cot == 4 and a.Cout < 128:
            continue
        kt = 4 if tile == 3 else 2
        if tile == 3 and (Cin % 128 or a.C0 % 128):
            continue
        tiles = a.ksize * a.ksize * (Cin // (32 * kt)) * ((a.Cout + 32 * cot - 1) // (32 * cot))
        for stages in (2, 1, 3):          # 3 LDS-DMA stages, 2 stages, 2 stages of 64-row chunks
            for target in (256, 320, 384, 448, 512, 640, 768, 1024):
                ms = max(1, min((target + tiles - 1) // tiles, (nchunks // 2 if stages == 3 else nchunks) // 2))
                code = 1 + tile + 4 * stages + 16 * ms
                if code not in codes:
                    codes.append(code)
    # tap-fused kernels (stage field 0): tile 1 = one filter row (three taps) per workgroup, tile 2 = all nine taps
    HW = a.Ho * a.Wo
    if (a.ksize == 3 and a.stride == 1 and a.up == 0 and HW % 32 == 0 and (a.Wo % 32 == 0 or a.Wo in (8, 16))
            and a.Hs == a.Ho and a.Ws == a.Wo and a.out_mode == 0):        # (packed accumulator layout only: no OIHW store)
        for tile, rows in ((1, 3), (2, 1)):
            tiles = rows * (Cin // 64) * ((a.Cout + 63) // 64)
            for target in (128, 192, 256, 320, 384, 512):
                ms = max(1, min((target + tiles - 1) // tiles, (M // 32) // 2))
                code = 1 + tile + 16 * ms
                if code not in codes:
                    codes.append(code)
    return codes


def _capturing():
    """Is the current stream being captured?  (False on a host without a device: the rank-agreement logic also runs in the
    CPU tests of the exchange)"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _tuned_wgrad_code(a, out_floats):
    """Cached launch code of this weight-gradient shape; measured on first sight (outside stream capture) on SCRATCH
    outputs - the real launch accumulates.  The weight-gradient kernels are a quarter of a training step and how their
    (filter tile, channel tile, M slice) workgroups divide the 256 CUs differs per layer."""
    cache = tune_cache()
    key = _wgrad_key(a)
    store = _rank_store()
    skey = "lfvdm/wgrad/" + json.dumps([int(x) for x in key])

    def publish(code):
        # rank 0, every resolution once a store exists - also the ones made BEFORE the process group existed (the first
        # call found no store) and the heuristic 0 taken under stream capture: a peer blocked on a key that is never set
        # would sit in the backward pass until the store's timeout
        if store is not None and store[1] == 0 and key not in _wgrad_published:
            store[0].set(skey, str(int(code)))
            _wgrad_published.add(key)

    code = _wgrad_agreed.get(key)
    if code is not None:
        publish(code)
        return code
    if store is not None and store[1] != 0:
        # data-parallel job: ranks must run the SAME kernels (bitwise-equal replicas in deterministic mode, no skew from
        # one rank tuning while its peers sit in a bucket all-reduce): rank 0 decides, the others read its choice from
        # the rendezvous store (once per shape and process; no collective that could mismatch).  Bounded: if rank 0 does
        # not publish within LFVDM_WGRAD_AGREE_S seconds the cached / heuristic code is used and said on stderr
        if _capturing():
            return cache.get(key, 0)
        import datetime
        try:
            store[0].wait([skey], datetime.timedelta(seconds=float(os.environ.get("LFVDM_WGRAD_AGREE_S", "60"))))
            code = int(store[0].get(skey).decode())
        except Exception:
            code = cache.get(key, 0)
            import sys
            print(f"[lfvdm] rank {store[1]}: no weight-gradient launch code from rank 0 for {skey}; using {code}", file=sys.stderr,
                  flush=True)
        _wgrad_agreed[key] = code
        return code
    code = cache.get(key)
    if code is None:
        if _capturing() or os.environ.get("LFVDM_AUTOTUNE", "1") == "0" or deterministic():
            code = 0                    # the heuristic (nothing may be measured inside a capture): kept for the process and
                                        # published below, so that every rank runs it and nobody waits
        else:
            code = _measure_wgrad_code(a, out_floats)
            cache[key] = code
    _wgrad_agreed[key] = code
    publish(code)
    return code


_wgrad_agreed = {}
_wgrad_published = set()
_store_memo = []


def _wgrad_key(a):
    # the bias reduction and a strided dout (ldr != Cout: the head's padded rows) change the kernel's work: own entries
    return (-1,) + tune_key(a) + (int(bool(a.bias)), int(a.ldr != a.Cout and a.ldr != 0))


def _rank_store():
    """(c10d store, rank) of an initialised multi-rank job, else None."""
    if not _store_memo:
        import torch.distributed as dist
        st = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            try:
                st = (dist.distributed_c10d._get_default_store(), dist.get_rank())
            except Exception:
                st = None
        if not (dist.is_available() and dist.is_initialized()):
            return None                 # not memoised: the process group may still be created later
        _store_memo.append(st)
    return _store_memo[0]


def _measure_wgrad_code(a, out_floats):
    codes = _wgrad_codes(a)
    if not codes:
        return 0
    L, s = lib(), stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    scratch, sb = torch.zeros(out_floats, device=dev), torch.zeros(max(a.Cout, 1), device=dev)
    real_out, real_bias = a.out, a.bias
    a.out = scratch.data_ptr()
    if real_bias:
        a.bias = sb.data_ptr()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, best_t = 0, float("inf")
    for code in [0] + codes:
        a.tune = code
        if L.lfvdm_conv_wgrad(C.byref(a), s) != 0:
            continue
        t_min = float("inf")
        for _ in range(int(os.environ.get("LFVDM_TUNE_ROUNDS", 3))):
            ev0.record()
            for _ in range(int(os.environ.get("LFVDM_TUNE_REPS", 4))):
                L.lfvdm_conv_wgrad(C.byref(a), s)
            ev1.record()
            ev1.synchronize()
            t_min = min(t_min, ev0.elapsed_time(ev1))
        if t_min < best_t * 0.98:
            best, best_t = code, t_min
    a.out, a.bias, a.tune = real_out, real_bias, 0
    return best


def conv_wgrad(**kw):
    """Weight/bias gradient launch; kw as conv_igemm plus res=dout rows, out=packed dW, bias=db."""
    a = fill_conv_args(**kw)
    if deterministic():
        # tile shape / M slices: the table entry measured in the default (atomics) mode, if there is one - nothing is timed in
        # this mode (same table on every rank: same kernels, bitwise-equal replicas); key without the slab pointer
        key = _wgrad_key(a)
        ws = det_workspace(kw["out"].device)
        a.splitk_ws, a.splitk_ws_floats = ws.data_ptr(), ws.numel()
        a.tune = tune_cache().get(key, 0)
    else:
        a.tune = _tuned_wgrad_code(a, kw["out"].numel())
    check(lib().lfvdm_conv_wgrad(C.byref(a), stream()), "lfvdm_conv_wgrad")


def pack_conv_weight_t(w, out):
    Cout, Cin, k = w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)
    check(lib().lfvdm_pack_conv_weight_t(ptr(w), ptr(out), Cout, Cin, k, stream()), "lfvdm_pack_conv_weight_t")


def unpack_conv_grad(gp, g, accumulate):
    Cout, Cin, k = g.shape[0], g.shape[1], (g.shape[2] if g.dim() == 4 else 1)
    check(lib().lfvdm_unpack_conv_grad(ptr(gp), ptr(g), Cout, Cin, k, int(bool(accumulate)), stream()), "lfvdm_unpack_conv_grad")


def conv_igemm_struct(a):
    check(lib().lfvdm_conv_igemm(C.byref(a), stream()), "lfvdm_conv_igemm")


def pack_conv_weight(w, out):
    Cout, Cin, k, _ = w.shape
    check(lib().lfvdm_pack_conv_weight(ptr(w), ptr(out), Cout, Cin, k, stream()), "lfvdm_pack_conv_weight")


def pack_conv_weight_up2x(w, out):
    """OIHW 3x3 weight -> [4 classes][Cout][4 taps][Cin], the pre-summed pack of a nearest-2x conv run with up = 3."""
    Cout, Cin, k, _ = w.shape
    if k != 3 or out.numel() != 16 * Cout * Cin:
        raise RuntimeError("lfvdm_pack_conv_weight_up2x needs a 3x3 weight and a [4][Cout][4][Cin] output")
    check(lib().lfvdm_pack_conv_weight_up2x(ptr(w), ptr(out), Cout, Cin, stream()), "lfvdm_pack_conv_weight_up2x")


def conv_in(x, x0, obs, w, bias, out, N, Cc, H, W, Cout):
    check(lib().lfvdm_conv_in(ptr(x), ptr(x0), ptr(obs), ptr(w), ptr(bias), ptr(out), N, Cc, H, W, Cout, stream()),
          "lfvdm_conv_in")


def gn_coef(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, coefA, coefB):
    check(lib().lfvdm_gn_coef(ptr(src0), ptr(src1), C0, C1, N, P, ptr(gamma), ptr(beta), ptr(film), film_div, film_ld,
                              eps, ptr(coefA), ptr(coefB), stream()), "lfvdm_gn_coef")


def gn_temporal(x, gamma, beta, eps, y, B, T, P, Cc):
    check(lib().lfvdm_gn_temporal(ptr(x), ptr(gamma), ptr(beta), eps, ptr(y), B, T, P, Cc, stream()), "lfvdm_gn_temporal")


def rowdot(jobs_dev, njobs, total_rows):
    check(lib().lfvdm_rowdot(ptr(jobs_dev, torch.uint8), njobs, total_rows, stream()), "lfvdm_rowdot")


def rpe_nets(jobs_dev, njobs, total_tiles, frame_indices, B, T):
    check(lib().lfvdm_rpe_nets(ptr(jobs_dev, torch.uint8), njobs, total_tiles, ptr(frame_indices, torch.int64), B, T,
                               stream()), "lfvdm_rpe_nets")


def attn_spatial(qkv, o, attn_out, N, P, Cc, heads, lse=None):
    check(lib().lfvdm_attn_spatial(ptr(qkv), ptr(o), ptr(attn_out), ptr(lse), N, P, Cc, heads, stream()),
          "lfvdm_attn_spatial")


def attn_spatial_bwd(qkv, o, d_o, lse, delta_ws, dqkv, N, P, Cc, heads):
    check(lib().lfvdm_attn_spatial_bwd(ptr(qkv), ptr(o), ptr(d_o), ptr(lse), ptr(delta_ws), ptr(dqkv), N, P, Cc, heads,
                                       stream()), "lfvdm_attn_spatial_bwd")


def attn_temporal(qkv, Rq, Rk, Rv, mask, o, attn_out, B, T, P, Cc, heads):
    check(lib().lfvdm_attn_temporal(ptr(qkv), ptr(Rq), ptr(Rk), ptr(Rv), ptr(mask), ptr(o), ptr(attn_out), B, T, P, Cc,
                                    heads, stream()), "lfvdm_attn_temporal")


def attn_temporal_bwd(qkv, d_o, Rq, Rk, Rv, mask, ws_p, ws_ds, dqkv, dRq, dRk, dRv, B, T, P, Cc, heads):
    check(lib().lfvdm_attn_temporal_bwd(ptr(qkv), ptr(d_o), ptr(Rq), ptr(Rk), ptr(Rv), ptr(mask), ptr(ws_p), ptr(ws_ds),
                                        ptr(dqkv), ptr(dRq), ptr(dRk), ptr(dRv), B, T, P, Cc, heads, stream()),
          "lfvdm_attn_temporal_bwd")


def q_sample(x0, noise, t, sa, sb, out):
    B = x0.shape[0]
    check(lib().lfvdm_q_sample(ptr(x0), ptr(noise), ptr(t, torch.int64), ptr(sa), ptr(sb), ptr(out), B,
                               x0.numel() // B, stream()), "lfvdm_q_sample")


RULE_ANCESTRAL, RULE_DDIM = 0, 1      # LFVDM_RULE_* / LFVDM_MEAN_* of include/lfvdm_hip.h
MEAN_EPS, MEAN_X0 = 0, 1
# not a value of the library's ``rule`` argument: the multistep rule has entries of its own (lfvdm_update_ms_x0,
# lfvdm_conv_out_update_ms_x0).  _engine.update_args hands it out so that the callers can tell which entry to launch
RULE_DPMPP2M = "dpmpp2m"


def update_x0(x, out, noise, t, recip, recipm1, c1, c2, sg, rule, mean_type, clip, sample, pred=None, mean=None):
    """The x_{t-1} update with given noise (lfvdm_update_x0).  ``out``: the network's output; MEAN_X0: ``recip`` /
    ``recipm1`` may be None; RULE_DDIM with ``sg=None``: deterministic, ``noise`` is not read."""
    B = x.shape[0]
    check(lib().lfvdm_update_x0(ptr(x), ptr(out), ptr(noise), ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(c1), ptr(c2),
                                ptr(sg), int(rule), int(mean_type), int(bool(clip)), ptr(sample), ptr(pred), ptr(mean), B,
                                x.numel() // B, stream()), "lfvdm_update_x0")


def update_rng_x0(x, out, noise_out, t, recip, recipm1, c1, c2, sg, rule, mean_type, clip, sample, seed, pred=None, mean=None):
    """The same update with the noise drawn in the kernel (lfvdm_update_rng_x0): Philox keyed by the device int64 ``seed``;
    ``noise_out`` (optional) receives the values used."""
    B = x.shape[0]
    check(lib().lfvdm_update_rng_x0(ptr(x), ptr(out), ptr(noise_out), ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(c1),
                                    ptr(c2), ptr(sg), int(rule), int(mean_type), int(bool(clip)), ptr(sample), ptr(pred),
                                    ptr(mean), B, x.numel() // B, ptr(seed, torch.int64) if seed is not None else None, stream()),
          "lfvdm_update_rng_x0")


def conv_out_update_x0(act, wp, bias, out, x, noise_in, noise_out, t, recip, recipm1, c1, c2, sg, rule, mean_type, clip, sample,
                       seed, pred=None, mean=None):
    """The U-Net's output conv and the update in one launch (lfvdm_conv_out_update_x0).  act: channels-last rows
    [B*T*H*W][C]; wp: packed filters [Cout][9][C]; x / sample / out: (B, T, Cout, H, W); ``noise_in=None``: the noise is
    update_rng_x0's for the same seed."""
    B, T, Cout, H, W = x.shape
    check(lib().lfvdm_conv_out_update_x0(ptr(act), ptr(wp), ptr(bias), ptr(out), ptr(x), ptr(noise_in), ptr(noise_out),
                                         ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(c1), ptr(c2), ptr(sg), int(rule),
                                         int(mean_type), int(bool(clip)), ptr(sample), ptr(pred), ptr(mean), B, T, H, W,
                                         act.shape[-1], Cout, ptr(seed, torch.int64) if seed is not None else None, stream()),
          "lfvdm_conv_out_update_x0")


def update_ms_x0(x, out, hist, t, recip, recipm1, k1, k2, k3, mean_type, clip, sample, pred=None):
    """The DPM-Solver++(2M) update (lfvdm_update_ms_x0): the deterministic DDIM step of ``k1`` / ``k2`` plus
    ``k3[t] (x0-hat - hist)`` where ``k3[t] != 0``.  ``hist``: the x0-hat of the step before - it may BE ``pred`` - or None
    for a first-order step in every row."""
    B = x.shape[0]
    check(lib().lfvdm_update_ms_x0(ptr(x), ptr(out), ptr(hist), ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(k1), ptr(k2),
                                   ptr(k3), int(mean_type), int(bool(clip)), ptr(sample), ptr(pred), B, x.numel() // B, stream()),
          "lfvdm_update_ms_x0")


def conv_out_update_ms_x0(act, wp, bias, out, x, hist, t, recip, recipm1, k1, k2, k3, mean_type, clip, sample, pred=None):
    """The U-Net's output conv and the DPM-Solver++(2M) update in one launch (lfvdm_conv_out_update_ms_x0); act / wp / x /
    sample / out as for ``conv_out_update_x0``, ``hist`` as for ``update_ms_x0``."""
    B, T, Cout, H, W = x.shape
    check(lib().lfvdm_conv_out_update_ms_x0(ptr(act), ptr(wp), ptr(bias), ptr(out), ptr(x), ptr(hist), ptr(t, torch.int64),
                                            ptr(recip), ptr(recipm1), ptr(k1), ptr(k2), ptr(k3), int(mean_type), int(bool(clip)),
                                            ptr(sample), ptr(pred), B, T, H, W, act.shape[-1], Cout, stream()),
          "lfvdm_conv_out_update_ms_x0")


def known_blend(x, known, mask, t, a, s, eps=None, seed=None, noise_out=None):
    """The known-region blend in place over ``x`` (B, T, C, H, W) (lfvdm_known_blend): ``mask`` (B, T, H, W) in [0, 1],
    ``t`` the timestep the step just consumed, ``a`` / ``s`` the tables of ``GaussianDiffusion.known_region_tables``.
    ``eps`` given: fixed noise; else fresh noise keyed by the device int64 ``seed``, stored to ``noise_out`` if given."""
    B, T, Cx, H, W = x.shape
    if known.shape != x.shape or tuple(mask.shape) != (B, T, H, W) or (eps is not None and eps.shape != x.shape):
        raise RuntimeError("known_blend: known / eps are shaped like x (B, T, C, H, W) and mask is (B, T, H, W)")
    check(lib().lfvdm_known_blend(ptr(x), ptr(known), ptr(mask), ptr(eps), ptr(noise_out), ptr(t, torch.int64), ptr(a), ptr(s),
                                  ptr(seed, torch.int64) if seed is not None else None, B, T, Cx, H * W, stream()),
          "lfvdm_known_blend")


def renoise(x, t, c, d, seed, noise_out=None):
    """One forward diffusion step in place (lfvdm_renoise): x = c[t] x + d[t] eps with fresh noise keyed by ``seed``."""
    B = x.shape[0]
    check(lib().lfvdm_renoise(ptr(x), ptr(noise_out), ptr(t, torch.int64), ptr(c), ptr(d), ptr(seed, torch.int64), B,
                              x.numel() // B, stream()), "lfvdm_renoise")


def dyn_threshold_workspace(B, inner):
    """Bytes of workspace ``dyn_threshold`` needs for B rows of ``inner`` elements (lfvdm_dyn_threshold_workspace).  The
    caller zero-fills it once; every call hands it back ready for the next."""
    n = C.c_size_t(0)
    check(lib().lfvdm_dyn_threshold_workspace(int(B), int(inner), C.byref(n)), "lfvdm_dyn_threshold_workspace")
    return int(n.value)


def dyn_threshold(x, out, t, recip, recipm1, mean_type, x0hat_fma, frame_mask, percentile, max_value, xhat, stats, workspace):
    """Dynamic thresholding of x0-hat (lfvdm_dyn_threshold): x / out / xhat (B, T, ...), ``frame_mask`` (B, T) or None,
    ``stats`` (B, 3) receives (v_lo, v_hi, s), ``max_value`` None: no cap.  ``x0hat_fma``: the rounding of an epsilon model's
    x0-hat - that of the deterministic DDIM / multistep update (True) or of the ancestral / stochastic DDIM one (False).
    ``xhat`` is then the ``out`` of an update entry under MEAN_X0 with clip off."""
    B, T = x.shape[0], x.shape[1]
    if out.shape != x.shape or xhat.shape != x.shape or stats.numel() != 3 * B or (
            frame_mask is not None and frame_mask.numel() != B * T):
        raise RuntimeError("dyn_threshold: out / xhat are shaped like x (B, T, ...), frame_mask is (B, T), stats is (B, 3)")
    check(lib().lfvdm_dyn_threshold(ptr(x), ptr(out), ptr(t, torch.int64), ptr(recip), ptr(recipm1), int(mean_type),
                                    int(bool(x0hat_fma)), ptr(frame_mask), B, T, x.numel() // (B * T), float(percentile),
                                    float("inf") if max_value is None else float(max_value), ptr(xhat), ptr(stats),
                                    ptr(workspace, torch.uint8), stream()), "lfvdm_dyn_threshold")


def cfg_workspace(B, inner):
    """Bytes of workspace ``cfg_combine`` needs with rescale > 0 for B rows of ``inner`` elements (lfvdm_cfg_workspace).  It
    is never zero-filled: a call writes every word it reads."""
    n = C.c_size_t(0)
    check(lib().lfvdm_cfg_workspace(int(B), int(inner), C.byref(n)), "lfvdm_cfg_workspace")
    return int(n.value)


def cfg_combine(x, out2, t, recip, recipm1, mean_type, x0hat_fma, frame_mask, scale, rescale, xhat, stats, workspace=None):
    """Classifier-free guidance (lfvdm_cfg_combine): x / xhat (B, T, ...), ``out2`` (2B, T, ...) - rows [0, B) the conditional
    network output, rows [B, 2B) the one with obs_mask = 0 -, ``frame_mask`` (B, T) or None, ``stats`` (B, 3) receives
    (s_c, s_g, f).  ``x0hat_fma`` as in ``dyn_threshold``.  ``workspace`` (``cfg_workspace`` bytes) is needed with rescale > 0
    only.  ``xhat`` is then the ``out`` of ``dyn_threshold`` or of an update entry under MEAN_X0."""
    B, T = x.shape[0], x.shape[1]
    if out2.shape[0] != 2 * B or out2.shape[1:] != x.shape[1:] or xhat.shape != x.shape or stats.numel() != 3 * B or (
            frame_mask is not None and frame_mask.numel() != B * T):
        raise RuntimeError("cfg_combine: out2 is (2B, T, ...) for x (B, T, ...), xhat is shaped like x, frame_mask is (B, T), "
                           "stats is (B, 3)")
    check(lib().lfvdm_cfg_combine(ptr(x), ptr(out2), ptr(t, torch.int64), ptr(recip), ptr(recipm1), int(mean_type),
                                  int(bool(x0hat_fma)), ptr(frame_mask), float(scale), float(rescale), ptr(xhat), ptr(stats),
                                  ptr(workspace, torch.uint8), B, T, x.numel() // (B * T), stream()), "lfvdm_cfg_combine")


def noise_prior_factor(frame_indices, a, c, rho, out=None):
    """The lower Cholesky factor of the noise prior's covariance per sample (lfvdm_noise_prior_factor): ``frame_indices``
    (B, T) int64 -> L (B, T, T) fp32, the strict upper triangle 0.  ``out``: a static buffer to write instead."""
    B, T = frame_indices.shape
    L = torch.empty(B, T, T, device=frame_indices.device) if out is None else out
    if L.numel() != B * T * T:
        raise RuntimeError("noise_prior_factor: L is (B, T, T)")
    check(lib().lfvdm_noise_prior_factor(ptr(frame_indices, torch.int64), float(a), float(c), float(rho), ptr(L), B, T, stream()),
          "lfvdm_noise_prior_factor")
    return L


def noise_prior_fill(L, out, xi=None, seed=None, t=None):
    """out (B, T, ...) <- L xi along the frame axis (lfvdm_noise_prior_fill).  ``xi`` given (it may be ``out``): mix mode.
    ``xi`` None: xi is drawn in the kernel under ``seed`` (one int64) at the rows' timesteps ``t`` (B,), Philox stream 4."""
    B, T = out.shape[0], out.shape[1]
    if L.numel() != B * T * T or (xi is not None and xi.shape != out.shape):
        raise RuntimeError("noise_prior_fill: L is (B, T, T), xi is shaped like out (B, T, ...)")
    if xi is None and (seed is None or t is None or t.numel() != B):
        raise RuntimeError("noise_prior_fill: draw mode needs seed and t (B,)")
    check(lib().lfvdm_noise_prior_fill(ptr(L), ptr(xi), ptr(seed, torch.int64), ptr(t, torch.int64), ptr(out), B, T,
                                       out.numel() // (B * T), stream()), "lfvdm_noise_prior_fill")


def vb_terms(x_start, x_t, out, noise, t, recip, recipm1, c1, c2, post_logvar, model_logvar, mask, mean_type, clip, vb,
             xstart_mse=None, eps_mse=None, pred=None, col_base=-1):
    """One variational-bound term per batch row in bits per dimension (lfvdm_vb_terms).  ``out``: the network's output;
    ``vb`` (and the optional ``xstart_mse`` / ``eps_mse``) are (B,) or (B, n) tensors - with ``col_base`` >= 0 row b is
    written at column ``col_base - t[b]``; MEAN_X0 without ``eps_mse``: ``recip`` / ``recipm1`` may be None."""
    B, T = x_t.shape[0], x_t.shape[1]
    ld = vb.shape[1] if vb.dim() == 2 else 1
    check(lib().lfvdm_vb_terms(ptr(x_start), ptr(x_t), ptr(out), ptr(noise), ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(c1),
                               ptr(c2), ptr(post_logvar), ptr(model_logvar), ptr(mask), int(mean_type), int(bool(clip)), ptr(vb),
                               ptr(xstart_mse), ptr(eps_mse), ptr(pred), B, T, x_t.numel() // (B * T), ld, int(col_base),
                               stream()), "lfvdm_vb_terms")


def vb_terms_bwd(x_start, x_t, out, t, recip, recipm1, c1, c2, model_logvar, mask, g, mean_type, clip, d_out):
    """d_out = g[b] * d vb[b] / d out, clip_denoised=False only (lfvdm_vb_terms_bwd)."""
    B, T = x_t.shape[0], x_t.shape[1]
    check(lib().lfvdm_vb_terms_bwd(ptr(x_start), ptr(x_t), ptr(out), ptr(t, torch.int64), ptr(recip), ptr(recipm1), ptr(c1), ptr(c2),
                                   ptr(model_logvar), ptr(mask), ptr(g), int(mean_type), int(bool(clip)), ptr(d_out), B, T,
                                   x_t.numel() // (B * T), stream()), "lfvdm_vb_terms_bwd")


PIX_F32, PIX_U8 = 0, 1
_PIX = {torch.float32: PIX_F32, torch.uint8: PIX_U8}


def frame_metrics_workspace(K, N, C, H, W):
    """Floats of scratch ``frame_metrics`` needs for this shape (lfvdm_frame_metrics_workspace); 0: the shape is refused."""
    return int(lib().lfvdm_frame_metrics_workspace(K, N, C, H, W))


def frame_metrics(pred, truth, scale, shift, K, N, C, H, W, mse, ssim, partials):
    """Per-frame MSE and mean SSIM of ``pred`` (K, N, C, H, W) against ``truth`` (N, C, H, W), float32 or uint8, value =
    scale * raw + shift in [0, 1]; ``mse`` / ``ssim``: (K, N) float32 (lfvdm_frame_metrics)."""
    dt = pred.dtype
    if dt not in _PIX or truth.dtype != dt:
        raise RuntimeError(f"expected float32 or uint8 pixels of one dtype, got {pred.dtype} and {truth.dtype}")
    if pred.numel() != K * N * C * H * W or truth.numel() != N * C * H * W or mse.numel() != K * N or ssim.numel() != K * N:
        raise RuntimeError("frame_metrics: tensor sizes do not match (K, N, C, H, W)")
    check(lib().lfvdm_frame_metrics(ptr(pred, dt), ptr(truth, dt), _PIX[dt], float(scale), float(shift), K, N, C, H, W, ptr(mse),
                                    ptr(ssim), ptr(partials), partials.numel(), stream()), "lfvdm_frame_metrics")


def frame_dist_rows(x, B, T, C, H, W, levels, new_idx, cand_idx, dist):
    """dist (B, T, T) float32 <- the ``levels``-level distance of every frame in ``new_idx`` to every frame in ``new_idx`` and
    ``cand_idx`` (device int32 lists; ``cand_idx`` None or empty: none), rows and columns, of ``x`` (B, T, C, H, W) float32
    (lfvdm_frame_dist_rows)."""
    if x.numel() != B * T * C * H * W or dist.numel() != B * T * T:
        raise RuntimeError("frame_dist_rows: tensor sizes do not match (B, T, C, H, W)")
    n_cand = 0 if cand_idx is None else cand_idx.numel()
    check(lib().lfvdm_frame_dist_rows(ptr(x), B, T, C, H, W, int(levels), ptr(new_idx, torch.int32), new_idx.numel(),
                                      ptr(cand_idx, torch.int32) if n_cand else None, n_cand, ptr(dist), stream()),
          "lfvdm_frame_dist_rows")


def fps_select(dist, B, T, cand_idx, forced_pos, n, picks):
    """picks (B, n) int32 <- greedy farthest-point positions into ``cand_idx`` (device int32) on ``dist`` (B, T, T), starting
    from the positions ``forced_pos`` (device int32, at least one) (lfvdm_fps_select)."""
    if dist.numel() != B * T * T or picks.numel() != B * n:
        raise RuntimeError("fps_select: tensor sizes do not match (B, T, n)")
    check(lib().lfvdm_fps_select(ptr(dist), B, T, ptr(cand_idx, torch.int32), cand_idx.numel(), ptr(forced_pos, torch.int32),
                                 forced_pos.numel(), int(n), ptr(picks, torch.int32), stream()), "lfvdm_fps_select")


def prepare_batch(pool, table, batch, frame_indices, obs_mask, latent_mask):
    """pool (B, Tp, ...) fp32, table (B, F, 4) int32 -> batch (B, F, ...), frame_indices (B, F) int64, masks (B, F, 1, 1, 1)."""
    B, Tp = pool.shape[:2]
    F = table.shape[1]
    check(lib().lfvdm_prepare_batch(ptr(pool), ptr(table, torch.int32), ptr(batch), ptr(frame_indices, torch.int64), ptr(obs_mask),
                                    ptr(latent_mask), B, F, Tp, pool[0, 0].numel(), stream()), "lfvdm_prepare_batch")


WAVELET_NORMS = {"range": 0, "orthonormal": 1}
_U8_SCALE, _U8_SHIFT = 1.0 / 127.5, -1.0      # uint8 0..255 -> [-1, 1]


def _pix_affine(dt):
    if dt not in _PIX:
        raise RuntimeError(f"expected float32 or uint8 pixels, got {dt}")
    return (_U8_SCALE, _U8_SHIFT) if dt == torch.uint8 else (1.0, 0.0)


def wavelet_encode(pix, coef, levels, norm, mean=None, rstd=None):
    """pix (N, C, H, W) float32 in [-1, 1] or uint8 -> coef (N, 4^L C, H / 2^L, W / 2^L) float32 (lfvdm_wavelet_encode)."""
    N, Cc, H, W = pix.shape
    if coef.numel() != pix.numel():
        raise RuntimeError("wavelet_encode: coef does not hold as many elements as pix")
    scale, shift = _pix_affine(pix.dtype)
    check(lib().lfvdm_wavelet_encode(ptr(pix, pix.dtype), _PIX[pix.dtype], scale, shift, ptr(coef), ptr(mean), ptr(rstd), N, Cc, H,
                                     W, int(levels), WAVELET_NORMS[norm], stream()), "lfvdm_wavelet_encode")


def wavelet_decode(coef, pix, levels, norm, mean=None, std=None):
    """coef (N, 4^L C, H / 2^L, W / 2^L) float32 -> pix (N, C, H, W) float32, or uint8 ROUNDED to nearest
    (lfvdm_wavelet_decode)."""
    N, Cc, H, W = pix.shape
    if coef.numel() != pix.numel() or pix.dtype not in _PIX:
        raise RuntimeError("wavelet_decode: pix must be float32 or uint8 with as many elements as coef")
    check(lib().lfvdm_wavelet_decode(ptr(coef), ptr(mean), ptr(std), ptr(pix, pix.dtype), _PIX[pix.dtype], N, Cc, H, W, int(levels),
                                     WAVELET_NORMS[norm], stream()), "lfvdm_wavelet_decode")


def prepare_batch_wavelet(pool, table, batch, frame_indices, obs_mask, latent_mask, levels, norm, mean=None, rstd=None):
    """``prepare_batch`` on a pool of PIXELS (B, Tp, C, H, W), float32 or uint8, with the wavelet encode folded into the
    gather: batch (B, F, 4^L C, H / 2^L, W / 2^L) (lfvdm_prepare_batch_wavelet)."""
    B, Tp, Cc, H, W = pool.shape
    F = table.shape[1]
    if batch.numel() != B * F * Cc * H * W:
        raise RuntimeError("prepare_batch_wavelet: batch does not hold B * F frames of the pool's size")
    scale, shift = _pix_affine(pool.dtype)
    check(lib().lfvdm_prepare_batch_wavelet(ptr(pool, pool.dtype), _PIX[pool.dtype], scale, shift, ptr(table, torch.int32), ptr(batch),
                                            ptr(frame_indices, torch.int64), ptr(obs_mask), ptr(latent_mask), ptr(mean), ptr(rstd),
                                            B, F, Tp, Cc, H, W, int(levels), WAVELET_NORMS[norm], stream()),
          "lfvdm_prepare_batch_wavelet")


def shapes_trajectories(video_idx, traj, consts, seed, split, stochastic, H, W):
    """video_idx (N,) int64 -> traj (N, T, S, 2) int32 and consts (N, S, 4) int32 of the bouncing-shapes dataset
    (lfvdm_shapes_trajectories); split: 0 train, 1 test."""
    N, T, S = traj.shape[:3]
    if video_idx.numel() != N or tuple(traj.shape) != (N, T, S, 2) or tuple(consts.shape) != (N, S, 4):
        raise RuntimeError("shapes_trajectories: expected video_idx (N,), traj (N, T, S, 2), consts (N, S, 4)")
    check(lib().lfvdm_shapes_trajectories(ptr(video_idx, torch.int64), ptr(traj, torch.int32), ptr(consts, torch.int32),
                                          int(seed) % (1 << 64), int(split), N, T, S, int(H), int(W), int(bool(stochastic)),
                                          stream()), "lfvdm_shapes_trajectories")


def shapes_render(traj, consts, out, table=None, lut=None, frame_indices=None, obs_mask=None, latent_mask=None):
    """traj (N, T, S, 2), consts (N, S, 4) -> out (B, F, 3, H, W) float32 (``lut``: 256 floats) or uint8; N = B (whole videos or
    a table over one video) or 2 B (videos 2 b and 2 b + 1: video 1 and the padding video of batch element b).  ``table``
    (B, F, 4) int32 names the frames as for ``prepare_batch`` and the three index / mask tensors are written when given
    (lfvdm_shapes_render)."""
    N, T, S = traj.shape[:3]
    B, F, Cc, H, W = out.shape
    if Cc != 3 or N % B or N // B not in (1, 2) or tuple(consts.shape) != (N, S, 4) or out.dtype not in _PIX:
        raise RuntimeError("shapes_render: out (B, F, 3, H, W) float32 / uint8 over B or 2 B trajectory videos")
    if table is not None and tuple(table.shape) != (B, F, 4):
        raise RuntimeError("shapes_render: table must be (B, F, 4)")
    for m in (frame_indices, obs_mask, latent_mask):
        if m is not None and m.numel() != B * F:
            raise RuntimeError("shapes_render: index / mask tensors hold B * F elements")
    if lut is not None and lut.numel() != 256:
        raise RuntimeError("shapes_render: the uint8 -> float table has 256 entries")
    check(lib().lfvdm_shapes_render(ptr(traj, torch.int32), ptr(consts, torch.int32), ptr(table, torch.int32), ptr(lut),
                                    ptr(out, out.dtype), _PIX[out.dtype], ptr(frame_indices, torch.int64), ptr(obs_mask),
                                    ptr(latent_mask), B, F, (N // B) * T, T, S, H, W, stream()), "lfvdm_shapes_render")


def masked_mse(a, b, mask, out, B, T, frame_inner):
    check(lib().lfvdm_masked_mse(ptr(a), ptr(b), ptr(mask), ptr(out), B, T, frame_inner, stream()), "lfvdm_masked_mse")


def train_loss(target, pred, mask, eval_mask, t, wtab, mse, eval_mse, loss):
    """The weighted loss head in one launch (lfvdm_train_loss): mse / eval_mse (B,) as ``masked_mse`` gives them under ``mask`` /
    ``eval_mask`` ((B, T) fp32 or None), loss = mse * wtab[t] with the index clamped into the table.  t: (B,) int64."""
    B, T = pred.shape[0], pred.shape[1]
    check(lib().lfvdm_train_loss(ptr(target), ptr(pred), ptr(mask), ptr(eval_mask), ptr(t, torch.int64), ptr(wtab), wtab.numel(),
                                 ptr(mse), ptr(eval_mse), ptr(loss), B, T, pred.numel() // (B * T), stream()), "lfvdm_train_loss")


def train_loss_bwd(target, pred, mask, t, wtab, g, dpred):
    """dpred = g[b] * d loss[b] / d pred (lfvdm_train_loss_bwd); every element is written."""
    B, T = pred.shape[0], pred.shape[1]
    check(lib().lfvdm_train_loss_bwd(ptr(target), ptr(pred), ptr(mask), ptr(t, torch.int64), ptr(wtab), wtab.numel(), ptr(g),
                                     ptr(dpred), B, T, pred.numel() // (B * T), stream()), "lfvdm_train_loss_bwd")


def grad_norm_nparts(n):
    """Workgroups of lfvdm_grad_norm_partials for an arena of n floats = floats of its scratch (a function of n alone)."""
    return int(lib().lfvdm_grad_norm_nparts(int(n)))


def grad_clip_stat(g, grad_scale, max_norm, partials, stat):
    """stat (4 x fp32) <- {squared norm of grad_scale*g, clip coefficient, non-finite flag, += skipped count}: the two norm
    launches in front of ``adamw_ema_clip``.  g: 1-D fp32 (any 4-byte alignment); partials: grad_norm_nparts(g.numel()) floats."""
    n = g.numel()
    if partials.numel() != grad_norm_nparts(n) or stat.numel() != 4:
        raise RuntimeError("grad_clip_stat: partials must hold grad_norm_nparts(n) floats and stat four")
    check(lib().lfvdm_grad_norm_partials(ptr(g), n, float(grad_scale), ptr(partials), partials.numel(), stream()),
          "lfvdm_grad_norm_partials")
    check(lib().lfvdm_grad_norm_finalize(ptr(partials), partials.numel(), float(max_norm), ptr(stat), stream()),
          "lfvdm_grad_norm_finalize")


def adamw_ema_clip(a, stat):
    """lfvdm_adamw_ema on an AdamWArgs with the clip record of ``grad_clip_stat`` applied."""
    check(lib().lfvdm_adamw_ema_clip(C.byref(a), ptr(stat), stream()), "lfvdm_adamw_ema_clip")


class StreamFlags:
    """Counters in device memory that order another stream behind points INSIDE a replayed graph (lfvdm_flag_add /
    lfvdm_flag_wait; one 128-byte line per counter)."""

    def __init__(self, n, device):
        self.buf = torch.zeros(n + 1, 32, device=device, dtype=torch.int32)     # row n: the timed-out word
        self.n = n

    def add(self, k):
        """Counter k += 1 behind everything enqueued so far on the current stream (capturable)."""
        check(lib().lfvdm_flag_add(self.buf[k].data_ptr(), stream()), "lfvdm_flag_add")

    def wait(self, k, target, torch_stream, timeout_s=20.0, also_f32=None):
        """``torch_stream`` proceeds once counter k has reached ``target``.  also_f32: device address of a float that a
        timeout raises to 1.0 as well (the skip word that rides in the last gradient bucket)."""
        wrapped = ((int(target) + 2 ** 31) % 2 ** 32) - 2 ** 31        # the device counter is a wrapping int32: so is the target
        check(lib().lfvdm_flag_wait2(self.buf[k].data_ptr(), wrapped, float(timeout_s), self.buf[self.n].data_ptr(), also_f32,
                                     torch_stream.cuda_stream), "lfvdm_flag_wait2")

    def timed_out_ptr(self):
        """Device address of the timed-out word (lfvdm_adamw_args.skip_flag)."""
        return self.buf[self.n].data_ptr()

    def timed_out(self):
        """Host check (synchronises): did any wait give up?"""
        return bool(self.buf[self.n, 0].item())


def jobs_to_device(jobs, device):
    """Pack a list of ctypes Structures into one uint8 device tensor (job table)."""
    if not jobs:
        return None
    arr = (type(jobs[0]) * len(jobs))(*jobs)
    raw = bytes(memoryview(arr))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


SLOT_PAD, SLOT_OBS, SLOT_LATENT = 0, 1, 2      # LFVDM_SLOT_* of include/lfvdm_hip.h


def search_assemble(pool, table, role, x0, x_start, obs_mask, latent_mask, mask, frame_indices):
    """Windows of the schedule search (lfvdm_search_assemble): pool (V, Tv, ...) fp32, table / role (W, K) int32 -> x0 /
    x_start (W, K, ...), obs_mask / latent_mask / mask (W * K floats each), frame_indices (W, K) int64."""
    V, Tv = pool.shape[:2]
    W, K = table.shape
    check(lib().lfvdm_search_assemble(ptr(pool), ptr(table, torch.int32), ptr(role, torch.int32), ptr(x0), ptr(x_start),
                                      ptr(obs_mask), ptr(latent_mask), ptr(mask), ptr(frame_indices, torch.int64), W, K, V, Tv,
                                      pool[0, 0].numel(), stream()), "lfvdm_search_assemble")


def search_noise_qsample(x_start, table, t_list, ctl, key, sa, sb, noise, x_t, t_buf, V):
    """Head of the search's replayed step (lfvdm_search_noise_qsample): position ctl[0] of ``t_list`` (ctl: int32 [4] =
    position, ticket, list length, unused; key: int64 [2] = seed, window step) -> t_buf, noise, x_t; ctl[0] += 1."""
    W, K = table.shape
    check(lib().lfvdm_search_noise_qsample(ptr(x_start), ptr(table, torch.int32), ptr(t_list, torch.int64), ptr(ctl, torch.int32),
                                           ptr(key, torch.int64), ptr(sa), ptr(sb), ptr(noise), ptr(x_t), ptr(t_buf, torch.int64),
                                           W, K, int(V), x_start[0, 0].numel(), stream()), "lfvdm_search_noise_qsample")


def search_noise_fill(table, seed, step, j, noise, V):
    """The search's noise of timestep position ``j`` for the windows of ``table`` (lfvdm_search_noise_fill) -> ``noise``
    (W, K, ...)."""
    W, K = table.shape
    check(lib().lfvdm_search_noise_fill(ptr(table, torch.int32), int(seed) & (2 ** 64 - 1), int(step), int(j), ptr(noise), W, K,
                                        int(V), noise[0, 0].numel(), stream()), "lfvdm_search_noise_fill")


def search_scores(terms, t_list, scores, G, V, col_base=-1):
    """scores[g] = mean over the V windows of candidate g and the positions of ``t_list`` of ``terms`` (W, ld)
    (lfvdm_search_scores); ``col_base`` as in ``vb_terms``."""
    n_t = t_list.numel() if t_list is not None else terms.shape[1]
    check(lib().lfvdm_search_scores(ptr(terms), ptr(t_list, torch.int64) if t_list is not None else None, ptr(scores), int(G),
                                    int(V), n_t, terms.shape[1], int(col_base), stream()), "lfvdm_search_scores")
