"""ctypes binding of libs2p_hip.so (C ABI declared in include/s2p_hip.h).

The product path has NO CPU fallback: `lib()` raises if the shared library is missing, and every op
raises if a tensor is not on a HIP device.  PyTorch is used only for device memory and streams.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "csrc", "libs2p_hip.so")     # (tools/uselib.py points this at a second build for an A/B; no environment variable is read here)

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SWISH = 0, 1, 2, 3, 4
EPI_STORE, EPI_ADD, EPI_MUL_ACTGRAD = 0, 1, 2
# s2p_conv2d_path: the dispatcher's path of a conv problem; for PATH_HALO the kernel variant is in bits 8 and up (halo_path), for
# PATH_THIN the kernel behind it (thin_path)
(PATH_THIN, PATH_THIN4, PATH_THIN_CIN, PATH_THIN_ROWS, PATH_PLANE, PATH_PLANEG, PATH_HALO, PATH_SPLITK, PATH_DMA, PATH_PHASES,
 PATH_GENERIC) = range(11)
HALO_S9_176_PIPE, HALO_S9_176, HALO_S9_320, HALO_R_176, HALO_R_320 = range(5)
THIN_LANES, THIN_TILED, THIN_ROWS, THIN_HEAD, THIN_HEAD_MFMA = range(5)
# s2p_in_norm_form: the launch form of an InstanceNorm problem (the reduce + apply pair, a fused launch of 256 / 512 / 1024 threads, a
# large-plane forward of <channels per slab> x <chunks per thread>, the diagnostics-only 32-channel 1024-thread variant)
(NORM_FORM_PAIR, NORM_FORM_F256, NORM_FORM_F512, NORM_FORM_F1024, NORM_FORM_L64X28, NORM_FORM_L32X14, NORM_FORM_L16X28,
 NORM_FORM_F1024_CS32) = range(8)

c_int, c_float, c_void_p, c_int64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "dtype", "N", "H", "W", "Cin", "x_pitch", "Ho", "Wo", "Cout", "y_pitch",
        "KH", "KW", "stride", "pad", "transposed", "reflect", "groups", "x_gstride", "y_gstride", "cin_real")]


class L1Job(ctypes.Structure):
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("grad_a", c_void_p), ("count", c_int64), ("scale", c_float),
                ("loss_out", c_void_p)]


class WgradJob(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("dy", c_void_p), ("dw", c_void_p), ("db", c_void_p)]


class PackJob(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("dst_fwd", c_void_p), ("dst_bwd", c_void_p),
                ("R", ctypes.c_int32), ("T", ctypes.c_int32), ("C", ctypes.c_int32),
                ("Cpad", ctypes.c_int32), ("Rrow", ctypes.c_int32), ("r_off", ctypes.c_int32),
                ("dtype", ctypes.c_int32)]


class SnJob(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("u", c_void_p), ("v", c_void_p), ("sigma", c_void_p), ("ws", c_void_p), ("grad", c_void_p),
                ("R", ctypes.c_int32), ("K", ctypes.c_int32)]


class MlpFwdGroup(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("pre", c_void_p), ("act", c_void_p),
                ("x_pitch", ctypes.c_int32), ("y_pitch", ctypes.c_int32), ("rows", ctypes.c_int32), ("K", ctypes.c_int32)]


class ChainMlp(ctypes.Structure):
    """s2p_chain_mlp: the packed operands of one Gaussian MLP of the fused posterior chain (k1: the chain columns of its first layer)."""
    _fields_ = [("w1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p), ("w3", c_void_p), ("b3", c_void_p),
                ("k1", ctypes.c_int32), ("w1_row", ctypes.c_int32)]


class ChainMlpBf16(ctypes.Structure):
    """s2p_chain_mlp_bf16: ChainMlp with the three weight operands as bf16 bits (w1_row in bf16 elements); the biases stay fp32."""
    _fields_ = ChainMlp._fields_


class ChainState(ctypes.Structure):
    """s2p_chain_state: the activations the posterior chain keeps for its backward (t = 0: a0_*, b0_*; t >= 1 time-major: the rest)."""
    _fields_ = [(n, c_void_p) for n in ("a0_h1", "a0_h2", "a0_raw", "b0_h1", "b0_h2", "b0_raw", "h1a", "h2a", "rawa", "h1b", "h2b", "rawb",
                                        "xz")]


class ChainGrads(ctypes.Structure):
    """s2p_chain_grads: what s2p_posterior_chain_bwd writes, time-major."""
    _fields_ = [(n, c_void_p) for n in ("drawa", "dh2a", "dh1a", "drawb", "dh2b", "dh1b", "dxz")]


class ChainMlpBwd(ctypes.Structure):
    """s2p_chain_mlp_bwd: the transposed packs of one chain MLP (k1: the chain columns of its first layer = the rows of w1t)."""
    _fields_ = [("w1t", c_void_p), ("w2t", c_void_p), ("w3t", c_void_p), ("k1", ctypes.c_int32), ("w1t_row", ctypes.c_int32)]


class ChainMlpBwdBf16(ctypes.Structure):
    """s2p_chain_mlp_bwd_bf16: ChainMlpBwd with the three transposed packs as bf16 bits (w1t_row in bf16 elements)."""
    _fields_ = ChainMlpBwd._fields_


class Bf16PackJob(ctypes.Structure):
    """s2p_bf16_pack_job: fp32 src [rows][cols] -> bf16 dst [rows][dst_pitch] and / or its transpose dst_t [cols][dst_t_pitch]."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("dst_t", c_void_p), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("src_pitch", ctypes.c_int32), ("dst_pitch", ctypes.c_int32), ("dst_t_pitch", ctypes.c_int32)]


class PolicyMlp(ctypes.Structure):
    """s2p_policy_mlp: the packed layers of a two-hidden-layer tanh policy for the closed-loop chain (w3 / b3: the last_fc rows first)."""
    _fields_ = [("w1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p), ("w3", c_void_p), ("b3", c_void_p),
                ("w1_row", ctypes.c_int32), ("width", ctypes.c_int32)]


class PolicyMlpBf16(ctypes.Structure):
    """s2p_policy_mlp_bf16: PolicyMlp with the three weight operands as bf16 bits (w1_row in bf16 elements); the biases stay fp32."""
    _fields_ = PolicyMlp._fields_


class MlpBwdGroup(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("dpre", c_void_p), ("w", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("pre_prev", c_void_p),
                ("dprev", c_void_p), ("x_pitch", ctypes.c_int32), ("dpre_pitch", ctypes.c_int32), ("prev_pitch", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("K", ctypes.c_int32)]


# name -> argtypes; every entry returns int unless listed in _RESTYPE
_P = c_void_p
_DESC = ctypes.POINTER(ConvDesc)
SIGNATURES = {
    "s2p_version": [],
    "s2p_last_error": [],
    "s2p_conv2d_fwd": [_DESC, _P, _P, _P, _P, _P, c_int, c_float, c_int, _P],
    "s2p_conv2d_dgrad": [_DESC, _P, _P, _P, _P, _P, c_int, c_int, c_float, _P],
    "s2p_conv2d_fwd_workspace": [_DESC, c_int],
    "s2p_conv2d_fwd_ws": [_DESC, _P, _P, _P, _P, _P, c_int, c_float, c_int, _P, ctypes.c_size_t, _P],
    "s2p_conv2d_fwd_mat": [_DESC, _P, _P, _P, _P, _P, c_int, _P, c_int, _P, c_int, c_int, c_float, c_float, _P, c_int, _P, _P,
                           ctypes.c_size_t, _P],
    "s2p_conv2d_dgrad_mat": [_DESC, _P, _P, _P, _P, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_float, c_float, _P, _P, c_int, _P, c_int,
                             _P, c_int, _P, c_int, _P, ctypes.c_size_t, _P],
    "s2p_conv2d_mat_is_fused": [_DESC, c_int, c_int],
    "s2p_conv2d_path": [_DESC, c_int, c_int],
    "s2p_conv2d_dgrad_workspace": [_DESC],
    "s2p_conv2d_dgrad_ws": [_DESC, _P, _P, _P, _P, _P, c_int, c_int, c_float, _P, ctypes.c_size_t, _P],
    "s2p_conv2d_wgrad": [_DESC, _P, _P, _P, _P, c_int, c_int, c_int64, c_int, _P],
    "s2p_conv2d_wgrad_workspace": [_DESC, c_int, c_int],
    "s2p_conv2d_wgrad_det_workspace": [_DESC, c_int, c_int, c_int],
    "s2p_channel_sum_workspace": [c_int64, c_int],
    "s2p_channel_sum_ws": [c_int, _P, c_int64, c_int, c_int, _P, _P, ctypes.c_size_t, _P],
    "s2p_conv2d_wgrad_ws": [_DESC, _P, _P, _P, _P, c_int, c_int, c_int64, c_int, _P, ctypes.c_size_t, _P],
    "s2p_conv2d_wgrad_batched_workspace": [_DESC, c_int, c_int, c_int],
    "s2p_conv2d_wgrad_batched": [_DESC, ctypes.POINTER(WgradJob), c_int, c_int, c_int, _P, ctypes.c_size_t, _P],
    "s2p_reflect_pad_bwd": [c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, _P],
    "s2p_channel_sum": [c_int, _P, c_int64, c_int, c_int, _P, _P],
    "s2p_in_stats": [c_int, _P, c_int, c_int, c_int, c_int, c_float, _P, _P],
    "s2p_in_apply_fwd": [c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int, c_float,
                         c_float, _P, c_int, _P],
    "s2p_in_norm_fwd": [c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_float, c_float, _P, c_int,
                        _P, _P],
    "s2p_in_bwd_reduce": [c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int,
                          c_float, c_float, _P, _P],
    "s2p_in_bwd_apply": [c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int,
                         c_float, c_float, _P, _P, c_int, _P, c_int, _P, c_int, _P],
    "s2p_in_norm_bwd": [c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int,
                        c_float, c_float, _P, _P, c_int, _P, c_int, _P, c_int, _P],
    "s2p_in_norm_bwd_res": [c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int,
                            c_float, c_float, _P, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P],
    "s2p_in_norm_form": [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int],
    "s2p_in_stats_floats": [c_int, c_int, c_int],
    "s2p_in_bwd_sums_floats": [c_int, c_int, c_int],
    "s2p_linear_fwd": [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_float, _P, c_int, c_int, _P],
    "s2p_linear_bwd_workspace": [c_int, c_int, c_int],
    "s2p_linear_bwd": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_float, _P, c_int, _P, _P,
                       c_int, _P, ctypes.c_size_t, _P],
    "s2p_gauss_head_fwd": [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P],
    "s2p_gauss_head_bwd": [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P],
    "s2p_linear_add_fwd": [_P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_float, _P, c_int, c_int, _P],
    "s2p_posterior_chain_fwd": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlp), _P, c_int, _P, c_int, _P, c_int, c_int, c_int,
                                _P],
    "s2p_posterior_chain_fwd_save": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlp), _P, c_int, _P, c_int, _P, c_int,
                                     ctypes.POINTER(ChainState), c_int, c_int, _P],
    "s2p_posterior_chain_bwd": [_P, c_int, _P, c_int, _P, c_int, _P, c_int, ctypes.POINTER(ChainMlpBwd), ctypes.POINTER(ChainState),
                                ctypes.POINTER(ChainGrads), c_int, c_int, _P],
    "s2p_prior_chain_fwd": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlp), _P, c_int, _P, c_int, _P, c_int, c_int, c_int, _P],
    "s2p_posterior_chain_fwd_bf16": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlpBf16), _P, c_int, _P, c_int, _P, c_int, c_int,
                                     c_int, _P],
    "s2p_prior_chain_fwd_bf16": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlpBf16), _P, c_int, _P, c_int, _P, c_int, c_int, c_int,
                                 _P],
    "s2p_imagine_chain_fwd": [_P, c_int, _P, c_int, ctypes.POINTER(ChainMlp), _P, c_int, _P, c_int, c_int, ctypes.POINTER(PolicyMlp),
                              _P, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, _P],
    "s2p_imagine_chain_fwd_bf16": [_P, c_int, _P, c_int, ctypes.POINTER(ChainMlpBf16), _P, c_int, _P, c_int, c_int,
                                   ctypes.POINTER(PolicyMlpBf16), _P, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, _P],
    "s2p_posterior_chain_fwd_save_bf16": [_P, c_int, _P, _P, _P, c_int, ctypes.POINTER(ChainMlpBf16), _P, c_int, _P, c_int, _P, c_int,
                                          ctypes.POINTER(ChainState), c_int, c_int, _P],
    "s2p_posterior_chain_bwd_bf16": [_P, c_int, _P, c_int, _P, c_int, _P, c_int, ctypes.POINTER(ChainMlpBwdBf16),
                                     ctypes.POINTER(ChainState), ctypes.POINTER(ChainGrads), c_int, c_int, _P],
    "s2p_chain_pack_bf16": [ctypes.POINTER(Bf16PackJob), c_int, _P],
    "s2p_linear_add_bwd": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_float, _P, c_int, _P, _P,
                           c_int, c_int, _P, c_int, _P],
    "s2p_gauss_kl": [_P, _P, c_int, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, c_int, _P, _P, c_int, _P],
    "s2p_gauss_ll": [_P, c_int, _P, c_int, _P, _P, c_int64, c_float, _P, _P, _P, _P],
    "s2p_gauss_ll_image": [c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P, _P],
    "s2p_posenc_fwd": [_P, c_int, c_int, c_int, _P, c_int, _P],
    "s2p_avgpool3x3s2_fwd": [c_int, _P, c_int, c_int, c_int, c_int, _P, _P],
    "s2p_avgpool3x3s2_bwd": [c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P],
    "s2p_maxpool2x2_fwd": [c_int, _P, c_int, c_int, c_int, c_int, _P, _P],
    "s2p_maxpool2x2_bwd": [c_int, _P, _P, c_int, c_int, c_int, c_int, _P, _P],
    "s2p_resize_nearest": [c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P],
    "s2p_nchw_to_nhwc": [c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P],
    "s2p_nhwc_to_nchw": [c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P],
    "s2p_cast": [c_int, _P, c_int, _P, c_int64, _P],
    "s2p_u8_to_nhwc": [c_int, _P, c_int64, c_int, _P, c_int, _P],
    "s2p_nhwc_to_u8": [c_int, _P, c_int, c_int64, c_int, _P, _P],
    "s2p_window_gather_u8": [c_int, _P, c_int64, c_int64, c_int, _P, c_int, _P, c_int, _P, c_int, _P, _P],
    "s2p_decoded_to_frames": [c_int, _P, c_int, c_int64, c_int, c_int, _P, c_int, _P, _P],
    "s2p_feature_window_gather": [_P, c_int64, c_int, c_int, _P, c_int, _P, c_int, _P, _P, _P, c_int, _P, _P, _P, c_int, _P, _P, c_int,
                                  _P, _P, _P],
    "s2p_frame_pair_gather": [_P, c_int64, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_int, _P, _P, _P, _P],
    "s2p_l1_loss": [c_int, _P, _P, c_int64, c_float, _P, _P, c_int, _P],
    "s2p_l1_loss_multi": [c_int, ctypes.POINTER(L1Job), c_int, _P],
    "s2p_hinge_loss": [c_int, _P, c_int64, c_int, c_float, _P, _P, _P],
    "s2p_hinge_loss_strided": [c_int, _P, c_int64, c_int, c_int, c_float, _P, _P, _P],
    "s2p_adam_step": [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int, c_float, _P],
    "s2p_ensemble_head": [_P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_float, c_float, _P, _P,
                          _P, _P, _P],
    "s2p_ensemble_linear_fwd": [_P, c_int64, c_int, _P, _P, ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_int, c_int, c_int, _P, _P,
                                c_int, _P],
    "s2p_ensemble_linear_bwd": [_P, c_int64, c_int, _P, c_int, _P, ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_int, c_int, c_int,
                                _P, _P, _P, _P, c_int, _P],
    "s2p_ensemble_nll": [_P, c_int, _P, c_int64, c_int, _P, c_int64, c_int, c_int, c_int, c_int, _P, _P, c_float, c_float,
                         _P, _P, _P, c_int, _P, _P, _P, _P, _P],
    "s2p_transition_pack": [_P, c_int, _P, c_int, _P, _P, c_int64, c_int, c_int, _P, c_int, _P],
    "s2p_mlp_linear_fwd": [ctypes.POINTER(MlpFwdGroup), c_int, c_int, c_int, _P],
    "s2p_mlp_linear_bwd": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, _P],
    "s2p_iql_critic_head": [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_float, c_float, c_float, c_float, c_float, _P, _P, _P, _P, _P,
                            _P, _P, _P],
    "s2p_tanh_gauss_policy_head": [_P, c_int, _P, c_int, _P, c_int, c_int, _P, _P, c_int, _P, _P],
    "s2p_soft_update": [_P, _P, c_int64, c_float, _P],
    "s2p_mlp_linear_dgrad": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, _P],
    "s2p_mlp_linear_bwd_split_workspace": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int],
    "s2p_mlp_linear_bwd_split": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, c_int, _P, ctypes.c_size_t, _P],
    "s2p_mlp_linear_fwd_bf16": [ctypes.POINTER(MlpFwdGroup), c_int, c_int, c_int, _P],
    "s2p_mlp_linear_bwd_bf16": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, _P],
    "s2p_mlp_linear_dgrad_bf16": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, _P],
    "s2p_mlp_linear_bwd_split_bf16": [ctypes.POINTER(MlpBwdGroup), c_int, c_int, c_int, c_int, _P, ctypes.c_size_t, _P],
    "s2p_tanh_gauss_rsample": [_P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, _P, c_int, _P],
    "s2p_tanh_gauss_rsample_bwd": [_P, c_int, _P, c_int, _P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, _P],
    "s2p_sac_policy_head": [_P, _P, _P, c_int, c_int, c_float, c_float, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P],
    "s2p_cql_critic_head": [_P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float, c_float, c_float, c_float,
                            c_int, _P, _P, c_int64, _P, c_int64, _P, _P, _P],
    "s2p_u8_chw_to_nhwc01": [c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P],
    "s2p_feature_action_push": [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, _P],
    "s2p_mlp_linear_fwd_skinny": [ctypes.POINTER(MlpFwdGroup), c_int, c_int, c_int, _P],
    "s2p_adam_step_dev": [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, _P, c_float, _P],
    "s2p_adam_step_dev_part": [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, _P, c_float, c_int, _P],
    "s2p_pack_weights": [_P, c_int, c_int, _P],
    "s2p_pack_weights_scaled": [_P, _P, c_int, c_int, _P],
    "s2p_sn_workspace_floats": [c_int, c_int],
    "s2p_sn_power_iter": [_P, c_int, c_int, c_int, c_int, _P],
    "s2p_sn_project_grad": [_P, c_int, c_int, c_int, _P],
    "s2p_act_bwd": [c_int, _P, _P, c_int64, c_int, c_float, _P, _P],
    "s2p_scale": [c_int, _P, c_int64, _P, _P],
    "s2p_add": [c_int, _P, _P, _P, c_int64, _P],
    "s2p_copy_channels": [c_int, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int64, c_int, _P],
    "s2p_image_metrics": [_P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P],
}
_RESTYPE = {"s2p_last_error": ctypes.c_char_p, "s2p_mlp_linear_bwd_split_workspace": ctypes.c_size_t, "s2p_conv2d_wgrad_det_workspace": ctypes.c_size_t, "s2p_channel_sum_workspace": ctypes.c_size_t, "s2p_conv2d_wgrad_batched_workspace": ctypes.c_size_t, "s2p_conv2d_wgrad_workspace": ctypes.c_size_t, "s2p_conv2d_fwd_workspace": ctypes.c_size_t, "s2p_conv2d_dgrad_workspace": ctypes.c_size_t, "s2p_linear_bwd_workspace": ctypes.c_size_t, "s2p_in_stats_floats": c_int64, "s2p_in_bwd_sums_floats": c_int64,
            "s2p_sn_workspace_floats": c_int64}

_lib = None


def build(force=False):
    """Compile libs2p_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    env = dict(os.environ)
    if force:
        env["FORCE"] = "1"                 # recompile every .hip even when the shipped .so is newer than the sources
    subprocess.check_call(["bash", script], env=env)
    return os.path.join(_HERE, "csrc", "libs2p_hip.so")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                f"libs2p_hip.so not found at {_SO}: the S2P hot path has no CPU fallback; run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc) first")
        L = ctypes.CDLL(_SO)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the export is missing
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, c_int)
        if L.s2p_version() < 125:
            raise RuntimeError("libs2p_hip.so is older than this package")
        _lib = L
    return _lib


def halo_path(kind):
    """The s2p_conv2d_path answer for the halo-resident kernel in variant `kind` (HALO_*)."""
    return PATH_HALO | (kind << 8)


def thin_path(kind):
    """The s2p_conv2d_path answer for the thin-Cout forward on kernel `kind` (THIN_*)."""
    return PATH_THIN | (kind << 8)


def check(rc, what):
    if rc != 0:
        msg = lib().s2p_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def dtype_id(t):
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t}")


def chunk_elems(t):
    return 4 if t == torch.float32 else 8


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("S2P HIP op called with a non-HIP tensor: the product path has no CPU fallback")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream
