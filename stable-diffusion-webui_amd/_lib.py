"""ctypes binding of libsdmi.so (the C ABI in include/sdmi.h).  No CPU fallback exists: if the library is missing
or fails to load, importing this module raises, and every wrapper raises ``SdmiError`` on a non-zero return code.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDMI_LIB") or os.path.join(_HERE, "lib", "libsdmi.so")      # SDMI_LIB: A/B of two builds (tools/gpu)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdmi.h")

F16, F32 = 0, 1
EP_OUT_F32, EP_GEGLU, EP_NCHW, EP_BIAS_ROW = 1, 2, 4, 8
EP_TRANSPOSE = 64
EP_WRAP = 128
EP_LNFOLD = 0x4000       # sdmi_conv_gemm_ex only
RRDB_EP_NONE, RRDB_EP_LRELU, RRDB_EP_RES1, RRDB_EP_RES2, RRDB_EP_RELU = 0, 1, 2, 3, 4
RRDB_ST_F16, RRDB_ST_F32_NCHW, RRDB_ST_U8_HWC = 0, 1, 2
COMPACT_EP_NONE, COMPACT_EP_PRELU, COMPACT_EP_TAIL = 0, 1, 2


class SdmiError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [
        ("a0", C.c_void_p), ("a1", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("rowbias", C.c_void_p),
        ("resid", C.c_void_p), ("out", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32), ("lda0", C.c_int32), ("lda1", C.c_int32),
        ("B", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("taps", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("up", C.c_int32),
        ("N", C.c_int32), ("n_real", C.c_int32), ("ldo", C.c_int32), ("ldr", C.c_int32),
        ("flags", C.c_int32), ("alpha", C.c_float), ("batch", C.c_int32),
        ("a_bs", C.c_int64), ("w_bs", C.c_int64), ("o_bs", C.c_int64), ("r_bs", C.c_int64),
        ("force_generic", C.c_int32), ("reserved", C.c_int32),
        ("splitk_workspace", C.c_void_p), ("splitk_workspace_bytes", C.c_int64),
    ]


class GemmExtras(C.Structure):
    """include/sdmi.h sdmi_gemm_extras (test entry sdmi_conv_gemm_ex); its leading fields are tests/hostemu/emu.cpp emu_gemm_extras."""
    _fields_ = [
        ("stats_out", C.c_void_p), ("stats_cpg", C.c_int32), ("stats_nchunk", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_s", C.c_void_p), ("ln_np", C.c_int32), ("ln_inv_c", C.c_float), ("ln_eps", C.c_float),
        ("lnp_out", C.c_void_p), ("lnp_np", C.c_int32), ("bias_scale", C.c_float),
        ("out_lo", C.c_void_p), ("resid_lo", C.c_void_p), ("gate", C.c_void_p),
        ("stats_bytes", C.c_int64), ("lnp_bytes", C.c_int64), ("ln_stats_bytes", C.c_int64), ("ln_s_bytes", C.c_int64),
        ("out_lo_bytes", C.c_int64), ("resid_lo_bytes", C.c_int64),
    ]


class RrdbDesc(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("r1", C.c_void_p), ("r2", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32), ("lda", C.c_int32), ("up", C.c_int32),
        ("nout", C.c_int32), ("n_real", C.c_int32), ("ldo", C.c_int32), ("ldr1", C.c_int32), ("ldr2", C.c_int32),
        ("ep", C.c_int32), ("store", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float),
    ]


class CompactDesc(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("slope", C.c_void_p), ("base", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32), ("lda", C.c_int32), ("ldo", C.c_int32),
        ("n_real", C.c_int32), ("ep", C.c_int32), ("r", C.c_int32), ("base_u8", C.c_int32), ("out_u8", C.c_int32), ("grid_cap", C.c_int32),
    ]


class SwinAttnDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32),
        ("ldq", C.c_int32), ("ldo", C.c_int32), ("shift", C.c_int32), ("scale", C.c_float),
    ]


class SwinIRConfigC(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16), ("num_heads", C.c_int32),
                ("mlp_hidden", C.c_int32), ("resi_3conv", C.c_int32), ("scale", C.c_int32)]


class Swin2AttnDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32),
        ("ldq", C.c_int32), ("ldo", C.c_int32), ("shift", C.c_int32), ("head_scale", C.c_void_p),
    ]


class Swin2SRConfigC(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16), ("num_heads", C.c_int32),
                ("mlp_hidden", C.c_int32), ("resi_3conv", C.c_int32), ("upsampler", C.c_int32), ("scale", C.c_int32)]


class ScuBlockDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p), ("packs", C.c_void_p), ("bias", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("ldx", C.c_int32), ("ldo", C.c_int32), ("shift", C.c_int32),
    ]


class ScuNETConfigC(C.Structure):
    _fields_ = [("depths", C.c_int32 * 7)]


class DatAttnDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("bias0", C.c_void_p), ("bias1", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32),
        ("ldq", C.c_int32), ("ldo", C.c_int32), ("s0", C.c_int32), ("s1", C.c_int32),
        ("shift_h", C.c_int32), ("shift_w", C.c_int32), ("scale", C.c_float),
    ]


class DatAimDesc(C.Structure):
    _fields_ = [
        ("s", C.c_void_p), ("t", C.c_void_p), ("gate", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p),
        ("b2", C.c_float), ("out", C.c_void_p), ("rows", C.c_int64),
        ("rows_per_image", C.c_int32), ("C", C.c_int32), ("C16", C.c_int32), ("lds", C.c_int32), ("ldt", C.c_int32), ("ldo", C.c_int32),
    ]


class DATConfigC(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16), ("num_heads", C.c_int32),
                ("split0", C.c_int32), ("split1", C.c_int32), ("ffn_hidden", C.c_int32), ("scale", C.c_int32)]


class HatAttnDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32),
        ("ldq", C.c_int32), ("ldo", C.c_int32), ("mode", C.c_int32), ("shift", C.c_int32), ("scale", C.c_float),
    ]


class HATConfigC(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16), ("num_heads", C.c_int32),
                ("mlp_hidden", C.c_int32), ("cab_mid", C.c_int32), ("cab_squeeze", C.c_int32), ("conv_scale", C.c_float), ("scale", C.c_int32)]


class UNetConfigC(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("model_channels", C.c_int32),
        ("num_levels", C.c_int32), ("channel_mult", C.c_int32 * 8), ("num_res_blocks", C.c_int32),
        ("attn_level", C.c_int32 * 8), ("transformer_depth", C.c_int32 * 8),
        ("num_heads", C.c_int32), ("num_head_channels", C.c_int32), ("context_dim", C.c_int32),
        ("adm_in_channels", C.c_int32), ("reserved", C.c_int32 * 4),
    ]


class VAEConfigC(C.Structure):
    _fields_ = [
        ("ch", C.c_int32), ("num_levels", C.c_int32), ("ch_mult", C.c_int32 * 8),
        ("num_res_blocks", C.c_int32), ("in_channels", C.c_int32), ("out_ch", C.c_int32), ("z_channels", C.c_int32),
        ("scale_factor", C.c_float), ("reserved", C.c_int32 * 4),
    ]


class ClipConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("max_positions", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32),
                ("heads", C.c_int32), ("intermediate", C.c_int32), ("act", C.c_int32), ("eps", C.c_float)]


def declared_symbols() -> list:
    """Every function name declared in include/sdmi.h (used by the CPU-side export test)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdmi_[a-z0-9_]+)\s*\(", src)))


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the MI355X engine.")

lib = C.CDLL(LIB_PATH)

_vp, _i, _i64, _f, _u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
_SIGS = {
    "sdmi_version": (C.c_int, []),
    "sdmi_last_error": (C.c_char_p, []),
    "sdmi_device_ok": (C.c_int, []),
    "sdmi_attention_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "sdmi_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i64, _vp]),
    "sdmi_attention_wide_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "sdmi_attention_wide": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i64, _vp]),
    "sdmi_attention_vt": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "sdmi_attention_vt_ex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp]),
    "sdmi_conv_gemm": (_i, [C.POINTER(ConvDesc), _vp]),
    "sdmi_conv_gemm_ex": (_i, [C.POINTER(ConvDesc), C.POINTER(GemmExtras), _vp]),
    "sdmi_conv_splitk_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "sdmi_bench_conv_gemm": (_i, [C.POINTER(ConvDesc), _i, C.POINTER(C.c_float), _vp]),
    "sdmi_pack_conv_weight": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "sdmi_groupnorm": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _i64, _vp]),
    "sdmi_groupnorm_workspace_bytes": (_i64, [_i, _i, _i]),
    "sdmi_layernorm": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _f, _vp]),
    "sdmi_groupnorm_ex": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _i64, _i, _vp, _vp, _vp]),
    "sdmi_ln_rowstats": (_i, [_vp, _vp, _i64, _i, _f, _vp]),
    "sdmi_ln_fold_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "sdmi_small_linear": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "sdmi_silu_f32": (_i, [_vp, _vp, _i64, _vp]),
    "sdmi_timestep_embedding": (_i, [_vp, _i, _vp, _i, _i, _vp]),
    "sdmi_nchw_to_nhwc": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    "sdmi_add_nchw_residual": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "sdmi_ctx_compare": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sdmi_ctx_update_gated": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sdmi_hn_act": (_i, [_vp, _i64, _i, _vp]),
    "sdmi_axpy_f16": (_i, [_vp, _vp, _vp, _f, _i64, _vp]),
    "sdmi_clip_embed": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sdmi_clip_pool": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sdmi_convert": (_i, [_vp, _i, _vp, _i, _i64, _vp]),
    "sdmi_rowchain_ff_pack_bytes": (_i64, [_i, _i]),
    "sdmi_rowchain_ff_pack": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "sdmi_rowchain_ff": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _f, _vp]),
    "sdmi_xattn_chain": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _f, _vp]),
    "sdmi_philox_randn": (_i, [_vp, _i64, C.c_uint64, C.c_uint32, _vp]),
    "sdmi_slerp": (_i, [_vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    "sdmi_cfg_prepare_input": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp]),
    "sdmi_cfg_prepare_concat": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, _u32, _vp]),
    "sdmi_cfg_combine": (_i, [_vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _i, _i64, _vp]),
    "sdmi_cfg_combine_affine": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i64, _vp]),
    "sdmi_euler_step": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _i64, _vp]),
    "sdmi_dpmpp2m_step": (_i, [_vp, _vp, _vp, _f, _f, _f, _f, _i64, _vp]),
    "sdmi_ddim_step": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _f, _i64, _vp]),
    "sdmi_axpby": (_i, [_vp, _vp, _f, _vp, _f, _i64, _vp]),
    "sdmi_dpm_error_partials": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i64, _vp]),
    "sdmi_lincomb": (_i, [_vp, C.POINTER(_vp), C.POINTER(_f), _i, _i64, _vp]),
    "sdmi_mask_blend": (_i, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "sdmi_latent_resize": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sdmi_image_to_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sdmi_engine_create": (_vp, [_i]),
    "sdmi_engine_destroy": (None, [_vp]),
    "sdmi_unet_configure": (_i, [_vp, C.POINTER(UNetConfigC)]),
    "sdmi_unet_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, _i, C.POINTER(C.c_int64), _i]),
    "sdmi_unet_finalize": (_i, [_vp]),
    "sdmi_clip_configure": (_i, [_vp, _i, C.POINTER(ClipConfigC)]),
    "sdmi_clip_load_tensor": (_i, [_vp, _i, C.c_char_p, _vp, _i, _i, C.POINTER(C.c_int64), _i]),
    "sdmi_clip_finalize": (_i, [_vp, _i]),
    "sdmi_clip_forward": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sdmi_unet_update_weight": (_i, [_vp, C.c_char_p, _vp, _i, _i, C.POINTER(C.c_int64), _i]),
    "sdmi_unet_hypernet_clear": (_i, [_vp]),
    "sdmi_unet_hypernet_begin": (_i, [_vp, _f]),
    "sdmi_unet_hypernet_linear": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i]),
    "sdmi_unet_hypernet_act": (_i, [_vp, _i, _i, _i]),
    "sdmi_unet_hypernet_layernorm": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i]),
    "sdmi_unet_update_vector": (_i, [_vp, C.c_char_p, _vp, _i, _i64, _i]),
    "sdmi_lora_merge": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp]),
    "sdmi_weight_hadamard": (_i, [_vp, _vp, _vp, _vp, _f, _i64, _vp]),
    "sdmi_weight_kron": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "sdmi_weight_ia3": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "sdmi_weight_dora": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "sdmi_vae_configure": (_i, [_vp, C.POINTER(VAEConfigC)]),
    "sdmi_vae_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, _i, C.POINTER(C.c_int64), _i]),
    "sdmi_vae_finalize": (_i, [_vp]),
    "sdmi_unet_set_context": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sdmi_unet_set_context_cached": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sdmi_unet_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sdmi_unet_set_control": (_i, [_vp, _vp, _vp, _i, _i]),
    "sdmi_unet_forward_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sdmi_vae_decode": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "sdmi_vae_encode": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "sdmi_debug_set": (_i, [C.c_char_p, _i]),
    "sdmi_debug_set_str": (_i, [C.c_char_p, C.c_char_p]),
    "sdmi_profile_begin": (_i, []),
    "sdmi_profile_end": (_i, [C.c_char_p, _i]),
    "sdmi_engine_arena_bytes": (_i64, [_vp]),
    "sdmi_engine_set_option": (_i, [_vp, C.c_char_p, _i]),
    "sdmi_engine_tap_count": (_i, [_vp]),
    "sdmi_engine_tap_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_int64)]),
    "sdmi_engine_tap_read": (_i, [_vp, _i, _vp, _vp]),
    "sdmi_rrdb_conv": (_i, [C.POINTER(RrdbDesc), _vp]),
    "sdmi_esrgan_blob_floats": (_i64, [_i, _i]),
    "sdmi_esrgan_create": (_vp, [_vp, _vp, _i64, _i, _i, _i]),
    "sdmi_compact_conv": (_i, [C.POINTER(CompactDesc), _vp]),
    "sdmi_compact_blob_floats": (_i64, [_i, _i]),
    "sdmi_compact_create": (_vp, [_vp, _vp, _i64, _i, _i]),
    "sdmi_swin_attention": (_i, [C.POINTER(SwinAttnDesc), _vp]),
    "sdmi_swin_layernorm": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _f, _vp]),
    "sdmi_swinir_blob_floats": (_i64, [C.POINTER(SwinIRConfigC)]),
    "sdmi_swinir_create": (_vp, [_vp, _vp, _i64, C.POINTER(SwinIRConfigC)]),
    "sdmi_swin2_attention": (_i, [C.POINTER(Swin2AttnDesc), _vp]),
    "sdmi_swin_layernorm_add": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _f, _vp]),
    "sdmi_swin2sr_blob_floats": (_i64, [C.POINTER(Swin2SRConfigC)]),
    "sdmi_swin2sr_create": (_vp, [_vp, _vp, _i64, C.POINTER(Swin2SRConfigC)]),
    "sdmi_scu_block": (_i, [C.POINTER(ScuBlockDesc), _vp]),
    "sdmi_scu_block_pack_bytes": (_i64, [_i]),
    "sdmi_scu_block_pack": (_i, [_vp] * 13 + [_i, _vp]),
    "sdmi_scunet_blob_floats": (_i64, [C.POINTER(ScuNETConfigC)]),
    "sdmi_scunet_create": (_vp, [_vp, _vp, _i64, C.POINTER(ScuNETConfigC)]),
    "sdmi_dat_window_attention": (_i, [C.POINTER(DatAttnDesc), _vp]),
    "sdmi_dat_channel_gram": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "sdmi_dat_channel_softmax": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sdmi_dat_dwconv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "sdmi_dat_pool_gate": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sdmi_dat_aim_combine": (_i, [C.POINTER(DatAimDesc), _vp]),
    "sdmi_dat_blob_floats": (_i64, [C.POINTER(DATConfigC)]),
    "sdmi_dat_create": (_vp, [_vp, _vp, _i64, C.POINTER(DATConfigC)]),
    "sdmi_hat_window_attention": (_i, [C.POINTER(HatAttnDesc), _vp]),
    "sdmi_hat_channel_gate": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sdmi_hat_cab_add": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _f, _vp]),
    "sdmi_hat_blob_floats": (_i64, [C.POINTER(HATConfigC)]),
    "sdmi_hat_create": (_vp, [_vp, _vp, _i64, C.POINTER(HATConfigC)]),
}
for _net in ("esrgan", "compact", "swinir", "swin2sr", "scunet", "dat", "hat"):       # the upscaler nets: create / blob_floats differ (above), the rest is one shape
    _SIGS[f"sdmi_{_net}_destroy"] = (None, [_vp])
    _SIGS[f"sdmi_{_net}_scratch_bytes"] = (_i64, [_vp, _i, _i, _i])
    _SIGS[f"sdmi_{_net}_run"] = (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp])
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)       # AttributeError here == the .so does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


def last_error() -> str:
    return (lib.sdmi_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "sdmi call"):
    if rc != 0:
        raise SdmiError(f"{what} failed: {last_error()}")


def device_ok() -> bool:
    return bool(lib.sdmi_device_ok())


def require_device():
    if not device_ok():
        raise SdmiError("no gfx950 (MI355X) device visible to HIP: the engine has no CPU path")


def ptr(t):
    """data_ptr of a torch tensor (must be contiguous where the kernel assumes it) or None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t) -> int:
    import torch
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float32:
        return F32
    raise SdmiError(f"unsupported dtype {t.dtype}: the engine takes fp16 or fp32 tensors")
