"""Op-level wrappers over the C ABI (torch tensors in, torch tensors out; all compute in HIP kernels).

These are the units the parity tests exercise one by one and what the SdOptimization adapter calls.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import lib, check, ptr, stream_ptr, ConvDesc, F16, F32, EP_OUT_F32, EP_GEGLU, EP_NCHW, EP_BIAS_ROW


def _rup(x, m):
    return (x + m - 1) // m * m


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q k^T * scale) v per head.  q [B,N,H*D], k/v [B,M,H*D] fp16 (last dim contiguous) -> [B,N,H*D] fp16.

    Replaces the math of modules/sd_hijack_optimizations.py:221-281 / hypernetwork.py:382-407 after to_q/to_k/to_v."""
    _lib.require_device()
    assert q.dtype == torch.float16 and k.dtype == torch.float16 and v.dtype == torch.float16
    b, n, c = q.shape
    m = k.shape[1]
    d = c // heads
    q, k, v = [t if t.stride(-1) == 1 and t.stride(0) == t.shape[1] * t.stride(1) else t.contiguous() for t in (q, k, v)]
    out = torch.empty((b, n, c), dtype=torch.float16, device=q.device)
    scale = d ** -0.5 if scale is None else scale
    if heads == 1 and d > 160 and d % 64 == 0:           # the VAE AttnBlock (d = 512): materialised scores, one image at a time
        ws_bytes = lib.sdmi_attention_wide_workspace_bytes(b, n, m, d)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        check(lib.sdmi_attention_wide(ptr(q), ptr(k), ptr(v), ptr(out), b, n, m, d, q.stride(1), k.stride(1), v.stride(1), out.stride(1),
                                      float(scale), ptr(ws), ws_bytes, stream_ptr()), "sdmi_attention_wide")
        return out
    ws_bytes = lib.sdmi_attention_workspace_bytes(b, heads, m, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    check(lib.sdmi_attention(ptr(q), ptr(k), ptr(v), ptr(out), b, heads, n, m, d, q.stride(1), k.stride(1), v.stride(1),
                             out.stride(1), float(scale), ptr(ws), ws_bytes, stream_ptr()), "sdmi_attention")
    return out


def attention_vt(q, k, vt, heads, m, scale=None, force_generic=False):
    """Same with V pre-transposed: vt [B, H*D, Mpad]."""
    b, n, c = q.shape
    d = c // heads
    out = torch.empty((b, n, c), dtype=torch.float16, device=q.device)
    scale = d ** -0.5 if scale is None else scale
    check(lib.sdmi_attention_vt(ptr(q), ptr(k), ptr(vt), ptr(out), b, heads, n, m, d, q.stride(1), k.stride(1), vt.shape[2],
                                out.stride(1), float(scale), 1 if force_generic else 0, stream_ptr()), "sdmi_attention_vt")
    return out


def attention_vt_ex(q, k, vt, heads, m, scale=None, prescaled=False, form=0, force_generic=False):
    """attention_vt with the kernel form chosen by the caller (an "attn_occ" value, 0 = default dispatch); prescaled: q and k already
    carry sqrt(scale * log2(e)) each.  q and k may be views into a stacked q | k tensor (their row stride is passed on)."""
    b, n, _ = q.shape
    d = vt.shape[1] // heads
    out = torch.empty((b, n, heads * d), dtype=torch.float16, device=q.device)
    scale = d ** -0.5 if scale is None else scale
    check(lib.sdmi_attention_vt_ex(ptr(q), ptr(k), ptr(vt), ptr(out), b, heads, n, m, d, q.stride(1), k.stride(1), vt.shape[2],
                                   out.stride(1), float(scale), 1 if prescaled else 0, int(form), 1 if force_generic else 0, stream_ptr()),
          "sdmi_attention_vt_ex")
    return out


def pack_conv_weight(w: torch.Tensor, geglu: bool = False, pad: int = 64) -> torch.Tensor:
    """OIHW / [O,I] weight -> packed fp16 [O_pad][taps][I_pad] on the weight's device."""
    _lib.require_device()
    w = w.contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None]
    o, i, kh, kw = w.shape
    o_pad, i_pad = _rup(o, pad), _rup(i, pad)
    out = torch.empty((o_pad, kh * kw, i_pad), dtype=torch.float16, device=w.device)
    check(lib.sdmi_pack_conv_weight(ptr(w), _lib.dtype_code(w), ptr(out), o, i, kh, kw, o_pad, i_pad, 1 if geglu else 0,
                                    stream_ptr()), "pack_conv_weight")
    return out


def pack_bias(b: Optional[torch.Tensor], n_pad: int, geglu: bool = False) -> Optional[torch.Tensor]:
    if b is None:
        return None
    bf = b.float()
    if geglu:
        o = bf.shape[0]
        half = o // 2
        idx = torch.arange(o, device=bf.device)
        g, r = idx // 64, idx % 64
        src = torch.where(r < 32, g * 32 + r, half + g * 32 + (r - 32))
        bf = bf[src]
    out = torch.zeros(n_pad, dtype=torch.float32, device=b.device)
    out[: bf.shape[0]] = bf
    return out


def conv_gemm(a0: torch.Tensor, w_packed: torch.Tensor, *, a1: Optional[torch.Tensor] = None, bias=None, rowbias=None,
              resid=None, taps: int = 9, stride: int = 1, pad: int = 1, up: bool = False, Ho=None, Wo=None,
              geglu: bool = False, out_f32: bool = False, nchw_real: int = 0, bias_row: bool = False, alpha: float = 1.0,
              impl: str = "mfma", transpose: bool = False, wrap: bool = False) -> torch.Tensor:
    """Implicit-GEMM conv / linear on NHWC fp16 tensors a0 [B,Hi,Wi,c0] (+ a1 [B,Hi,Wi,c1]).
    impl: "mfma" (LDS-direct loads), "mfma_reg" (register-staged variant), "generic" (simple HIP kernel)."""
    _lib.require_device()
    assert a0.dtype == torch.float16 and a0.is_contiguous()
    b, hi, wi, c0 = a0.shape
    c1 = a1.shape[3] if a1 is not None else 0
    n = w_packed.shape[0]
    if Ho is None:
        if up:
            Ho, Wo = 2 * hi, 2 * wi
        elif taps == 9:
            p2 = 2 if pad else 1
            Ho, Wo = (hi + p2 - 3) // stride + 1, (wi + p2 - 3) // stride + 1
        else:
            Ho, Wo = hi, wi
    d = ConvDesc()
    d.a0, d.a1, d.w = a0.data_ptr(), (a1.data_ptr() if a1 is not None else None), w_packed.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.rowbias = rowbias.data_ptr() if rowbias is not None else None
    d.resid = resid.data_ptr() if resid is not None else None
    d.c0, d.c1, d.lda0, d.lda1 = c0, c1, c0, c1
    d.B, d.Hi, d.Wi, d.Ho, d.Wo = b, hi, wi, Ho, Wo
    d.taps, d.stride, d.pad, d.up = taps, stride, pad if taps == 9 else 0, 1 if up else 0
    d.N = n
    flags = 0
    n_out = n
    if geglu:
        flags |= EP_GEGLU
        n_out = n // 2
    if bias_row:
        flags |= EP_BIAS_ROW
    if wrap:
        flags |= _lib.EP_WRAP
    if nchw_real:
        flags |= EP_NCHW
        out = torch.empty((b, nchw_real, Ho, Wo), dtype=torch.float32, device=a0.device)
        d.n_real = nchw_real
    elif out_f32:
        flags |= EP_OUT_F32
        out = torch.empty((b, Ho, Wo, n_out), dtype=torch.float32, device=a0.device)
    elif transpose:
        flags |= _lib.EP_TRANSPOSE
        out = torch.empty((b, n_out, Ho * Wo), dtype=torch.float16, device=a0.device)       # out^T per image (V^T for attention)
    else:
        out = torch.empty((b, Ho, Wo, n_out), dtype=torch.float16, device=a0.device)
    d.out = out.data_ptr()
    d.ldo = Ho * Wo if transpose else n_out
    d.ldr = resid.shape[-1] if resid is not None else 0
    d.flags = flags
    d.alpha = alpha
    d.batch = 1
    d.force_generic = {"mfma": 0, "generic": 1, "mfma_reg": 2}[impl]
    wsb = lib.sdmi_conv_splitk_workspace_bytes(b * Ho * Wo, n, taps * (c0 + c1), 1)
    if wsb and not geglu and not nchw_real:
        ws = torch.empty(wsb, dtype=torch.uint8, device=a0.device)       # lets small-M / large-K shapes use split-K
        d.splitk_workspace, d.splitk_workspace_bytes = ws.data_ptr(), wsb
    check(lib.sdmi_conv_gemm(C.byref(d), stream_ptr()), "sdmi_conv_gemm")
    return out


def groupnorm(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, x1: Optional[torch.Tensor] = None,
              groups: int = 32, eps: float = 1e-5, silu: bool = True) -> torch.Tensor:
    """GroupNorm(+SiLU) over NHWC fp16 [B,H,W,c0] (optionally channel-concatenated with x1) -> [B,H,W,c0+c1] fp16."""
    _lib.require_device()
    b, h, w, c0 = x0.shape
    c1 = x1.shape[3] if x1 is not None else 0
    out = torch.empty((b, h, w, c0 + c1), dtype=torch.float16, device=x0.device)
    wsb = lib.sdmi_groupnorm_workspace_bytes(b, h * w, groups)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x0.device)
    check(lib.sdmi_groupnorm(ptr(x0), ptr(x1), c0, c1, ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()),
                             ptr(out), b, h * w, groups, float(eps), 1 if silu else 0, ptr(ws), wsb, stream_ptr()), "sdmi_groupnorm")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    _lib.require_device()
    c = x.shape[-1]
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib.sdmi_layernorm(ptr(x), ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()), ptr(out),
                             x.numel() // c, c, float(eps), stream_ptr()), "sdmi_layernorm")
    return out


def rowchain_ff_pack(w1: torch.Tensor, b1, w2: torch.Tensor) -> torch.Tensor:
    """Packed operand stream of the fused feed-forward chain (csrc/rowchain.hip): w1 [2*hidden, C] = ff.net.0.proj.weight (value rows,
    then gate rows), b1 [2*hidden] or None, w2 [C, hidden] = ff.net.2.weight."""
    _lib.require_device()
    hidden, c = w2.shape[1], w2.shape[0]
    w1, w2 = w1.half().contiguous(), w2.half().contiguous()
    b1 = b1.float().contiguous() if b1 is not None else None
    packs = torch.empty(int(lib.sdmi_rowchain_ff_pack_bytes(c, hidden)), dtype=torch.uint8, device=w1.device)
    check(lib.sdmi_rowchain_ff_pack(ptr(w1), ptr(b1) if b1 is not None else None, ptr(w2), ptr(packs), c, hidden, stream_ptr()),
          "sdmi_rowchain_ff_pack")
    return packs


def rowchain_ff(x: torch.Tensor, gamma, beta, packs: torch.Tensor, b2, hidden: int, eps: float = 1e-5) -> torch.Tensor:
    """x + ff(LayerNorm(x)) of a BasicTransformerBlock (GEGLU feed-forward) as one launch; x [rows, C] fp16, rows % 128 == 0."""
    _lib.require_device()
    c = x.shape[-1]
    x = x.contiguous()
    out = torch.empty_like(x)
    b2 = b2.float().contiguous() if b2 is not None else None
    check(lib.sdmi_rowchain_ff(ptr(x), ptr(out), ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()), ptr(packs),
                               ptr(b2) if b2 is not None else None, x.numel() // c, c, hidden, float(eps), stream_ptr()), "sdmi_rowchain_ff")
    return out


def xattn_chain(x: torch.Tensor, gamma, beta, wq: torch.Tensor, wo: torch.Tensor, bo, k: torch.Tensor, vt: torch.Tensor, L: int,
                heads: int = 8, eps: float = 1e-5) -> torch.Tensor:
    """x + attn2(LayerNorm(x), context) of a BasicTransformerBlock at the 320-wide level as one launch (csrc/xattn_chain.hip).
    x [images, rows_per_image, C] fp16 (rows_per_image % 128 == 0); wq / wo [C, C]; bo [C] or None; k [images, L, C] = to_k(context);
    vt [images, C, Lpad] = to_v(context) transposed, Lpad a multiple of 32 (the engine pads to 64)."""
    _lib.require_device()
    images, rpi, c = x.shape
    x = x.contiguous()
    out = torch.empty_like(x)
    wq, wo, k, vt = wq.half().contiguous(), wo.half().contiguous(), k.half().contiguous(), vt.half().contiguous()
    bo = bo.float().contiguous() if bo is not None else None
    check(lib.sdmi_xattn_chain(ptr(x), ptr(out), ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()), ptr(wq), ptr(wo),
                               ptr(bo) if bo is not None else None, ptr(k), ptr(vt), images * rpi, rpi, c, heads, int(L), vt.shape[-1],
                               float(eps), stream_ptr()), "sdmi_xattn_chain")
    return out


def philox_randn(shape, seed: int, offset: int, device) -> torch.Tensor:
    """One draw of rng_philox.Generator(seed) at ``offset`` (modules/rng_philox.py:84-102), generated on the GPU."""
    _lib.require_device()
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    check(lib.sdmi_philox_randn(ptr(out), out.numel(), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint32(offset), stream_ptr()),
          "sdmi_philox_randn")
    return out


def lincomb(out: torch.Tensor, terms, coefs) -> torch.Tensor:
    """out = sum_k coefs[k] * terms[k] on fp32 tensors of one shape (out may be one of the terms)."""
    _lib.require_device()
    n = len(terms)
    assert 1 <= n <= 6 and len(coefs) == n
    for t in terms:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()
    assert out.dtype == torch.float32 and out.is_contiguous()
    tarr = (C.c_void_p * n)(*[t.data_ptr() for t in terms])
    carr = (C.c_float * n)(*[float(c) for c in coefs])
    check(lib.sdmi_lincomb(ptr(out), tarr, carr, n, out.numel(), stream_ptr()), "sdmi_lincomb")
    return out


def mask_blend(x: torch.Tensor, init: torch.Tensor, mask: torch.Tensor, nmask: torch.Tensor) -> torch.Tensor:
    """x = init*mask + nmask*x in place (modules/sd_samplers_cfg_denoiser.py:206-209); mask/nmask are broadcast to x's shape."""
    _lib.require_device()
    m = mask.to(x.device, torch.float32).expand_as(x).contiguous()
    nm = nmask.to(x.device, torch.float32).expand_as(x).contiguous()
    init = init.to(x.device, torch.float32).expand_as(x).contiguous()
    check(lib.sdmi_mask_blend(ptr(x), ptr(init), ptr(m), ptr(nm), x.numel(), stream_ptr()), "sdmi_mask_blend")
    return x


def latent_resize(x: torch.Tensor, size, mode: str = "bilinear", antialias: bool = False) -> torch.Tensor:
    """F.interpolate(x, size=size, mode=mode, antialias=antialias) for fp32 NCHW latents (modules/processing.py:1392; antialias with
    the bilinear / bicubic modes only, as in torch)."""
    _lib.require_device()
    x = x.float().contiguous()
    b, c, hi, wi = x.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=x.device)
    code = {"nearest": 0, "nearest-exact": 1, "bilinear": 2, "bicubic": 3}[mode]
    if antialias:
        if mode not in ("bilinear", "bicubic"):
            raise ValueError("antialias is defined for the bilinear and bicubic modes")     # torch raises the same way
        code += 2
    check(lib.sdmi_latent_resize(ptr(x), ptr(out), b * c, hi, wi, ho, wo, code, stream_ptr()), "sdmi_latent_resize")
    return out


def image_to_u8(img: torch.Tensor) -> torch.Tensor:
    """fp32 NCHW in [-1,1] -> uint8 NHWC (modules/processing.py:1004-1005, 1034-1035)."""
    _lib.require_device()
    img = img.float().contiguous()
    b, c, h, w = img.shape
    out = torch.empty((b, h, w, c), dtype=torch.uint8, device=img.device)
    check(lib.sdmi_image_to_u8(ptr(img), ptr(out), b, c, h, w, stream_ptr()), "sdmi_image_to_u8")
    return out


def pack_rrdb_weight(w: torch.Tensor, nout: Optional[int] = None) -> torch.Tensor:
    """OIHW 3x3 weight -> fp16 [nout][9][cin] for rrdb_conv: output channels zero-padded to nout (32 or 64; conv_last: 3 -> 32), input
    channels to a multiple of 32 (conv_first: 3 / 12 / 48 -> 32 / 32 / 64)."""
    _lib.require_device()
    w = w.contiguous()
    o, i, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    nout = nout or (32 if o <= 32 else 64)
    cin = _rup(i, 32)
    out = torch.empty((nout, 9, cin), dtype=torch.float16, device=w.device)
    check(lib.sdmi_pack_conv_weight(ptr(w), _lib.dtype_code(w), ptr(out), o, i, 3, 3, nout, cin, 0, stream_ptr()), "pack_rrdb_weight")
    return out


def rrdb_conv(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor] = None, *, cin: Optional[int] = None,
              out: Optional[torch.Tensor] = None, out_offset: int = 0, n_real: Optional[int] = None, ep: str = "lrelu",
              alpha: float = 1.0, r1: Optional[torch.Tensor] = None, beta: float = 1.0, r2: Optional[torch.Tensor] = None,
              up: bool = False, store: str = "f16") -> torch.Tensor:
    """One RRDBNet 3x3 conv launch (csrc/rrdb.hip; a line of ResidualDenseBlock.forward, basicsr/archs/rrdbnet_arch.py).
    x [B,H,W,lda] fp16 NHWC: its first `cin` channels are the input (a dense block's concat is a channel prefix of one buffer); with `up`
    the conv runs on the nearest-x2 enlargement of x without building it.  The nout = w_packed.shape[0] output channels go to channels
    [out_offset, out_offset + n_real) of `out` [B,Ho,Wo,ldo] (fp16; made if None), or with store = "f32_nchw" / "u8_hwc" to a new
    [B,n_real,Ho,Wo] fp32 / [B,Ho,Wo,n_real] uint8 (clamp, x255, round half to even) tensor.
    ep: "none" | "lrelu" | "res1" (alpha * v + r1) | "res2" (beta * (alpha * v + r1) + r2); r1 / r2 [B,Ho,Wo,ld] fp16, first nout channels."""
    _lib.require_device()
    assert x.dtype == torch.float16 and x.is_contiguous() and w_packed.dtype == torch.float16 and w_packed.is_contiguous()
    b, hi, wi, lda = x.shape
    nout, cin_w = w_packed.shape[0], w_packed.shape[2]
    cin = cin_w if cin is None else cin
    assert cin == cin_w, "the packed weights fix the number of input channels"
    ho, wo = (2 * hi, 2 * wi) if up else (hi, wi)
    n_real = nout if n_real is None else n_real
    d = _lib.RrdbDesc()
    d.in_, d.w = x.data_ptr(), w_packed.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == nout
    for name, r in (("r1", r1), ("r2", r2)):
        if r is not None:
            assert r.dtype == torch.float16 and r.is_contiguous() and tuple(r.shape[:3]) == (b, ho, wo)
            setattr(d, name, r.data_ptr())
            setattr(d, "ld" + name, r.shape[3])
    d.B, d.H, d.W, d.cin, d.lda, d.up = b, ho, wo, cin, lda, 1 if up else 0
    d.nout, d.n_real = nout, n_real
    d.ep = {"none": _lib.RRDB_EP_NONE, "lrelu": _lib.RRDB_EP_LRELU, "res1": _lib.RRDB_EP_RES1, "res2": _lib.RRDB_EP_RES2,
            "relu": _lib.RRDB_EP_RELU}[ep]
    d.store = {"f16": _lib.RRDB_ST_F16, "f32_nchw": _lib.RRDB_ST_F32_NCHW, "u8_hwc": _lib.RRDB_ST_U8_HWC}[store]
    d.alpha, d.beta = alpha, beta
    if store == "f16":
        if out is None:
            out = torch.empty((b, ho, wo, out_offset + n_real), dtype=torch.float16, device=x.device)
        assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape[:3]) == (b, ho, wo)
        assert out_offset + n_real <= out.shape[3]
        d.out, d.ldo = out.data_ptr() + 2 * out_offset, out.shape[3]
    elif store == "f32_nchw":
        out = torch.empty((b, n_real, ho, wo), dtype=torch.float32, device=x.device)
        d.out = out.data_ptr()
    else:
        out = torch.empty((b, ho, wo, n_real), dtype=torch.uint8, device=x.device)
        d.out = out.data_ptr()
    check(lib.sdmi_rrdb_conv(C.byref(d), stream_ptr()), "sdmi_rrdb_conv")
    return out


def pack_compact_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 weight -> fp16 [64][9][cin] for compact_conv: output channels zero-padded to 64 (the last conv: 3 r^2 -> 64), input
    channels to 32 (the first conv: 3 -> 32) or 64."""
    _lib.require_device()
    w = w.contiguous()
    o, i, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and o <= 64 and i <= 64
    cin = _rup(i, 32)
    out = torch.empty((64, 9, cin), dtype=torch.float16, device=w.device)
    check(lib.sdmi_pack_conv_weight(ptr(w), _lib.dtype_code(w), ptr(out), o, i, 3, 3, 64, cin, 0, stream_ptr()), "pack_compact_weight")
    return out


def compact_conv(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor] = None, *, slope: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, n_real: Optional[int] = None, ep: str = "prelu", r: int = 0,
                 base: Optional[torch.Tensor] = None, store: str = "f32_nchw", grid_cap: int = 0) -> torch.Tensor:
    """One launch of the compact Real-ESRGAN 3x3 conv (csrc/compact.hip; a conv + PReLU pair of SRVGGNetCompact.forward,
    realesrgan/archs/srvgg_arch.py).  x [B,H,W,lda] fp16 NHWC: its first cin = w_packed.shape[2] (32 | 64) channels are the input.
    ep "none" | "prelu" (slope: fp32 [64]): n_real (default 64) channels go to the first channels of `out` [B,H,W,ldo] (fp16; made if
    None; never x itself).  ep "tail": the last conv, n_real = 3 r^2 — pixel shuffle by r plus the nearest-upsampled `base` (the network's
    input: uint8 [B,H,W,3], divided by 255, or fp32 [B,3,H,W]) -> store "f32_nchw" [B,3,H r,W r] fp32 or "u8_hwc" [B,H r,W r,3] uint8
    (clamp, x255, round half to even).  grid_cap: 0 = one persistent workgroup per tile up to the CU count; n > 0: at most n workgroups."""
    _lib.require_device()
    assert x.dtype == torch.float16 and x.is_contiguous() and w_packed.dtype == torch.float16 and w_packed.is_contiguous()
    b, h, w, lda = x.shape
    d = _lib.CompactDesc()
    d.in_, d.w = x.data_ptr(), w_packed.data_ptr()
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == 64
        d.bias = bias.data_ptr()
    if slope is not None:
        assert slope.dtype == torch.float32 and slope.numel() == 64
        d.slope = slope.data_ptr()
    d.B, d.H, d.W, d.cin, d.lda = b, h, w, w_packed.shape[2], lda
    d.ep = {"none": _lib.COMPACT_EP_NONE, "prelu": _lib.COMPACT_EP_PRELU, "tail": _lib.COMPACT_EP_TAIL}[ep]
    d.grid_cap = grid_cap
    if ep == "tail":
        d.r, d.n_real = r, (3 * r * r if n_real is None else n_real)
        if base is not None:
            assert base.is_contiguous() and base.dtype in (torch.uint8, torch.float32)
            assert tuple(base.shape) == ((b, h, w, 3) if base.dtype == torch.uint8 else (b, 3, h, w))
            d.base, d.base_u8 = base.data_ptr(), 1 if base.dtype == torch.uint8 else 0
        rs = max(r, 0)
        out = (torch.empty((b, h * rs, w * rs, 3), dtype=torch.uint8, device=x.device) if store == "u8_hwc"
               else torch.empty((b, 3, h * rs, w * rs), dtype=torch.float32, device=x.device))
        d.out, d.out_u8 = out.data_ptr(), 1 if store == "u8_hwc" else 0
    else:
        d.n_real = 64 if n_real is None else n_real
        if out is None:
            out = torch.empty((b, h, w, d.n_real), dtype=torch.float16, device=x.device)
        assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape[:3]) == (b, h, w)
        d.out, d.ldo = out.data_ptr(), out.shape[3]
    check(lib.sdmi_compact_conv(C.byref(d), stream_ptr()), "sdmi_compact_conv")
    return out


def swin_attention(qkv: torch.Tensor, bias: torch.Tensor, heads: int, d: int, shift: int = 0, scale: Optional[float] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Shifted-window attention of a SwinIR block (csrc/swinir.hip; window 8, head dim d <= 32): the roll, the window partition, the
    relative-position bias, the shift mask, softmax and the product with v of SwinTransformerBlock.forward / WindowAttention.forward
    between the qkv and proj linears.  qkv fp16 [B, H, W, ldq]: head h has q / k / v in 32-wide slots at columns h*32, (heads + h)*32,
    (2 heads + h)*32, dims d..31 zero; bias fp32 [heads, 64, 64]; shift 0 | 4 -> fp16 [B, H, W, ldo] (ldo = 32 heads, or `out`'s row
    width: columns past 32 heads keep their bits), head h at columns h*32 with dims d..31 zero."""
    _lib.require_device()
    assert qkv.dtype == torch.float16 and qkv.dim() == 4 and qkv.is_contiguous()
    b, h, w, ldq = qkv.shape
    bias = bias.float().contiguous()
    assert tuple(bias.shape) == (heads, 64, 64)
    if out is None:
        out = torch.empty((b, h, w, 32 * heads), dtype=torch.float16, device=qkv.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape[:3]) == (b, h, w)
    desc = _lib.SwinAttnDesc()
    desc.qkv, desc.bias, desc.out = qkv.data_ptr(), bias.data_ptr(), out.data_ptr()
    desc.B, desc.H, desc.W, desc.heads, desc.D = b, h, w, heads, d
    desc.ldq, desc.ldo, desc.shift, desc.scale = ldq, out.shape[3], shift, float(d ** -0.5 if scale is None else scale)
    check(lib.sdmi_swin_attention(C.byref(desc), stream_ptr()), "sdmi_swin_attention")
    return out


def swin_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the first C = len(gamma) columns of fp16 rows [..., ld] (ld >= C rounded up to 64): columns C .. roundup(C, 64) - 1
    of the result are zeros (the engine's padded token rows, csrc/swinir.hip); columns past that keep `out`'s bits."""
    _lib.require_device()
    assert x.dtype == torch.float16 and x.is_contiguous()
    c, ld = gamma.numel(), x.shape[-1]
    if out is None:
        out = torch.zeros_like(x)
    assert out.dtype == torch.float16 and out.is_contiguous() and out.shape == x.shape
    check(lib.sdmi_swin_layernorm(ptr(x), ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()), ptr(out), x.numel() // ld, c, ld,
                                  float(eps), stream_ptr()), "sdmi_swin_layernorm")
    return out


def swin2_attention(qkv: torch.Tensor, bias: torch.Tensor, head_scale: torch.Tensor, heads: int, d: int, shift: int = 0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cosine window attention of a Swin2SR (Swin-V2) block (csrc/swinir.hip; window 8, head dim d <= 32): swin_attention's layout and
    geometry with the score cos(q, k) * head_scale[h] + bias + mask.  bias fp32 [heads, 64, 64] = 16 sigmoid(cpb_mlp(coords)) expanded;
    head_scale fp32 [heads] = exp(min(logit_scale, ln 100)).  The norms are taken in fp32 from the fp16 q / k as stored; a token whose
    q or k is all zero scores bias + mask."""
    _lib.require_device()
    assert qkv.dtype == torch.float16 and qkv.dim() == 4 and qkv.is_contiguous()
    b, h, w, ldq = qkv.shape
    bias = bias.float().contiguous()
    head_scale = head_scale.float().contiguous()
    assert tuple(bias.shape) == (heads, 64, 64) and head_scale.numel() == heads
    if out is None:
        out = torch.empty((b, h, w, 32 * heads), dtype=torch.float16, device=qkv.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape[:3]) == (b, h, w)
    desc = _lib.Swin2AttnDesc()
    desc.qkv, desc.bias, desc.out, desc.head_scale = qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), head_scale.data_ptr()
    desc.B, desc.H, desc.W, desc.heads, desc.D = b, h, w, heads, d
    desc.ldq, desc.ldo, desc.shift = ldq, out.shape[3], shift
    check(lib.sdmi_swin2_attention(C.byref(desc), stream_ptr()), "sdmi_swin2_attention")
    return out


def swin_layernorm_add(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, resid: torch.Tensor, eps: float = 1e-5,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resid + LayerNorm(y) over the first C = len(gamma) columns of fp16 rows [..., ld] (ld >= C rounded up to 64), the res-post-norm
    of a Swin-V2 block (csrc/swinir.hip): columns C .. roundup(C, 64) - 1 of the result are zeros, columns past that keep `out`'s bits.
    `out` may be `resid` (in place), not `y`."""
    _lib.require_device()
    assert y.dtype == torch.float16 and y.is_contiguous() and resid.dtype == torch.float16 and resid.is_contiguous() and resid.shape == y.shape
    c, ld = gamma.numel(), y.shape[-1]
    if out is None:
        out = torch.zeros_like(y)
    assert out.dtype == torch.float16 and out.is_contiguous() and out.shape == y.shape
    check(lib.sdmi_swin_layernorm_add(ptr(y), ptr(gamma.float().contiguous()), ptr(beta.float().contiguous()), ptr(resid), ptr(out),
                                      y.numel() // ld, c, ld, float(eps), stream_ptr()), "sdmi_swin_layernorm_add")
    return out


def scu_block_pack(ln1_g, ln1_b, wqkv, bqkv, wproj, bproj, ln2_g, ln2_b, w1, b1, w2, b2) -> torch.Tensor:
    """The weights of one ScuNET transformer Block (torch layouts; C = len(ln1_g) in {32, 64}) -> the uint8 operand image scu_block reads
    (sdmi_scu_block_pack): matrices as fp16, vectors as fp32."""
    _lib.require_device()
    c = ln1_g.numel()
    n = int(lib.sdmi_scu_block_pack_bytes(c))
    if n <= 0:
        raise _lib.SdmiError(f"sdmi_scu_block_pack_bytes: scu_block is built for C = 32 and 64, not {c}")
    mats = [t.half().contiguous() for t in (wqkv, wproj, w1, w2)]
    vecs = [t.float().contiguous() for t in (ln1_g, ln1_b, bqkv, bproj, ln2_g, ln2_b, b1, b2)]
    packs = torch.empty(n, dtype=torch.uint8, device=wqkv.device)
    check(lib.sdmi_scu_block_pack(ptr(vecs[0]), ptr(vecs[1]), ptr(mats[0]), ptr(vecs[2]), ptr(mats[1]), ptr(vecs[3]), ptr(vecs[4]), ptr(vecs[5]),
                                  ptr(mats[2]), ptr(vecs[6]), ptr(mats[3]), ptr(vecs[7]), ptr(packs), c, stream_ptr()), "sdmi_scu_block_pack")
    return packs


def scu_block(x: torch.Tensor, packs: torch.Tensor, bias: torch.Tensor, c: int, shift: int = 0, col: int = 0,
              out: Optional[torch.Tensor] = None, out_col: int = 0) -> torch.Tensor:
    """The transformer Block of a ScuNET ConvTransBlock as one launch (csrc/scunet.hip; window 8, head dim 32, trans_dim c = 32 | 64):
    x + msa(ln1(x)), then + mlp(ln2(.)), of Block.forward.  x fp16 [B, H, W, ldx]: columns col .. col + c - 1 are the input; bias fp32
    [c / 32, 64, 64]; shift 0 ('W') | 4 ('SW') -> fp16 [B, H, W, ldo], the result in columns out_col .. out_col + c - 1 (a fresh dense
    [B, H, W, c] tensor without `out`; the other columns of `out` keep their bits; `out` may be `x`)."""
    _lib.require_device()
    assert x.dtype == torch.float16 and x.dim() == 4 and x.is_contiguous()
    b, h, w, ldx = x.shape
    bias = bias.float().contiguous()
    if out is None:
        out = torch.empty((b, h, w, c), dtype=torch.float16, device=x.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape[:3]) == (b, h, w)
    desc = _lib.ScuBlockDesc()
    desc.x, desc.out = x.data_ptr() + 2 * col, out.data_ptr() + 2 * out_col
    desc.packs, desc.bias = packs.data_ptr(), bias.data_ptr()
    desc.B, desc.H, desc.W, desc.C = b, h, w, c
    desc.ldx, desc.ldo, desc.shift = ldx, out.shape[3], shift
    check(lib.sdmi_scu_block(C.byref(desc), stream_ptr()), "sdmi_scu_block")
    return out
