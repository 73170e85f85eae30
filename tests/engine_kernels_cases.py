"""The cases of the engine-only elementwise helpers (csrc/elementwise.hip), one launch at a time through the test entries of include/sdmi.h:
sdmi_small_linear, sdmi_silu_f32, sdmi_timestep_embedding, sdmi_nchw_to_nhwc, sdmi_add_nchw_residual, sdmi_ctx_compare,
sdmi_ctx_update_gated, sdmi_hn_act, sdmi_axpy_f16, sdmi_clip_embed, sdmi_clip_pool and sdmi_convert.

Each `check_*` function holds one case: inputs seeded on the CPU, the reference (numpy float32 where the kernel is a copy, one rounding or
a fixed fp32 sequence: asserted bit for bit; float64 otherwise) and the assertions.  It is written against a small back end
(tests/test_gpu_engine_kernels.py; tests/test_cpu_engine_kernels.py runs that file on the host-emulated library):

    be.dev, be.ptr(tensor), be.sp() (stream), be.last_error(), be.knob(name, value), and one method per entry that forwards its
    arguments: be.small_linear(...) is sdmi_small_linear(...)

Outputs sit in sentinel-filled `Guarded` buffers (tests/test_gpu_abi.py); rows wider than the problem hold the sentinel (outputs) or 3000
(inputs) in the gap, and the sentinel must survive.  Every case prints one line with its measured figure and the cap.

Bounds (U = 2^-24; `mag` is the reference's formula with every term replaced by its absolute value, in float64):
  * small_linear: the kernel's own summation is 8 * ceil(K / 512) sequential FMAs per lane and a 6-level butterfly, one unit of slack
    (tests/test_gpu_models.py `_pooled_row_checks`): c0 = 8 ceil(K / 512) + 7.  With mag = sum_k |w_k a_k| + |bias|,
        |pre - ref_pre| <= (c0 + [bias]) U mag                                   (the bias add is one more rounding)
        silu_out:  |out - silu(ref_pre)| <= 1.1 (c0 + [bias]) U mag + 4 U |silu(ref_pre)|      (|silu'| <= 1.0999; the SiLU rule below)
        add:       one more rounding of the sum, U (|val| + |add|).
  * silu_f32: |err| <= 4 U |ref|: one ulp for expf, half an ulp each for the add and the divide, doubled.
  * timestep_embedding: worst |err| against the float64 formula <= 2 x the worst error of the numpy-float32 restatement of the same
    expression on the same inputs + 2^-23 (the device's expf / sinf / cosf are specified to 1-2 ulp where the host's are 0.5-1).
  * nchw_to_nhwc with mix_w: 0.5 fp16 ulp of the reference + (C + 1) U mag: C fmas and the rounding of x * scale.
  * hn_act: the result is one of the two fp16 neighbours of the float64 value, and at most 317 of the 63,488 finite inputs (0.5 %) differ
    from fp16(float64 value); gelu, whose 0.5 v (1 + erf) cancels in the negative tail: |err| <= 0.5 fp16 ulp + 3 |v| U, at most 1,000.
Everything else is bit-equality with numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_gpu_abi
from helpers import seeded
from test_gpu_abi import Guarded, up

U = 2.0 ** -24
F16, F32 = 0, 1
GAP = 3000.0
FILL = -777.0
CAP_ELEMS = 4096 * 256                  # ew_blocks' grid cap: a kernel's stride loop runs a second time past this many elements
BIG = (1 << 20) + 257
SIZES = [1, 255, 257, BIG]
f32, f16 = np.float32, np.float16


def note(family, case, text):
    print(f"[engine kernels {family}] {case}: {text}")


def release():
    test_gpu_abi._ALIVE.clear()


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dv(be, a):
    """numpy array -> a device copy that stays alive until the test ends (None stays None)."""
    return None if a is None else up(tt(a), be.dev)


def host(t):
    return t.detach().cpu().numpy()


def rnd(shape, seed, scale=1.0):
    return seeded(shape, seed, scale).numpy()


def code(a):
    return F16 if a.dtype == np.float16 else F32


def ok(be, rc, what):
    assert rc == 0, (what, be.last_error())
    torch.cuda.synchronize()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, "elements with other bits", int(bad.sum()), "first at", int(np.flatnonzero(bad.reshape(-1))[0]),
                           got.reshape(-1)[bad.reshape(-1)][:4], want.reshape(-1)[bad.reshape(-1)][:4])


def ulp16(x):
    """Spacing of fp16 at |x| (float64 in, float64 out): 2^(e - 10), 2^-24 in the subnormal range."""
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def silu64(x):
    return x / (1.0 + np.exp(-x))


# ---- small_linear / silu_f32 ---------------------------------------------------------------------------------------------------------------
# (B, N, K): the 4-row LDS form (B <= 4), the 16-row one (B <= 16, 16 K fp32 <= 96 KB: K = 1536 fits, 1544 does not), the wave-per-column form
# (N < 256, B > 16 with two or three b0 passes, or no room in LDS); K % 512 != 0 (ragged last lane pass), N % 4 != 0 (clamped weight row,
# guarded store), N = 4116 > 4096 (the grid is capped at 256 blocks: waves 0 .. 4 walk a second column group).
SMALL_LINEAR_GRID = [(1, 255, 8), (1, 256, 320), (4, 258, 2816), (4, 4116, 320), (5, 256, 520), (5, 255, 1280), (16, 258, 1536), (16, 256, 1544),
                     (16, 256, 2816), (16, 4116, 320), (17, 256, 320), (33, 258, 1280)]
# (B, N, K, options)
SMALL_LINEAR_FORMS = {
    "wide-rows-lds": (5, 258, 520, dict(lda_extra=4, ldo_extra=4)),
    "wide-rows-plain": (17, 255, 320, dict(lda_extra=4, ldo_extra=4)),
    "no-bias-lds": (4, 258, 320, dict(bias=False)),
    "no-bias-plain": (33, 255, 520, dict(bias=False)),
    "add-lds": (16, 258, 320, dict(add="separate")),
    "add-aliases-out-lds": (5, 4116, 320, dict(add="alias", ldo_extra=4)),
    "add-aliases-out-plain": (17, 258, 1280, dict(add="alias")),
    "silu-out-lds": (4, 256, 1280, dict(silu_out=True)),
    "silu-out-add-plain": (17, 255, 520, dict(silu_out=True, add="separate")),
}
KNOB_SHAPES = [(4, 256, 320), (5, 4116, 320), (16, 258, 1536), (3, 258, 2816)]


def lds_form(B, N, K):
    return B <= 16 and (4 if B <= 4 else 16) * K * 4 <= 96 * 1024 and N >= 256


def sl_operands(B, N, K, seed):
    a = rnd((B, K), seed, 1.5)
    w = (rnd((N, K), seed + 1) * K ** -0.5).astype(f16)
    bias = rnd((N,), seed + 2, 0.5)
    add = rnd((B, N), seed + 3, 2.0)
    return a, w, bias, add


def sl_launch(be, a, w, bias, add_mode, add, B, N, K, lda, ldo, silu_in=False, silu_out=False):
    """-> out [B, N] on the host.  Input rows wider than K hold 3000 in the gap, output rows wider than N the sentinel, which must survive."""
    abuf = np.full((B, lda), GAP, f32)
    abuf[:, :K] = a
    g = Guarded((B, ldo), torch.float32, be.dev)
    addp = None
    if add_mode == "alias":
        g.t[:, :N].copy_(tt(add))
        addp = be.ptr(g.t)
    elif add_mode == "separate":
        addbuf = np.full((B, ldo), GAP, f32)
        addbuf[:, :N] = add
        addp = be.ptr(dv(be, addbuf))
    ok(be, be.small_linear(be.ptr(dv(be, abuf)), be.ptr(dv(be, w)), be.ptr(dv(be, bias)) if bias is not None else None, addp, be.ptr(g.t),
                                  B, N, K, lda, ldo, int(silu_in), int(silu_out), be.sp()), "sdmi_small_linear")
    full = host(g.t)
    assert g.intact(), "small_linear wrote outside its buffer"
    assert (full[:, N:] == FILL).all(), "small_linear wrote into the columns [N, ldo)"
    return full[:, :N].copy()


def check_small_linear(be, B, N, K, *, lda_extra=0, ldo_extra=0, bias=True, add=None, silu_out=False, seed=100, label=None):
    a, w, b, ad = sl_operands(B, N, K, seed)
    got = sl_launch(be, a, w, b if bias else None, add, ad, B, N, K, K + lda_extra, N + ldo_extra, silu_out=silu_out)
    A, W = a.astype(np.float64), w.astype(np.float64)
    ref, mag = A @ W.T, np.abs(A) @ np.abs(W).T
    c = 8 * math.ceil(K / 512) + 7
    if bias:
        ref, mag, c = ref + b, mag + np.abs(b), c + 1
    bound = c * U * mag
    if silu_out:
        ref, bound = silu64(ref), 1.1 * bound + 4 * U * np.abs(silu64(ref))
    if add:
        bound = bound + U * (np.abs(ref) + np.abs(ad))
        ref = ref + ad
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    form = "lds" if lds_form(B, N, K) else "wave-per-column"
    note("small_linear", label or f"B {B} N {N} K {K}", f"{form}, worst |err| / bound {worst:.3f} (cap 1; c = {c})")
    bad = err > bound
    assert not bad.any(), ("elements over the bound", int(bad.sum()), "first (row, column)", np.argwhere(bad)[0].tolist(), "worst multiple", worst)


def check_small_linear_knob(be, B, N, K):
    """Both values of the small_linear_lds knob give the same bits (with every epilogue term on)."""
    assert lds_form(B, N, K)
    a, w, b, ad = sl_operands(B, N, K, 140)
    outs = {}
    try:
        for v in (1, 0):
            be.knob("small_linear_lds", v)
            outs[v] = sl_launch(be, a, w, b, "separate", ad, B, N, K, K, N, silu_out=True)
    finally:
        be.knob("small_linear_lds", 1)
    assert_bits(outs[1], outs[0], f"small_linear_lds 1 against 0, B {B} N {N} K {K}")
    note("small_linear", f"knob B {B} N {N} K {K}", "lds form and wave-per-column form: same bits")


def check_small_linear_silu_in(be, B, N, K):
    """silu_in = 1 is silu_f32 followed by the plain product, bit for bit (the comment above silu_f32_kernel)."""
    a, w, b, _ = sl_operands(B, N, K, 150)
    a[0, :4] = [0.0, -30.0, 30.0, -0.0]
    fused = sl_launch(be, a, w, b, None, None, B, N, K, K, N, silu_in=True)
    g = Guarded((B, K), torch.float32, be.dev)
    ok(be, be.silu_f32(be.ptr(dv(be, a)), be.ptr(g.t), B * K, be.sp()), "sdmi_silu_f32")
    assert g.intact()
    split = sl_launch(be, host(g.t), w, b, None, None, B, N, K, K, N)
    assert_bits(fused, split, f"silu_in against silu_f32 + small_linear, B {B} N {N} K {K}")
    note("small_linear", f"silu_in B {B} N {N} K {K}", f"{'lds' if lds_form(B, N, K) else 'wave-per-column'}: the bits of silu_f32 + small_linear")


def check_silu_f32(be):
    x = np.concatenate([np.linspace(-30, 30, 120001), [0.0, -0.0, 1e-30, -1e-30], rnd((4096,), 160, 4.0)]).astype(f32)
    g = Guarded(x.shape, torch.float32, be.dev)
    ok(be, be.silu_f32(be.ptr(dv(be, x)), be.ptr(g.t), x.size, be.sp()), "sdmi_silu_f32")
    got = host(g.t).astype(np.float64)
    assert g.intact() and np.isfinite(got).all()
    ref = silu64(x.astype(np.float64))
    assert (got[x == 0] == 0).all()
    nz = ref != 0
    ratio = np.abs(got - ref)[nz] / (U * np.abs(ref[nz]))
    at = float(x[nz][int(ratio.argmax())])
    note("silu_f32", f"n {x.size} on [-30, 30]", f"worst |err| = {float(ratio.max()):.3f} x 2^-24 |ref| at x = {at:.6g} (cap 4)")
    assert float(ratio.max()) <= 4.0, (float(ratio.max()), at)


# ---- timestep_embedding --------------------------------------------------------------------------------------------------------------------
TIMESTEPS = [0.0, 0.25, 1.0, 250.5, 601.0, 999.0, 1000.0]             # every one exact in fp16
TE_SHAPES = [(B, dim) for B in (1, 3, 16) for dim in (2, 34, 320, 33)]


def check_timestep_embedding(be, B, dim):
    from oracle.unet import timestep_embedding as oracle_te
    t = np.array([TIMESTEPS[(3 * B + i) % len(TIMESTEPS)] for i in range(B)], f32)
    assert (t.astype(f16).astype(f32) == t).all()
    outs = {}
    for src in (t, t.astype(f16)):
        g = Guarded((B, dim), torch.float32, be.dev)
        ok(be, be.timestep_embedding(be.ptr(dv(be, src)), code(src), be.ptr(g.t), B, dim, be.sp()), "sdmi_timestep_embedding")
        assert g.intact()
        outs[code(src)] = host(g.t).copy()
    assert_bits(outs[F16], outs[F32], f"timestep_embedding fp16 t against fp32 t, B {B} dim {dim}")
    got = outs[F32]
    half = dim // 2
    j = np.arange(half)
    args64 = t.astype(np.float64)[:, None] * np.exp(-math.log(10000.0) * j / half)[None]
    ref = np.concatenate([np.cos(args64), np.sin(args64)] + ([np.zeros((B, 1))] if dim % 2 else []), axis=1)
    freq32 = np.exp(f32(-9.210340371976184) * j.astype(f32) / f32(half))            # the kernel's expression in numpy float32
    assert freq32.dtype == f32
    args32 = t[:, None] * freq32[None]
    yard_out = np.concatenate([np.cos(args32), np.sin(args32)] + ([np.zeros((B, 1), f32)] if dim % 2 else []), axis=1)
    assert yard_out.dtype == f32
    worst, yard = float(np.abs(got - ref).max()), float(np.abs(yard_out - ref).max())
    note("timestep_embedding", f"B {B} dim {dim}", f"worst |err| vs float64 {worst:.3e}, numpy-float32 yardstick {yard:.3e} (cap {2 * yard + 2.0 ** -23:.3e})")
    assert np.isfinite(got).all() and worst <= 2 * yard + 2.0 ** -23, (worst, yard)
    if dim % 2:
        assert (bits(got[:, -1]) == 0).all()                                          # the odd column is written, with +0
    orc = oracle_te(tt(t), dim).numpy()
    assert orc.shape == got.shape and float(np.abs(orc - got).max()) < 1e-3, "layout [cos | sin] of oracle.unet.timestep_embedding"


# ---- nchw_to_nhwc --------------------------------------------------------------------------------------------------------------------------
VAE_SCALE = float(f32(1.0 / 0.18215))
NCHW_GEOMS = [(B, C, cpad, HW) for C in (3, 4, 8, 9, 16) for cpad in sorted({C, 8, 16, 64}) if cpad >= C for HW in (1, 15, 257) for B in (1, 3)]


def nchw_source(B, C, HW, dtype, seed, away_from_zero=False):
    x = rnd((B, C, HW), seed, 2.0)
    if away_from_zero:
        x = np.sign(x) * (0.5 + np.abs(x) % 7.5)
        x[x == 0] = 0.75
    return x.astype(dtype)


def nchw_launch(be, x, B, C, HW, cpad, scale, mix_w=None, mix_b=None, lo_ch=0):
    g = Guarded((B, HW, cpad), torch.float16, be.dev)
    ok(be, be.nchw_to_nhwc(be.ptr(dv(be, x)), code(x), be.ptr(g.t), B, C, HW, cpad, scale, be.ptr(dv(be, mix_w)), be.ptr(dv(be, mix_b)), lo_ch,
                                  be.sp()), "sdmi_nchw_to_nhwc")
    out = host(g.t).copy()
    assert g.intact(), "nchw_to_nhwc wrote outside its buffer"
    return out


def nchw_want(x, cpad, scale):
    B, C, HW = x.shape
    want = np.zeros((B, HW, cpad), f16)
    want[:, :, :C] = (x.astype(f32) * f32(scale)).astype(f16).transpose(0, 2, 1)
    return want


def check_nchw_plain(be, dtype, scale):
    for n, (B, C, cpad, HW) in enumerate(NCHW_GEOMS):
        x = nchw_source(B, C, HW, dtype, 200 + n)
        assert_bits(nchw_launch(be, x, B, C, HW, cpad, scale), nchw_want(x, cpad, scale), f"nchw_to_nhwc B {B} C {C} cpad {cpad} HW {HW} {np.dtype(dtype).name} scale {scale}")
    note("nchw_to_nhwc", f"{np.dtype(dtype).name} scale {scale:.6g}", f"{len(NCHW_GEOMS)} geometries bit-equal to fp16(fp32(x) * scale), padding channels 0")


def check_nchw_past_the_grid_cap(be):
    B, C, cpad, HW = 1, 3, 8, (1 << 20) + 300
    assert B * HW > CAP_ELEMS
    x = nchw_source(B, C, HW, f32, 260)
    assert_bits(nchw_launch(be, x, B, C, HW, cpad, VAE_SCALE), nchw_want(x, cpad, VAE_SCALE), "nchw_to_nhwc past the grid cap")
    note("nchw_to_nhwc", f"HW {HW}", "second stride of the pixel loop: bit-equal")


def check_nchw_lo(be, dtype):
    B, C, cpad, HW = 3, 4, 64, 257
    scale = VAE_SCALE if dtype == f16 else 1.0
    x = nchw_source(B, C, HW, dtype, 270, away_from_zero=True)
    got = nchw_launch(be, x, B, C, HW, cpad, scale, lo_ch=1)
    v = x.astype(f32) * f32(scale)
    hi = v.astype(f16)
    lo = (v - hi.astype(f32)).astype(f16)
    want = np.zeros((B, HW, cpad), f16)
    want[:, :, :C], want[:, :, C:2 * C] = hi.transpose(0, 2, 1), lo.transpose(0, 2, 1)
    assert (lo != 0).any()
    assert_bits(got, want, f"nchw_to_nhwc lo_ch {np.dtype(dtype).name}")
    back = got[:, :, :C].astype(np.float64) + got[:, :, C:2 * C].astype(np.float64)
    exact = (x.astype(np.float64) * float(f32(scale))).transpose(0, 2, 1)
    rel = float((np.abs(back - exact) / np.abs(exact)).max())
    note("nchw_to_nhwc", f"lo_ch {np.dtype(dtype).name}", f"channels [C, 2C) bit-equal; worst |hi + lo - x| / |x| = {rel:.3e} (cap 2^-21 = {2.0 ** -21:.3e})")
    assert rel <= 2.0 ** -21


def check_nchw_mix(be, dtype, with_bias):
    C, cpad = 4, 8
    mw, mb = rnd((C, C), 280, 0.7), rnd((C,), 281, 0.5)
    worst = 0.0
    for B, HW in ((1, 1), (3, 257)):
        x = nchw_source(B, C, HW, dtype, 282)
        got = nchw_launch(be, x, B, C, HW, cpad, VAE_SCALE, mix_w=mw, mix_b=mb if with_bias else None)
        assert (bits(got[:, :, C:]) == 0).all()
        v = x.astype(np.float64).transpose(0, 2, 1) * VAE_SCALE                          # [B, HW, C]
        ref = v @ mw.astype(np.float64).T + (mb if with_bias else 0.0)
        mag = np.abs(v) @ np.abs(mw.astype(np.float64)).T + (np.abs(mb) if with_bias else 0.0)
        bound = 0.5 * ulp16(ref) + (C + 1) * U * mag
        err = np.abs(got[:, :, :C].astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (B, HW, float((err / bound).max()))
    note("nchw_to_nhwc", f"mix_w {np.dtype(dtype).name} bias {with_bias}", f"worst |err| / (0.5 fp16 ulp + {C + 1} x 2^-24 mag) = {worst:.3f} (cap 1)")


# ---- add_nchw_residual -----------------------------------------------------------------------------------------------------------------------
def check_add_nchw_residual(be, dtype, hilo):
    worst_lo = 0
    for n, (C, HW, B, in_place) in enumerate((C, HW, B, ip) for C in (8, 320) for HW in (1, 63, 1024) for B in (1, 2) for ip in (False, True)):
        src = rnd((B, HW, C), 300 + n, 2.0).astype(f16)
        lo = (rnd((B, HW, C), 400 + n) * 2.0 ** -12).astype(f16) if hilo else None
        ctrl = rnd((B, C, HW), 500 + n, 3.0).astype(dtype)
        ctrl[0, 0, 0] = dtype(1000.25)                                                  # fp16 spacing at 1000 is 0.5: lo carries the rest
        gd, gl = Guarded((B, HW, C), torch.float16, be.dev), Guarded((B, HW, C), torch.float16, be.dev) if hilo else None
        if in_place:
            gd.t.copy_(tt(src))
            if hilo:
                gl.t.copy_(tt(lo))
            sp, slp = be.ptr(gd.t), be.ptr(gl.t) if hilo else None
        else:
            sp, slp = be.ptr(dv(be, src)), be.ptr(dv(be, lo)) if hilo else None
        ok(be, be.add_nchw_residual(sp, slp, be.ptr(dv(be, ctrl)), code(ctrl), be.ptr(gd.t), be.ptr(gl.t) if hilo else None, B, C, HW, be.sp()),
           "sdmi_add_nchw_residual")
        f = (src.astype(f32) + (lo.astype(f32) if hilo else f32(0))) + ctrl.astype(f32).transpose(0, 2, 1)
        assert f.dtype == f32
        want_hi = f.astype(f16)
        want_lo = (f - want_hi.astype(f32)).astype(f16)
        what = f"add_nchw_residual C {C} HW {HW} B {B} {np.dtype(dtype).name} hilo {hilo} in_place {in_place}"
        assert_bits(host(gd.t), want_hi, what + " (hi)")
        assert gd.intact()
        if hilo:
            assert_bits(host(gl.t), want_lo, what + " (lo)")
            assert gl.intact() and (want_lo != 0).any()
            worst_lo = max(worst_lo, int((want_lo != 0).sum()))
    note("add_nchw_residual", f"{np.dtype(dtype).name} hilo {hilo}", f"24 cases bit-equal to the numpy float32 sequence (up to {worst_lo} non-zero lo values per case)")


# ---- ctx_compare / ctx_update_gated ----------------------------------------------------------------------------------------------------------
CTX_GEOMS = [(2, 7, 64, 40), (2, 77, 128, 768), (16, 77, 128, 2048)]


def ctx_positions(n):
    """{label: flat index of the one changed element}"""
    pos = {"element 0": 0, "the last element": n - 1, "lane 37 of a full wave": 64 * 3 + 37, "lane 63 of the first wave": 63}
    if n % 64:
        pos["lane 17 of the last partial wave"] = n // 64 * 64 + 17
    if n > CAP_ELEMS:
        pos["the second stride (beyond 2^20)"] = (1 << 20) + 12345
        pos["the third stride (beyond 2^21)"] = (1 << 21) + 64 * 5 + 1
    assert all(0 <= i < n for i in pos.values())
    return pos


def check_ctx_compare(be, B, L, Lpad, C, dtype):
    n = B * L * C
    h = rnd((B, L, C), 600).astype(f16)
    h[0, 0, 1] = f16(0.0)
    src = h.astype(dtype)
    cached = np.full((B, Lpad, C), 55.0, f16)
    cached[:, :L] = h
    cd, sd = dv(be, cached), dv(be, src)
    gate = Guarded((1,), torch.int32, be.dev)

    def run(what):
        gate.t.zero_()
        ok(be, be.ctx_compare(be.ptr(sd), code(src), be.ptr(cd), B, L, Lpad, C, be.ptr(gate.t), be.sp()), "sdmi_ctx_compare")
        assert gate.intact(), what
        return int(gate.t.cpu()[0])

    assert run("identical") == 0, "an identical context raised the gate"
    flat = sd.view(-1)
    if dtype == f32:
        nudged = src * f32(1 + 2.0 ** -13)
        assert (nudged != src).any() and (bits(nudged.astype(f16)) == bits(h)).all()
        sd.copy_(tt(nudged))
        assert run("nudged") == 0, "fp32 values nudged within the same fp16 raised the gate"
        sd.copy_(tt(src))
    hf = h.reshape(-1)
    for label, i in ctx_positions(n).items():
        other = (bits(hf[i:i + 1]) ^ np.uint16(1)).view(f16)[0]                           # the neighbouring fp16: one bit
        assert np.isfinite(other)
        keep = flat[i].clone()
        flat[i] = float(other)
        assert run(label) == 1, f"a change of {label} (index {i} of {n}) was missed"
        flat[i] = keep
    assert run("restored") == 0
    flat[1] = -0.0
    assert run("-0.0") == 1, "-0.0 against a cached +0.0 must raise the gate (bit compare)"
    note("ctx_compare", f"B {B} L {L} Lpad {Lpad} C {C} {np.dtype(dtype).name}", f"{n} elements; gate 0 when identical, 1 for one changed element at each of {list(ctx_positions(n))} and for -0.0")


def check_ctx_update_gated(be, B, L, Lpad, C, dtype):
    src = rnd((B, L, C), 610).astype(dtype)
    old = np.full((B, Lpad, C), FILL, f16)
    old[:, :L] = rnd((B, L, C), 611).astype(f16)
    g = Guarded((B, Lpad, C), torch.float16, be.dev)
    g.t.copy_(tt(old))
    gate = Guarded((1,), torch.int32, be.dev)
    gate.t.zero_()
    sd = dv(be, src)
    ok(be, be.ctx_update_gated(be.ptr(sd), code(src), be.ptr(g.t), B, L, Lpad, C, be.ptr(gate.t), be.sp()), "sdmi_ctx_update_gated")
    assert_bits(host(g.t), old, "ctx_update_gated with gate 0")
    gate.t.fill_(1)
    ok(be, be.ctx_update_gated(be.ptr(sd), code(src), be.ptr(g.t), B, L, Lpad, C, be.ptr(gate.t), be.sp()), "sdmi_ctx_update_gated")
    want = old.copy()
    want[:, :L] = src.astype(f16)
    assert_bits(host(g.t), want, "ctx_update_gated with gate 1")
    assert g.intact() and gate.intact() and int(gate.t.cpu()[0]) == 1
    note("ctx_update_gated", f"B {B} L {L} Lpad {Lpad} C {C} {np.dtype(dtype).name}", "gate 0: cache untouched; gate 1: fp16(src) in rows < L, rows L .. Lpad keep the sentinel")


# ---- hn_act / axpy_f16 -----------------------------------------------------------------------------------------------------------------------
HN_ACTS = {0: lambda x: x, 1: F.relu, 2: F.leaky_relu, 3: F.elu, 4: F.hardswish, 5: torch.tanh, 6: torch.sigmoid, 7: F.silu, 8: F.gelu, 9: F.mish,
           10: F.relu6, 11: F.selu, 12: F.softplus, 13: F.softsign, 14: F.hardtanh, 15: F.hardsigmoid}
HN_NAMES = {0: "identity", 1: "relu", 2: "leakyrelu", 3: "elu", 4: "hardswish", 5: "tanh", 6: "sigmoid", 7: "silu", 8: "gelu", 9: "mish", 10: "relu6",
            11: "selu", 12: "softplus", 13: "softsign", 14: "hardtanh", 15: "hardsigmoid"}
HN_MISMATCH_CAP, HN_GELU_MISMATCH_CAP = 317, 1000
_FINITE = {}


def finite_halves():
    """Every finite fp16 value (63,488 of them) and the float64 of each; computed once."""
    if not _FINITE:
        allb = np.arange(1 << 16, dtype=np.uint16).view(f16)
        x = allb[np.isfinite(allb)].copy()
        assert x.size == 63488
        _FINITE["x"], _FINITE["x64"] = x, torch.from_numpy(x.astype(np.float64))
    return _FINITE["x"], _FINITE["x64"]


def hn_launch(be, x, kind):
    g = Guarded(x.shape, torch.float16, be.dev)
    g.t.copy_(tt(x))
    ok(be, be.hn_act(be.ptr(g.t), x.size, kind, be.sp()), "sdmi_hn_act")
    assert g.intact()
    return host(g.t).copy()


def check_hn_act(be, kind):
    x, x64 = finite_halves()
    got = hn_launch(be, x, kind)
    ref = HN_ACTS[kind](x64).numpy()
    assert not np.isnan(got).any(), ("NaN from finite inputs", x[np.isnan(got)][:8])
    with np.errstate(over="ignore"):
        nearest = ref.astype(f16)
    mism = int((got != nearest).sum())
    g64 = got.astype(np.float64)
    if kind == 0:
        assert_bits(got, x, "hn_act kind 0 is the identity")
        note("hn_act", "0 identity", "bit-equal")
        return
    if kind == 8:
        bound = 0.5 * ulp16(ref) + 3 * np.abs(x.astype(np.float64)) * U
        err = np.abs(g64 - ref)
        worst = float((err / ulp16(ref)).max())
        note("hn_act", "8 gelu", f"{mism} of {x.size} inputs differ from fp16(float64) (cap {HN_GELU_MISMATCH_CAP}); worst |err| {worst:.3f} fp16 ulp, "
                                 f"worst |err| / bound {float((err / bound).max()):.4f} (cap 1)")
        assert (err <= bound).all(), ("first at v =", float(x[err > bound][0]), "worst multiple", float((err / bound).max()))
        assert mism <= HN_GELU_MISMATCH_CAP, mism
        return
    # the two fp16 neighbours of the float64 value (one value where it is exact in fp16)
    n64 = nearest.astype(np.float64)
    with np.errstate(over="ignore"):
        below = np.where(n64 <= ref, nearest, np.nextafter(nearest, f16(-np.inf)))
        above = np.where(n64 >= ref, nearest, np.nextafter(nearest, f16(np.inf)))
    bad = (got != below) & (got != above)
    note("hn_act", f"{kind} {HN_NAMES[kind]}", f"{mism} of {x.size} inputs differ from fp16(float64) (cap {HN_MISMATCH_CAP}); {int(bad.sum())} outside the two fp16 neighbours (cap 0)")
    assert not bad.any(), ("first at v =", float(x[bad][0]), "got", float(got[bad][0]), "float64", float(ref[bad][0]))
    assert mism <= HN_MISMATCH_CAP, mism


def check_hn_act_non_finite(be):
    """+inf, -inf and NaN in, the float64 function's own answer out (NaN for NaN)."""
    x = np.array([np.inf, -np.inf, np.nan], f16)
    for kind in range(16):
        got = hn_launch(be, x, kind)
        with np.errstate(all="ignore"):
            want = HN_ACTS[kind](torch.from_numpy(x.astype(np.float64))).numpy().astype(f16)
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (kind, HN_NAMES[kind], "inputs", x.tolist(), "got", got.tolist(), "float64 function", want.tolist())
    note("hn_act", "non-finite", "+inf, -inf, NaN through all 16 kinds: the float64 functions' answers")


def check_axpy_f16(be, n):
    x, h = rnd((n,), 700, 2.0).astype(f16), rnd((n,), 701, 3.0).astype(f16)
    a = f32(0.35)
    g = Guarded((n,), torch.float16, be.dev)
    ok(be, be.axpy_f16(be.ptr(g.t), be.ptr(dv(be, x)), be.ptr(dv(be, h)), float(a), n, be.sp()), "sdmi_axpy_f16")
    prod = a * h.astype(f32)
    want = (x.astype(f32) + prod).astype(f16)
    assert prod.dtype == f32
    assert_bits(host(g.t), want, f"axpy_f16 n {n}")
    assert g.intact()
    note("axpy_f16", f"n {n}", "bit-equal to fp16(fp32(x) + fp32(a * h))")


# ---- clip_embed / clip_pool ------------------------------------------------------------------------------------------------------------------
def check_clip_embed(be, dtype, embeds):
    B, L, C, vocab = 3, 77, 64, 50
    tok = rnd((vocab, C), 800).astype(dtype)
    pos = rnd((L, C), 801, 0.3)
    g = torch.Generator().manual_seed(802)
    tokens = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int32).numpy()
    tokens[0, 0], tokens[1, 5], tokens[2, 76], tokens[0, 76] = -1, vocab, vocab + 5, vocab - 1
    out = Guarded((B, L, C), torch.float16, be.dev)
    if embeds:
        ie = rnd((B, L, C), 803)
        garbage = np.full((B, L), 1 << 30, np.int32)
        garbage[0, 0] = -(1 << 30)
        ok(be, be.clip_embed(be.ptr(dv(be, garbage)), be.ptr(dv(be, tok)), code(tok), be.ptr(dv(be, pos)), be.ptr(dv(be, ie)), be.ptr(out.t), B, L, C, vocab,
                                    be.sp()), "sdmi_clip_embed")
        v = ie
    else:
        ok(be, be.clip_embed(be.ptr(dv(be, tokens)), be.ptr(dv(be, tok)), code(tok), be.ptr(dv(be, pos)), None, be.ptr(out.t), B, L, C, vocab, be.sp()),
           "sdmi_clip_embed")
        v = tok[np.clip(tokens, 0, vocab - 1)].astype(f32)
    want = (v + pos[None]).astype(f16)
    assert_bits(host(out.t), want, f"clip_embed {np.dtype(dtype).name} inputs_embeds {embeds}")
    assert out.intact()
    note("clip_embed", f"{np.dtype(dtype).name} table, inputs_embeds {embeds}", "bit-equal to fp16(fp32(tok) + pos); ids -1, vocab, vocab + 5 clamped")


def check_clip_pool(be, C):
    B, L = 4, 77
    hidden = rnd((B, L, C), 810).astype(f16)
    g = torch.Generator().manual_seed(811)
    tokens = torch.randint(0, 1000, (B, L), generator=g, dtype=torch.int32).numpy()
    tokens[0, 0] = 49407                                  # the maximum at position 0
    tokens[1, L - 1] = 49407                              # at L - 1
    tokens[2, 9] = tokens[2, 40] = 49407                  # duplicated: the first wins
    tokens[3] = 7                                         # all equal: position 0
    at = [0, L - 1, 9, 0]
    out = Guarded((B, C), torch.float32, be.dev)
    ok(be, be.clip_pool(be.ptr(dv(be, tokens)), be.ptr(dv(be, hidden)), be.ptr(out.t), B, L, C, be.sp()), "sdmi_clip_pool")
    want = np.stack([hidden[b, at[b]] for b in range(B)]).astype(f32)
    assert_bits(host(out.t), want, f"clip_pool C {C}")
    assert out.intact()
    note("clip_pool", f"C {C}", "the fp32 of the fp16 row at the first maximum (position 0, L - 1, duplicated, all equal)")


# ---- convert ---------------------------------------------------------------------------------------------------------------------------------
def convert_values(n, dtype):
    if dtype == f32:
        special = np.array([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 1.5 * 2.0 ** -20, -0.0, 70000.0, -1e6, 65520.0, 65519.996, -65520.0, 65504.0,
                            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -20), 1e-30, 3.0e38], f32)
    else:
        special = np.array([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 1023 * 2.0 ** -24, -0.0, 65504.0, -65504.0, np.inf, -np.inf, 1 + 2.0 ** -10], f16)
    body = rnd((max(n, special.size),), 900, 4.0).astype(dtype)
    body[:special.size] = special
    return np.roll(body, -3)[:n] if n < special.size else body[:n]


def check_convert(be, src_dtype, dst_dtype, n):
    x = convert_values(n, src_dtype)
    g = Guarded((n,), torch.float16 if dst_dtype == f16 else torch.float32, be.dev)
    ok(be, be.convert(be.ptr(dv(be, x)), code(x), be.ptr(g.t), F16 if dst_dtype == f16 else F32, n, be.sp()), "sdmi_convert")
    with np.errstate(over="ignore"):
        want = x.astype(dst_dtype)
    if n >= 32 and src_dtype == f32 and dst_dtype == f16:
        assert np.isinf(want).any() and (bits(want) == 0x8000).any() and ((want != 0) & (np.abs(want) < 2.0 ** -14)).any()
    assert_bits(host(g.t), want, f"convert {np.dtype(src_dtype).name} -> {np.dtype(dst_dtype).name} n {n}")
    assert g.intact()
    note("convert", f"{np.dtype(src_dtype).name} -> {np.dtype(dst_dtype).name} n {n}", "bit-equal to numpy")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _buf(be, shape, dtype, fill=FILL):
    return torch.full(shape, fill, dtype=dtype, device=be.dev)


def check_refusals(be, entry):
    L, p, sp = be, be.ptr, be.sp
    h16, h32, i32 = torch.float16, torch.float32, torch.int32
    if entry == "sdmi_small_linear":
        B, N, K = 2, 8, 16
        a, w, out = _buf(be, (B, K + 8), h32, 1.0), _buf(be, (N, K), h16, 1.0), _buf(be, (B, N + 4), h32)
        def call(a_=a, w_=w, out_=out, B_=B, N_=N, K_=K, lda=K, ldo=N):
            return L.small_linear(p(a_), p(w_), None, None, p(out_), B_, N_, K_, lda, ldo, 0, 0, sp())
        bad = [lambda: call(a_=None), lambda: call(w_=None), lambda: call(out_=None), lambda: call(B_=0), lambda: call(N_=-1), lambda: call(K_=0),
               lambda: call(K_=12, lda=12), lambda: call(lda=K + 2), lambda: call(lda=K - 4), lambda: call(ldo=N - 1),
               lambda: L.small_linear(p(a.view(-1)[1:]), p(w), None, None, p(out), B, N, K, K, N, 0, 0, sp())]
        outs = [out]
    elif entry == "sdmi_silu_f32":
        x, y = _buf(be, (8,), h32, 1.0), _buf(be, (8,), h32)
        bad = [lambda: L.silu_f32(None, p(y), 8, sp()), lambda: L.silu_f32(p(x), None, 8, sp()), lambda: L.silu_f32(p(x), p(y), 0, sp()),
               lambda: L.silu_f32(p(x), p(y), -8, sp())]
        outs = [y]
    elif entry == "sdmi_timestep_embedding":
        t, out = _buf(be, (2,), h32, 1.0), _buf(be, (2, 8), h32)
        bad = [lambda: L.timestep_embedding(None, F32, p(out), 2, 8, sp()), lambda: L.timestep_embedding(p(t), F32, None, 2, 8, sp()),
               lambda: L.timestep_embedding(p(t), F32, p(out), 0, 8, sp()), lambda: L.timestep_embedding(p(t), F32, p(out), 2, 0, sp()),
               lambda: L.timestep_embedding(p(t), F32, p(out), 2, 1, sp()), lambda: L.timestep_embedding(p(t), F32, p(out), 2, -8, sp()),
               lambda: L.timestep_embedding(p(t), 2, p(out), 2, 8, sp()), lambda: L.timestep_embedding(p(t), -1, p(out), 2, 8, sp())]
        outs = [out]
    elif entry == "sdmi_nchw_to_nhwc":
        B, C, HW, cpad = 1, 4, 6, 8
        x, out, mw = _buf(be, (B, 17, HW), h32, 1.0), _buf(be, (B, HW, 64), h16), _buf(be, (C, C), h32, 1.0)
        def call(x_=x, dt=F32, out_=out, B_=B, C_=C, HW_=HW, cpad_=cpad, mw_=None, mb_=None, lo=0):
            return L.nchw_to_nhwc(p(x_), dt, p(out_), B_, C_, HW_, cpad_, 1.0, p(mw_), p(mb_), lo, sp())
        bad = [lambda: call(x_=None), lambda: call(out_=None), lambda: call(B_=0), lambda: call(C_=0), lambda: call(HW_=-1), lambda: call(C_=17, cpad_=64),
               lambda: call(cpad_=3), lambda: call(lo=1, cpad_=7), lambda: call(lo=1, cpad_=4), lambda: call(lo=1, mw_=mw), lambda: call(mb_=mw),
               lambda: call(dt=2), lambda: call(dt=-1)]
        outs = [out]
    elif entry == "sdmi_add_nchw_residual":
        B, C, HW = 1, 8, 4
        src, lo, ctrl, dst, dlo = _buf(be, (B, HW, 16), h16, 1.0), _buf(be, (B, HW, 16), h16, 1.0), _buf(be, (B, 16, HW), h32, 1.0), _buf(be, (B, HW, 16), h16), \
            _buf(be, (B, HW, 16), h16)
        def call(s=src, sl=None, c=ctrl, dt=F32, d=dst, dl=None, B_=B, C_=C, HW_=HW):
            return L.add_nchw_residual(p(s), p(sl), p(c), dt, p(d), p(dl), B_, C_, HW_, sp())
        bad = [lambda: call(s=None), lambda: call(c=None), lambda: call(d=None), lambda: call(B_=0), lambda: call(C_=0), lambda: call(HW_=0), lambda: call(C_=12),
               lambda: call(C_=4), lambda: call(sl=lo), lambda: call(dl=dlo), lambda: call(dt=3), lambda: call(dt=-1)]
        outs = [dst, dlo]
    elif entry in ("sdmi_ctx_compare", "sdmi_ctx_update_gated"):
        B, Ln, Lpad, C = 2, 4, 8, 8
        src, cached, gate = _buf(be, (B, Lpad, C), h32, 1.0), _buf(be, (B, Lpad, C), h16), _buf(be, (1,), i32)
        fn = getattr(be, entry[len("sdmi_"):])
        def call(s=src, dt=F32, c=cached, B_=B, L_=Ln, Lp=Lpad, C_=C, g=gate):
            return fn(p(s), dt, p(c), B_, L_, Lp, C_, p(g), sp())
        bad = [lambda: call(s=None), lambda: call(c=None), lambda: call(g=None), lambda: call(B_=0), lambda: call(L_=0), lambda: call(C_=-8), lambda: call(Lp=3),
               lambda: call(L_=9), lambda: call(dt=2), lambda: call(dt=-1)]
        outs = [cached, gate]
    elif entry == "sdmi_hn_act":
        x = _buf(be, (16,), h16)
        bad = [lambda: L.hn_act(None, 16, 1, sp()), lambda: L.hn_act(p(x), 0, 1, sp()), lambda: L.hn_act(p(x), -16, 1, sp()),
               lambda: L.hn_act(p(x), 16, 16, sp()), lambda: L.hn_act(p(x), 16, -1, sp()), lambda: L.hn_act(p(x), 16, 1 << 20, sp())]
        outs = [x]
    elif entry == "sdmi_axpy_f16":
        y, x, h = _buf(be, (16,), h16), _buf(be, (16,), h16, 1.0), _buf(be, (16,), h16, 1.0)
        bad = [lambda: L.axpy_f16(None, p(x), p(h), 0.5, 16, sp()), lambda: L.axpy_f16(p(y), None, p(h), 0.5, 16, sp()),
               lambda: L.axpy_f16(p(y), p(x), None, 0.5, 16, sp()), lambda: L.axpy_f16(p(y), p(x), p(h), 0.5, 0, sp()),
               lambda: L.axpy_f16(p(y), p(x), p(h), 0.5, -1, sp())]
        outs = [y]
    elif entry == "sdmi_clip_embed":
        B, Ln, C, vocab = 1, 4, 8, 5
        tokens, tok, pos, ie, out = torch.zeros((B, Ln), dtype=i32, device=be.dev), _buf(be, (vocab, C), h32, 1.0), _buf(be, (Ln, C), h32, 1.0), \
            _buf(be, (B, Ln, C), h32, 1.0), _buf(be, (B, Ln, C), h16)
        def call(t=tokens, e=tok, dt=F32, ps=pos, i=None, o=out, B_=B, L_=Ln, C_=C, v=vocab):
            return L.clip_embed(p(t), p(e), dt, p(ps), p(i), p(o), B_, L_, C_, v, sp())
        bad = [lambda: call(t=None), lambda: call(e=None), lambda: call(ps=None), lambda: call(o=None), lambda: call(B_=0), lambda: call(L_=0), lambda: call(C_=0),
               lambda: call(v=0), lambda: call(v=-3), lambda: call(i=ie, v=0), lambda: call(dt=2), lambda: call(dt=-1)]
        outs = [out]
    elif entry == "sdmi_clip_pool":
        B, Ln, C = 1, 4, 8
        tokens, hid, out = torch.zeros((B, Ln), dtype=i32, device=be.dev), _buf(be, (B, Ln, C), h16, 1.0), _buf(be, (B, C), h32)
        bad = [lambda: L.clip_pool(None, p(hid), p(out), B, Ln, C, sp()), lambda: L.clip_pool(p(tokens), None, p(out), B, Ln, C, sp()),
               lambda: L.clip_pool(p(tokens), p(hid), None, B, Ln, C, sp()), lambda: L.clip_pool(p(tokens), p(hid), p(out), 0, Ln, C, sp()),
               lambda: L.clip_pool(p(tokens), p(hid), p(out), B, 0, C, sp()), lambda: L.clip_pool(p(tokens), p(hid), p(out), B, Ln, -1, sp())]
        outs = [out]
    elif entry == "sdmi_convert":
        x, y = _buf(be, (16,), h32, 1.0), _buf(be, (16,), h32)
        bad = [lambda: L.convert(None, F32, p(y), F32, 16, sp()), lambda: L.convert(p(x), F32, None, F32, 16, sp()),
               lambda: L.convert(p(x), F32, p(y), F32, 0, sp()), lambda: L.convert(p(x), F32, p(y), F32, -16, sp()),
               lambda: L.convert(p(x), 2, p(y), F32, 16, sp()), lambda: L.convert(p(x), F32, p(y), -1, 16, sp()), lambda: L.convert(p(x), F16, p(y), 5, 16, sp())]
        outs = [y]
    else:
        raise AssertionError(entry)
    for n, call_bad in enumerate(bad):
        rc = call_bad()
        assert rc != 0, (entry, "refusal", n, "was accepted")
        msg = be.last_error()
        assert entry in msg and len(msg) > len(entry) + 8, (entry, n, msg)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.cpu() == FILL).all()), (entry, "a refused call stored something")
    note("refusals", entry, f"{len(bad)} bad calls refused on the host, outputs untouched")


ENTRIES = ["sdmi_small_linear", "sdmi_silu_f32", "sdmi_timestep_embedding", "sdmi_nchw_to_nhwc", "sdmi_add_nchw_residual", "sdmi_ctx_compare",
           "sdmi_ctx_update_gated", "sdmi_hn_act", "sdmi_axpy_f16", "sdmi_clip_embed", "sdmi_clip_pool", "sdmi_convert"]
