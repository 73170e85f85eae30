"""GPU parity tests of the compact Real-ESRGAN path (SRVGGNetCompact): the compact_conv kernel through sdmi_compact_conv against
F.conv2d, whole networks through sdmi_compact_run, UpscalerESRGAN.do_upscale on a compact checkpoint and one hires-fix job, against
tests/compact_reference.py (fp32, CPU).

Comparison rule: that of tests/test_gpu_esrgan.py (`assert_parity`): the yardstick is the distance of the fp16-storage twin from the fp32
reference; the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per output channel, per image row)
within 2 x that, and the yardstick itself is asserted above 1e-4.  Networks are compared on their RESIDUAL, out - nearest_upsample(x, r):
the output is the input image plus a small correction, so the output's own rel_l2 is dominated by the last rounding of the sum and barely
moves with the body.  Every case also runs on the host-emulated library (tests/test_cpu_compact.py)."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import compact_reference as R
from fp16_emu import r16
from helpers import rel_l2, seeded, worst_slice_rel_l2

pytestmark = pytest.mark.gpu


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


def assert_parity(got, ref, twin, channel_dim, row_dims, ctx=None):
    got, ref, twin = got.float().cpu(), ref.float(), twin.float()
    yard = rel_l2(twin, ref)
    err = rel_l2(got, ref)
    print(f"[compact parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
    assert yard > 1e-4, (ctx, yard)
    assert err <= 1.25 * yard, (ctx, err, yard)
    for keep in ((channel_dim,), row_dims):
        worst, idx = worst_slice_rel_l2(got, ref, keep)
        assert worst <= 2 * 1.25 * yard, (ctx, "slices over dims", keep, "worst at", idx, worst, yard)


def conv_case(dev, b, h, w, real_cin, seed, lda=None, nout=64, w_scale=None, poison=1e4):
    """Seeded NHWC input [b, h, w, lda]: real_cin channels of data, zeros up to the kernel's cin (32 | 64), 1e4 in the excess; weight
    [nout, real_cin, 3, 3], bias; the packed weight and the 64-padded bias on the device.  Everything fp16-rounded where the kernel
    reads fp16."""
    ops = sub("ops")
    cin = 32 if real_cin <= 32 else 64
    lda = lda or cin
    x = torch.full((b, h, w, lda), poison, dtype=torch.float32)
    x[..., :cin] = 0
    x[..., :real_cin] = seeded((b, h, w, real_cin), seed)
    wt = seeded((nout, real_cin, 3, 3), seed + 1, w_scale or (real_cin * 9) ** -0.5)
    bias = seeded((nout,), seed + 2, 0.1)
    wp = ops.pack_compact_weight(wt.to(dev))
    assert wp.shape == (64, 9, cin)
    bp = torch.zeros(64, dtype=torch.float32)
    bp[:nout] = bias
    return x.half().float(), wt.half().float(), bias, x.half().to(dev), wp, bp.to(dev)


def ref_conv(x, w, bias, real_cin):
    return F.conv2d(x[..., :real_cin].permute(0, 3, 1, 2), w, bias, padding=1).permute(0, 2, 3, 1)           # NHWC


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


# ---- op level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real_cin,lda", [(64, 72), (3, 40)])
def test_compact_conv_reads_cin_channels_of_wider_rows(dev, real_cin, lda):
    """cin 64, and cin 32 with 3 real channels (the first layer), B = 2, 12 x 20; the input rows are wider than cin and the excess holds 1e4."""
    ops = sub("ops")
    x, w, bias, xd, wp, bp = conv_case(dev, 2, 12, 20, real_cin, 100 + real_cin, lda=lda)
    got = ops.compact_conv(xd, wp, bp, ep="none")
    assert got.shape == (2, 12, 20, 64) and got.dtype == torch.float16
    ref = ref_conv(x, w, bias, real_cin)
    assert_parity(got, ref, r16(ref), 3, (0, 1), f"cin {real_cin} in rows of {lda}")


def test_compact_conv_prelu_has_one_slope_per_channel(dev):
    ops = sub("ops")
    x, w, bias, xd, wp, bp = conv_case(dev, 1, 12, 20, 64, 200)
    slope = torch.linspace(-0.3, 1.2, 64)
    slope[5], slope[17], slope[40] = 0.0, 1.0, -0.5
    assert len(set(slope.tolist())) == 64
    pre = ref_conv(x, w, bias, 64)
    assert bool((pre.amax(dim=(0, 1, 2)) > 0).all()) and bool((pre.amin(dim=(0, 1, 2)) < 0).all())         # both signs in every channel
    got = ops.compact_conv(xd, wp, bp, slope=slope.to(dev), ep="prelu")
    ref = F.prelu(pre.permute(0, 3, 1, 2), slope).permute(0, 2, 3, 1)
    assert_parity(got, ref, r16(ref), 3, (0, 1), "PReLU, 64 slopes")
    none = ops.compact_conv(xd, wp, bp, ep="none")
    assert same_bits(got[..., 17], none[..., 17]) and not same_bits(got[..., 5], none[..., 5])             # slope 1 is the identity


GEOMETRY = [(12, 20), (17, 13), (33, 35)]       # lower than a tile and ragged in x | one row over a tile edge | 9 tiles, the middle one interior


@pytest.mark.parametrize("h,w", GEOMETRY)
def test_compact_conv_tile_geometry(dev, h, w):
    ops = sub("ops")
    x, wt, bias, xd, wp, bp = conv_case(dev, 1, h, w, 64, 300 + h)
    slope = (seeded((64,), 7, 0.2) + 0.25).float()
    out = torch.full((1, h, w, 72), 3.0, dtype=torch.float16).to(dev)              # ldo 72: the 8 channels past n_real keep their bits
    got = ops.compact_conv(xd, wp, bp, slope=slope.to(dev), ep="prelu", out=out)
    assert got is out and bool((out.cpu()[..., 64:] == 3).all())
    ref = F.prelu(ref_conv(x, wt, bias, 64).permute(0, 3, 1, 2), slope).permute(0, 2, 3, 1)
    assert_parity(out[..., :64], ref, r16(ref), 3, (0, 1), f"{h}x{w}")


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_compact_conv_capped_grid_walks_tiles_through_both_halo_slots(dev, cap):
    """B = 2 x 33 x 35 = 18 tiles on 1, 2, 3 workgroups: each walks 18 / 9 / 6 tiles, alternating the two halo slots and crossing the
    image boundary (tile 9 is the first of image 1).  Bit-equal to the uncapped launch (a tile's arithmetic does not depend on who runs it)."""
    ops = sub("ops")
    x, wt, bias, xd, wp, bp = conv_case(dev, 2, 33, 35, 64, 400)
    slope = (seeded((64,), 8, 0.2) + 0.25).float().to(dev)
    full = ops.compact_conv(xd, wp, bp, slope=slope, ep="prelu")
    capped = ops.compact_conv(xd, wp, bp, slope=slope, ep="prelu", grid_cap=cap)
    assert same_bits(capped, full)
    if cap == 1:
        ref = F.prelu(ref_conv(x, wt, bias, 64).permute(0, 3, 1, 2), slope.cpu()).permute(0, 2, 3, 1)
        assert_parity(capped, ref, r16(ref), 3, (0, 1), "B2 33x35 on one workgroup")


@pytest.mark.parametrize("cin", [32, 64])
def test_compact_conv_border_tap_counts_are_exact(dev, cin):
    """All-ones input and weights: an output pixel equals (taps inside the image) x cin — 4 at corners, 6 on edges, 9 inside — exactly
    (a halo pixel that did not come from the zero page, or a stale one from the other slot, would show).  17 x 19: 4 tiles."""
    ops = sub("ops")
    xd = torch.ones((2, 17, 19, cin), dtype=torch.float16).to(dev)
    wp = ops.pack_compact_weight(torch.ones((64, cin, 3, 3)).to(dev))
    got = ops.compact_conv(xd, wp, None, ep="none", grid_cap=2).cpu().float()
    taps = F.conv2d(torch.ones(1, 1, 17, 19), torch.ones(1, 1, 3, 3), padding=1)[0, 0]
    assert sorted(set(taps.flatten().tolist())) == [4.0, 6.0, 9.0]
    assert torch.equal(got, (taps * cin)[None, :, :, None].expand(2, 17, 19, 64))


@pytest.mark.parametrize("r,h,w", [(1, 16, 24), (2, 12, 20), (3, 9, 11), (4, 17, 13)])
def test_compact_conv_tail_shuffles_adds_the_input_and_stores(dev, r, h, w):
    """The last launch: 3 r^2 channels -> pixel shuffle + nearest-upsampled network input, fp32 NCHW and uint8 HWC stores, with the input
    given as uint8 HWC and as fp32 NCHW (the same image)."""
    ops, up = sub("ops"), sub("upscaler")
    x, wt, bias, xd, wp, bp = conv_case(dev, 2, h, w, 64, 500 + r, nout=3 * r * r, w_scale=0.012)
    img8 = torch.from_numpy(np.random.RandomState(r).randint(0, 256, size=(2, h, w, 3), dtype=np.uint8))
    img32 = (img8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    conv = ref_conv(x, wt, bias, 64).permute(0, 3, 1, 2)
    shuffled = F.pixel_shuffle(conv, r)
    base = F.interpolate(img32, scale_factor=r, mode="nearest")
    ref = shuffled + base
    f32 = ops.compact_conv(xd, wp, bp, ep="tail", r=r, base=img8.to(dev), store="f32_nchw")
    assert f32.shape == (2, 3, h * r, w * r) and f32.dtype == torch.float32
    assert_parity(f32.cpu() - base, shuffled, r16(shuffled), 1, (0, 2), f"tail x{r} fp32 store (minus the base)")
    assert rel_l2(f32.cpu(), ref) < 1e-5                                        # no fp16 store in this form: fp32 accumulation error only
    from_f32 = ops.compact_conv(xd, wp, bp, ep="tail", r=r, base=img32.to(dev), store="f32_nchw")
    assert rel_l2(from_f32.cpu(), ref) < 1e-5 and float((from_f32 - f32).abs().max()) < 1e-6
    for src in (img8, img32):
        u8 = ops.compact_conv(xd, wp, bp, ep="tail", r=r, base=src.to(dev), store="u8_hwc")
        assert u8.shape == (2, h * r, w * r, 3) and u8.dtype == torch.uint8
        want = up.model_output_to_u8((f32 if src is img8 else from_f32).cpu().permute(0, 2, 3, 1).numpy())
        assert np.array_equal(u8.cpu().numpy(), want)                              # the same sums through clamp, x255, round-half-even
    assert 0.02 < (want == 0).mean() + (want == 255).mean() < 0.9                  # the clamp is exercised, and so is the interior


def test_compact_conv_refuses_what_it_is_not_built_for(dev):
    ops, _lib = sub("ops"), sub("_lib")
    z = lambda *s: torch.zeros(s, dtype=torch.float16).to(dev)
    x64, w64 = z(1, 4, 4, 64), z(64, 9, 64)
    with pytest.raises(_lib.SdmiError, match="32 or 64 input channels"):
        ops.compact_conv(z(1, 4, 4, 96), z(64, 9, 96), None, ep="none")
    with pytest.raises(_lib.SdmiError, match="stride >= cin"):
        ops.compact_conv(z(1, 4, 4, 32), w64, None, ep="none")                      # rows narrower than cin
    with pytest.raises(_lib.SdmiError, match="stride >= cin, 16-byte aligned"):
        ops.compact_conv(z(1, 4, 4, 68), w64, None, ep="none")                      # 136-byte rows
    with pytest.raises(_lib.SdmiError, match="fp16 output rows"):
        ops.compact_conv(x64, w64, None, ep="none", out=z(1, 4, 4, 66))             # 132-byte rows
    with pytest.raises(_lib.SdmiError, match="fp16 output rows"):
        ops.compact_conv(x64, w64, None, ep="none", n_real=64, out=z(1, 4, 4, 32))  # rows narrower than n_real
    with pytest.raises(_lib.SdmiError, match="PReLU needs"):
        ops.compact_conv(x64, w64, None, ep="prelu")
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8).to(dev)
    with pytest.raises(_lib.SdmiError, match="scale r in 1..4"):
        ops.compact_conv(x64, w64, None, ep="tail", r=5, base=img)
    with pytest.raises(_lib.SdmiError, match="n_real = 3 r\\^2"):
        ops.compact_conv(x64, w64, None, ep="tail", r=2, n_real=3, base=img)
    with pytest.raises(_lib.SdmiError, match="network's input"):
        ops.compact_conv(x64, w64, None, ep="tail", r=2)
    # in-place: refused before anything is launched (the input keeps its bits)
    xin = torch.ones((1, 20, 20, 64), dtype=torch.float16).to(dev)
    with pytest.raises(_lib.SdmiError, match="in-place"):
        ops.compact_conv(xin, torch.ones((64, 9, 64), dtype=torch.float16).to(dev), None, ep="none", out=xin)
    assert bool((xin.cpu() == 1).all())
    # B H W at 2^31 - 256: the descriptor alone (the buffers are never touched)
    d = _lib.CompactDesc()
    d.in_, d.w, d.out = x64.data_ptr(), w64.data_ptr(), z(1, 4, 4, 64).data_ptr()
    d.cin, d.lda, d.ldo, d.n_real, d.ep = 64, 64, 64, 64, _lib.COMPACT_EP_NONE
    for b, h, w in ((128, 4096, 4096), (1, 256, 8388607)):                          # 2^31, and the bound itself: 2^31 - 256
        d.B, d.H, d.W = b, h, w
        assert b * h * w >= (1 << 31) - 256
        assert _lib.lib.sdmi_compact_conv(d, None) != 0 and "below 2^31" in _lib.last_error()


# ---- network level ----------------------------------------------------------------------------------------------------------------
NETS = {}


def net_for(num_conv, scale):
    key = (num_conv, scale)
    if key not in NETS:
        sd = R.make_state_dict(num_conv, scale)
        NETS[key] = (sd, sub("upscaler").CompactNet(sd, device=0))
    return NETS[key]


def residual_parity(got, sd, x, ctx):
    base = R.base(sd, x)
    assert_parity(got.cpu() - base, R.forward(sd, x) - base, R.fp16_twin(sd, x) - base, 1, (0, 2), ctx)


@pytest.mark.parametrize("num_conv,scale,b,h,w", [(4, 4, 2, 12, 20), (16, 4, 1, 17, 13), (4, 2, 1, 12, 20), (4, 3, 1, 9, 11),
                                                  (4, 1, 1, 16, 24), (32, 4, 1, 33, 35)])
def test_compact_network_vs_reference(dev, num_conv, scale, b, h, w):
    sd, net = net_for(num_conv, scale)
    assert (net.num_conv, net.scale) == (num_conv, scale)
    x = R.image(b, h, w, 10 + scale)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * scale, w * scale) and got.dtype == torch.float32
    m = b * h * w                                                # the padded input and two 64-wide buffers, all at the input resolution
    assert m * (32 + 2 * 64) * 2 <= net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    residual_parity(got, sd, x, f"num_conv {num_conv} x{scale} {b}x{h}x{w} residual")
    if num_conv == 4 and scale == 4:                           # the uint8 input is the same image: the same output
        x8 = torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        assert float((net.run(x8.to(dev)).cpu() - got.cpu()).abs().max()) < 1e-6


def test_compact_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_compact_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB)."""
    engine = sub("engine").Engine(0)
    net = sub("upscaler").CompactNet(R.make_state_dict(4, 4), device=0, engine=engine)
    b, h, w = 2, 12, 20
    assert engine.arena_bytes() == 0
    got = net.run(R.image(b, h, w, 14).to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, 4 * h, 4 * w) and b * h * w * (32 + 2 * 64) * 2 <= n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


def test_compact_network_under_the_training_wrapper(dev):
    up = sub("upscaler")
    sd, net = net_for(4, 4)
    wrapped = up.CompactNet({"params_ema": sd, "params": R.make_state_dict(4, 4, seed=9)}, device=0, engine=net.engine)
    x = R.image(1, 17, 13, 31).to(dev)
    assert torch.equal(wrapped.run(x).cpu(), net.run(x).cpu())
    wrapped.close()


# ---- the scaler object ------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_compact_checkpoint(dev, tmp_path):
    """do_upscale on a compact .pth: a PIL image of the right size from one cached net; against the fp32 reference's uint8 image the share
    of differing bytes is at most 1.25 x the share the fp16-storage twin shows, the largest level difference no more than the twin's
    (floor 1) — the conditions of the ESRGAN test.
    Measured on the MI355X (profiles/compact_parity.md): engine 2.6476 % of bytes differ, twin 3.4549 %; largest level difference 1 and 1."""
    from PIL import Image
    up = sub("upscaler")
    sd = R.make_state_dict(4, 4)
    path = str(tmp_path / "tiny_compact_x4.pth")
    torch.save({"params": sd}, path)
    src = np.random.RandomState(5).randint(90, 166, size=(12, 20, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0)
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (80, 48) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.CompactNet)
    assert scaler.do_upscale(Image.fromarray(src), path).size == (80, 48) and len(scaler._nets) == 1
    x = torch.from_numpy(src.astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    ref = up.model_output_to_u8(R.forward(sd, x)[0].permute(1, 2, 0).numpy()).astype(np.int32)
    twin = up.model_output_to_u8(R.fp16_twin(sd, x)[0].permute(1, 2, 0).numpy()).astype(np.int32)
    got = np.asarray(img).astype(np.int32)
    share, twin_share = float((got != ref).mean()), float((twin != ref).mean())
    worst, twin_worst = int(np.abs(got - ref).max()), int(np.abs(twin - ref).max())
    print(f"[compact parity] do_upscale: differing bytes engine {share:.4%} twin {twin_share:.4%}; largest level difference engine {worst} twin {twin_worst}")
    assert ((ref == 0) | (ref == 255)).mean() < 0.05
    assert share <= 1.25 * twin_share, (share, twin_share)
    assert worst <= max(twin_worst, 1), (worst, twin_worst)


# ---- one job ----------------------------------------------------------------------------------------------------------------------
def test_hires_fix_job_with_a_registered_compact_upscaler(dev, tmp_path, monkeypatch):
    """txt2img with enable_hr, hr_scale = 2 and a registered compact x4 entry as hr_upscaler: the engine's job against the same job with
    the scaler's network replaced by the torch reference module in fp32 (test_hires_fix_job_with_a_registered_esrgan_upscaler with a
    compact checkpoint; the same tiny model and the same cap)."""
    from PIL import Image
    schema, processing, shared, up = sub("schema"), sub("processing"), sub("shared"), sub("upscaler")
    sd = R.make_state_dict(2, 4)
    path = str(tmp_path / "tiny_compact_x4.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae(ch_mult=(1, 1, 2, 2))
    model = sub("sd_models").SdModel(schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0x77), ucfg, vcfg, device=0)
    added = up.register_esrgan({"Tiny-Compact 4x": path}, engine=model.engine)          # one engine, one arena: UNet, VAE and upscaler
    assert added[0].scaler.engine is model.engine
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-Compact 4x"] and added[0].scale == 4
    g = torch.Generator().manual_seed(14)
    cond, uncond = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)

    def job():
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=3300, batch_size=1, steps=2, cfg_scale=5.0,
                                                        width=32, height=32, sampler_name="Euler a", enable_hr=True, hr_scale=2.0,
                                                        denoising_strength=0.6, hr_upscaler="Tiny-Compact 4x")
        return processing.process_images(p)
    res = job()
    assert res.latents.shape == (1, 4, 8, 8) and res.images[0].shape == (64, 64, 3)
    assert isinstance(added[0].scaler._nets[path], up.CompactNet)
    module = R.CompactModule(sd)

    def torch_do_upscale(img, selected_model=None):
        x = torch.from_numpy(np.asarray(img.convert("RGB")).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
        return Image.fromarray(up.model_output_to_u8(module(x)[0].permute(1, 2, 0).numpy()))
    monkeypatch.setattr(added[0].scaler, "do_upscale", torch_do_upscale)
    want = job()
    assert rel_l2(res.latents.cpu(), want.latents.cpu()) < 2e-2
