"""GPU parity tests of the RRDBNet (ESRGAN / Real-ESRGAN) path: the rrdb_conv kernel through sdmi_rrdb_conv against F.conv2d, whole
networks through sdmi_esrgan_run, UpscalerESRGAN.do_upscale and one hires-fix job, against tests/rrdb_reference.py (fp32, CPU).

Comparison rule (the project's: teacher_forcing.py, test_gpu_ops.py): the yardstick is the distance of the fp16-storage twin (same
arithmetic, every written tensor rounded to binary16) from the fp32 reference; the engine's rel_l2 from the same reference stays within
1.25 x the yardstick, every slice (per output channel, per image row) within 2 x that, and the yardstick itself is asserted above 1e-4
so that the comparison cannot pass vacuously.  Every case also runs on the host-emulated library (tests/test_cpu_esrgan.py)."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrdb_reference as R
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
    print(f"[esrgan parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
    assert yard > 1e-4, (ctx, yard)
    assert err <= 1.25 * yard, (ctx, err, yard)
    for keep in ((channel_dim,), row_dims):
        worst, idx = worst_slice_rel_l2(got, ref, keep)
        assert worst <= 2 * 1.25 * yard, (ctx, "slices over dims", keep, "worst at", idx, worst, yard)


def conv_case(dev, b, hi, wi, cin, nout, seed, lda=None, poison=1e4, w_scale=None, real_cin=None):
    """Seeded input buffer [b, hi, wi, lda] (channels >= cin poisoned), weight / bias, and the packed weight."""
    ops = sub("ops")
    lda = lda or cin
    real_cin = real_cin or cin
    x = torch.full((b, hi, wi, lda), poison, dtype=torch.float32)
    x[..., :cin] = 0
    x[..., :real_cin] = seeded((b, hi, wi, real_cin), seed)
    w = seeded((nout, real_cin, 3, 3), seed + 1, w_scale or (real_cin * 9) ** -0.5)
    bias = seeded((nout,), seed + 2, 0.1)
    xd = x.half().to(dev)
    wp = ops.pack_rrdb_weight(w.to(dev), 32 if nout <= 32 else 64)
    bp = torch.zeros(wp.shape[0], dtype=torch.float32)
    bp[:nout] = bias
    return x.half().float(), w.half().float(), bias, xd, wp, bp.to(dev)


def ref_conv(x, w, bias, cin, up=False):
    t = x[..., :cin].permute(0, 3, 1, 2)
    if up:
        t = F.interpolate(t, scale_factor=2, mode="nearest")
    return F.conv2d(t, w, bias, padding=1).permute(0, 2, 3, 1)            # NHWC


# ---- op level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [64, 96, 128, 160, 192])
def test_rrdb_conv_reads_a_channel_prefix_and_writes_its_slot(dev, cin):
    """B = 2, 12 x 20: 240 pixels per image against the 256-pixel tile, so the first tile straddles the two images.  The input is the
    first cin channels of a 192-stride buffer whose other channels hold 1e4; the 32 outputs land at channel offset cin of a 224-wide
    buffer whose other channels must keep their bits."""
    ops = sub("ops")
    x, w, bias, xd, wp, bp = conv_case(dev, 2, 12, 20, cin, 32, 100 + cin, lda=192)
    out = seeded((2, 12, 20, 224), 7).half().to(dev)
    before = out.clone()
    got = ops.rrdb_conv(xd, wp, bp, cin=cin, out=out, out_offset=cin, ep="lrelu")
    assert got is out
    ref = F.leaky_relu(ref_conv(x, w, bias, cin), 0.2)
    assert_parity(out[..., cin:cin + 32], ref, r16(ref), 3, (0, 1), f"prefix cin={cin}")
    keep = torch.ones(224, dtype=torch.bool)
    keep[cin:cin + 32] = False
    assert torch.equal(out.cpu()[..., keep].view(torch.int16), before.cpu()[..., keep].view(torch.int16))
    if cin < 192:                                            # the dense block's own use: the slot is in the buffer that is being read
        ops.rrdb_conv(xd, wp, bp, cin=cin, out=xd, out_offset=cin, ep="lrelu")
        assert torch.equal(xd[..., cin:cin + 32].cpu().view(torch.int16), out[..., cin:cin + 32].cpu().view(torch.int16))
        assert torch.equal(xd[..., :cin].cpu().float(), x[..., :cin])


@pytest.mark.parametrize("ep", ["res1", "res2"])
def test_rrdb_conv_residual_epilogues(dev, ep):
    ops = sub("ops")
    x, w, bias, xd, wp, bp = conv_case(dev, 2, 12, 20, 192, 64, 300)
    r1 = seeded((2, 12, 20, 192), 301).half()
    r2 = seeded((2, 12, 20, 72), 302).half()                # distinct row strides: ldr1 = 192, ldr2 = 72
    conv = ref_conv(x, w, bias, 192)
    if ep == "res1":
        got = ops.rrdb_conv(xd, wp, bp, ep="res1", alpha=0.2, r1=r1.to(dev))
        ref = conv * 0.2 + r1.float()[..., :64]
        twin = r16(r16(conv) * 0.2 + r1.float()[..., :64])
    else:
        got = ops.rrdb_conv(xd, wp, bp, ep="res2", alpha=0.2, r1=r1.to(dev), beta=0.2, r2=r2.to(dev))
        ref = (conv * 0.2 + r1.float()[..., :64]) * 0.2 + r2.float()[..., :64]
        twin = r16(r16(r16(conv) * 0.2 + r1.float()[..., :64]) * 0.2 + r2.float()[..., :64])
    assert got.shape == (2, 12, 20, 64)
    assert_parity(got, ref, twin, 3, (0, 1), ep)


@pytest.mark.parametrize("up", [False, True])
def test_rrdb_conv_odd_ragged_image_and_fused_x2_gather(dev, up):
    """17 x 13 (221 pixels: one ragged tile); with the gather 7 x 9 -> 14 x 18."""
    ops = sub("ops")
    hi, wi = (7, 9) if up else (17, 13)
    x, w, bias, xd, wp, bp = conv_case(dev, 1, hi, wi, 64, 64, 400 + up)
    got = ops.rrdb_conv(xd, wp, bp, ep="lrelu", up=up)
    ref = F.leaky_relu(ref_conv(x, w, bias, 64, up=up), 0.2)
    assert got.shape == ((1, 14, 18, 64) if up else (1, 17, 13, 64))
    assert_parity(got, ref, r16(ref), 3, (0, 1), f"ragged up={up}")


def test_rrdb_conv_first_padded_input_channels(dev):
    ops = sub("ops")
    x, w, bias, xd, wp, bp = conv_case(dev, 2, 12, 20, 32, 64, 500, real_cin=3)
    assert wp.shape == (64, 9, 32)
    got = ops.rrdb_conv(xd, wp, bp, ep="none")
    ref = ref_conv(x, w, bias, 3)
    assert_parity(got, ref, r16(ref), 3, (0, 1), "conv_first 3 -> 32")


def test_rrdb_conv_last_three_real_channels_in_every_store_form(dev):
    ops, up = sub("ops"), sub("upscaler")
    x, w, bias, xd, wp, bp = conv_case(dev, 2, 12, 20, 64, 3, 600, w_scale=0.02)
    bp[:3] += 0.5
    bias = bias + 0.5
    assert wp.shape == (32, 9, 64)
    ref = ref_conv(x, w, bias, 64)                           # NHWC [2, 12, 20, 3]
    out = torch.full((2, 12, 20, 8), 3.0, dtype=torch.float16).to(dev)
    ops.rrdb_conv(xd, wp, bp, out=out, out_offset=4, n_real=3, ep="none")
    assert_parity(out[..., 4:7], ref, r16(ref), 3, (0, 1), "conv_last fp16")
    assert bool((out.cpu()[..., :4] == 3).all()) and bool((out.cpu()[..., 7] == 3).all())
    f32 = ops.rrdb_conv(xd, wp, bp, n_real=3, ep="none", store="f32_nchw")
    assert f32.shape == (2, 3, 12, 20) and f32.dtype == torch.float32
    assert_parity(f32.permute(0, 2, 3, 1), ref, r16(ref), 3, (0, 1), "conv_last fp32 NCHW")
    assert rel_l2(f32.cpu().permute(0, 2, 3, 1), ref) < 1e-5        # no fp16 store in this form: fp32 accumulation error only
    u8 = ops.rrdb_conv(xd, wp, bp, n_real=3, ep="none", store="u8_hwc")
    assert u8.shape == (2, 12, 20, 3) and u8.dtype == torch.uint8
    want = up.model_output_to_u8(f32.cpu().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(u8.cpu().numpy(), want)            # the same accumulators through clamp, x255, round-half-even
    assert 0.02 < (want == 0).mean() + (want == 255).mean() < 0.9     # the clamp is exercised on both sides, and so is the interior


@pytest.mark.parametrize("cin", [32, 192])
def test_rrdb_conv_border_tap_counts_are_exact(dev, cin):
    """All-ones input and weights: an output pixel equals (taps inside the image) x cin — 4 at corners, 6 on edges, 9 inside — exactly."""
    ops = sub("ops")
    xd = torch.ones((2, 5, 6, cin), dtype=torch.float16).to(dev)
    wp = ops.pack_rrdb_weight(torch.ones((32, cin, 3, 3)).to(dev), 32)
    got = ops.rrdb_conv(xd, wp, None, ep="none", store="f32_nchw").cpu()
    taps = F.conv2d(torch.ones(1, 1, 5, 6), torch.ones(1, 1, 3, 3), padding=1)[0, 0]
    assert sorted(set(taps.flatten().tolist())) == [4.0, 6.0, 9.0]
    assert torch.equal(got, (taps * cin).expand(2, 32, 5, 6))


def test_rrdb_conv_refuses_what_it_is_not_built_for(dev):
    ops, _lib = sub("ops"), sub("_lib")
    xd = torch.zeros((1, 4, 4, 64), dtype=torch.float16).to(dev)
    wp = torch.zeros((48, 9, 64), dtype=torch.float16).to(dev)
    with pytest.raises(_lib.SdmiError, match="32 and 64"):
        ops.rrdb_conv(xd, wp, None)
    with pytest.raises(_lib.SdmiError, match="multiple of 32"):
        ops.rrdb_conv(torch.zeros((1, 4, 4, 224), dtype=torch.float16).to(dev), torch.zeros((32, 9, 224), dtype=torch.float16).to(dev), None)


# ---- network level ----------------------------------------------------------------------------------------------------------------
NETS = {}


def net_for(scale, old_arch=False):
    key = (scale, old_arch)
    if key not in NETS:
        sd = R.make_state_dict(2, scale)
        NETS[key] = (sd, sub("upscaler").EsrganNet(R.to_old_arch(sd, 2) if old_arch else sd, device=0))
    return NETS[key]


def image(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((b, 3, h, w), generator=g)


@pytest.mark.parametrize("scale,b,h,w", [(4, 2, 12, 20), (2, 1, 12, 20), (1, 1, 16, 24)])
def test_esrgan_network_vs_reference(dev, scale, b, h, w):
    sd, net = net_for(scale)
    assert (net.num_block, net.scale) == (2, scale)
    x = image(b, h, w, 10 + scale)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * scale, w * scale)
    m = b * (h * scale // 4) * (w * scale // 4)                 # low-resolution pixels; the 64-wide tensors at x4 alone are 2 x 16 m x 64 halfs
    assert 2 * 2 * 16 * m * 64 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    ref = R.forward(sd, x)
    assert_parity(got, ref, R.fp16_twin(sd, x), 1, (0, 2), f"x{scale} network")


def test_esrgan_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_esrgan_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB).  The x2 model:
    the pixel-unshuffle factor is part of the layout."""
    engine = sub("engine").Engine(0)
    net = sub("upscaler").EsrganNet(R.make_state_dict(2, 2), device=0, engine=engine)
    b, h, w = 1, 12, 20
    assert engine.arena_bytes() == 0
    got = net.run(image(b, h, w, 12).to(dev))
    n = net.scratch_bytes(b, h, w)
    m = b * (h // 2) * (w // 2)
    assert got.shape == (b, 3, 2 * h, 2 * w) and 2 * 2 * 16 * m * 64 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


def test_esrgan_old_arch_keys_give_the_same_network(dev):
    sd, new = net_for(4)
    _, old = net_for(4, old_arch=True)
    x = image(1, 17, 13, 21)
    got = old.run(x.to(dev))
    assert got.shape == (1, 3, 68, 52)
    assert torch.equal(got.cpu(), new.run(x.to(dev)).cpu())
    assert_parity(got, R.forward(sd, x), R.fp16_twin(sd, x), 1, (0, 2), "x4 old-arch 17x13")


# ---- the scaler object ------------------------------------------------------------------------------------------------------------
def test_upscaler_esrgan_do_upscale_hands_over_uint8_like_the_reference(dev, tmp_path):
    """do_upscale: a PIL image of the right size; against the fp32 reference's uint8 image the share of differing bytes is at most
    1.25 x the share the fp16-storage twin shows, the largest level difference no more than the twin's (floor 1).
    Measured on the MI355X (profiles/esrgan_parity.md): engine 2.5174 % of bytes differ, twin 3.3073 %; largest level difference 1 and 1."""
    from PIL import Image
    up = sub("upscaler")
    sd = R.make_state_dict(2, 4)
    path = str(tmp_path / "tiny_x4.pth")
    torch.save(sd, path)
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, size=(12, 20, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0)
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (80, 48) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and scaler.do_upscale(Image.fromarray(src), path).size == (80, 48) and len(scaler._nets) == 1
    x = torch.from_numpy(src.astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    ref = up.model_output_to_u8(R.forward(sd, x)[0].permute(1, 2, 0).numpy()).astype(np.int32)
    twin = up.model_output_to_u8(R.fp16_twin(sd, x)[0].permute(1, 2, 0).numpy()).astype(np.int32)
    got = np.asarray(img).astype(np.int32)
    share, twin_share = float((got != ref).mean()), float((twin != ref).mean())
    worst, twin_worst = int(np.abs(got - ref).max()), int(np.abs(twin - ref).max())
    print(f"[esrgan parity] do_upscale: differing bytes engine {share:.4%} twin {twin_share:.4%}; largest level difference engine {worst} twin {twin_worst}")
    assert ((ref == 0) | (ref == 255)).mean() < 0.05
    assert share <= 1.25 * twin_share, (share, twin_share)
    assert worst <= max(twin_worst, 1), (worst, twin_worst)


# ---- one job ----------------------------------------------------------------------------------------------------------------------
def test_hires_fix_job_with_a_registered_esrgan_upscaler(dev, tmp_path, monkeypatch):
    """txt2img with enable_hr, hr_scale = 2 and a registered x4 entry as hr_upscaler: the engine's job against the same job with the
    scaler's network replaced by the torch reference module in fp32.  Cap: that of test_hires_fix_image_space_upscaler_vs_oracle."""
    from PIL import Image
    schema, processing, shared, up = sub("schema"), sub("processing"), sub("shared"), sub("upscaler")
    sd = R.make_state_dict(1, 4)
    path = str(tmp_path / "tiny_x4.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae(ch_mult=(1, 1, 2, 2))
    model = sub("sd_models").SdModel(schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0x77), ucfg, vcfg, device=0)
    added = up.register_esrgan({"Tiny-ESRGAN 4x": path}, engine=model.engine)          # one engine, one arena: UNet, VAE and upscaler
    assert added[0].scaler.engine is model.engine
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-ESRGAN 4x"] and added[0].scale == 4
    g = torch.Generator().manual_seed(14)
    cond, uncond = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)

    def job():
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=3300, batch_size=1, steps=2, cfg_scale=5.0,
                                                        width=32, height=32, sampler_name="Euler a", enable_hr=True, hr_scale=2.0,
                                                        denoising_strength=0.6, hr_upscaler="Tiny-ESRGAN 4x")
        return processing.process_images(p)
    res = job()
    assert res.latents.shape == (1, 4, 8, 8) and res.images[0].shape == (64, 64, 3)
    module = R.RRDBNetModule(sd)

    def torch_do_upscale(img, selected_model=None):
        x = torch.from_numpy(np.asarray(img.convert("RGB")).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
        return Image.fromarray(up.model_output_to_u8(module(x)[0].permute(1, 2, 0).numpy()))
    monkeypatch.setattr(added[0].scaler, "do_upscale", torch_do_upscale)
    want = job()
    assert rel_l2(res.latents.cpu(), want.latents.cpu()) < 2e-2
