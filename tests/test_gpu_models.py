"""GPU parity tests, model level: whole-UNet forward, VAE decode/encode and the end-to-end txt2img/img2img loops of the
HIP engine against the fp32 CPU oracle on the same synthetic weights, conds and Philox seeds.

Stated tolerances (fp16 weights/activations, fp32 accumulation, fp32 sampler state):
  * one UNet / VAE forward ........ relative L2 <= 5e-3
  * final latent after a full sampler run: relative L2 <= 1e-2 on the tiny random-weight model (chaotic: random weights
    amplify fp16 rounding through the CFG scale 7); the SD1.5-size check on one step is held to 5e-3.
"""
import importlib

import os

import numpy as np
import pytest
import torch

from helpers import clip_tokens, rel_l2, seeded

pytestmark = pytest.mark.gpu


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tiny(dev):
    schema = sub("schema")
    from oracle import pipeline as opipe, unet as ou, vae as ov
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae()
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16)
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0)
    om = opipe.OracleModel(sd, ou.tiny_config(), ov.tiny_vae_config())
    g = torch.Generator().manual_seed(11)
    cond, uncond = torch.randn(4, 77, 64, generator=g), torch.randn(4, 77, 64, generator=g)
    return dict(sd=sd, model=model, oracle=om, cond=cond, uncond=uncond)


def test_unet_forward_tiny_vs_oracle(dev, tiny):
    eng, om = tiny["model"].engine, tiny["oracle"]
    x = seeded((4, 4, 16, 16), 1)
    t = torch.tensor([999.0, 500.25, 37.5, 1.0])
    ctx = tiny["cond"]
    ref = om.unet(x.half().float(), t, ctx.half().float())
    for dt in (torch.float32, torch.float16):
        got = eng.unet_forward(x.to(dev, dt), t.to(dev, dt), ctx.to(dev, dt))
        torch.cuda.synchronize()
        assert got.dtype == dt and got.shape == ref.shape
        tol = 5e-3 if dt == torch.float32 else 8e-3          # fp16 I/O also rounds the timesteps (500.25 -> 500.25, 37.5 ok)
        assert rel_l2(got.float().cpu(), ref) < tol
    # cached-context path gives the same bits as passing the context again
    a = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev))
    b = eng.unet_forward(x.to(dev), t.to(dev), None)
    assert torch.equal(a, b)


def test_unet_accuracy_mode_carries_the_residual_stream_with_22_bits(dev, tiny):
    """Engine option "residual_fp32": the carried stream as (hi, lo) fp16 pairs.  Same function, fewer roundings: the forward moves
    towards the fp32 oracle, and switching the option off restores the default forward bit for bit."""
    eng, om = tiny["model"].engine, tiny["oracle"]
    x = seeded((4, 4, 16, 16), 1)
    t = torch.tensor([999.0, 500.25, 37.5, 1.0])
    ctx = tiny["cond"]
    ref = om.unet(x.half().float(), t, ctx.half().float())
    base = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
    ref32 = om.unet(x, t, ctx.half().float())                # the accuracy mode hands conv_in the fp32 latent as a (hi, lo) pair
    xp, tp = torch.cat([x[:2], x[:2]]), torch.full((4,), 500.25)
    ctx_same = torch.cat([ctx[:2], ctx[:2]])
    eng.set_option("residual_fp32", 1)
    try:
        acc = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
        acc2 = eng.unet_forward(x.to(dev), t.to(dev), None).cpu()
        # round 6: the shared CFG prefix is combined with the option — both halves of every (hi, lo) tensor are copied
        rows = eng.unet_forward(xp.to(dev), tp.to(dev), ctx.to(dev)).cpu()
        pairs = eng.unet_forward(xp.to(dev), tp.to(dev), None, uniform_t=True, cfg_pairs=True).cpu()
        twin = eng.unet_forward(xp.to(dev), tp.to(dev), ctx_same.to(dev), uniform_t=True, cfg_pairs=True).cpu()
        eng.unet_forward(xp.to(dev), tp.to(dev), ctx.to(dev))  # (leaves both per-call options off)
    finally:
        eng.set_option("residual_fp32", 0)
    again = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
    assert torch.equal(base, again) and torch.equal(acc, acc2)
    e_base, e_acc = rel_l2(base, ref), rel_l2(acc, ref32)
    print(f"[tiny unet] default {e_base:.3e}  residual_fp32 {e_acc:.3e}  shared prefix vs per-row {rel_l2(pairs, rows):.3e}")
    assert torch.isfinite(acc).all() and e_acc < 0.9 * e_base and e_acc < 4e-3
    assert torch.equal(twin[:2], twin[2:]) and rel_l2(pairs, rows) < 6e-3 and rel_l2(pairs, om.unet(xp, tp, ctx.half().float())) < 4e-3


def test_unet_control_residuals_through_the_sdunet_boundary(dev, tiny):
    """Extra UNet inputs of SdUnet.forward (modules/sd_unet.py:76-77, 87-91 hand *args / **kwargs through): the ControlNet residuals of
    ldm's ControlledUnetModel.forward — one tensor per input block output + the middle block's, added to the skip connections as the
    output blocks read them and to the middle block's output — against the oracle's restatement; ``only_mid_control``; the residuals
    belong to ONE call; a wrong shape is an error, not a read past the tensor; the accuracy mode carries them into the (hi, lo) pair."""
    lib = sub("_lib")
    eng, om = tiny["model"].engine, tiny["oracle"]
    x = seeded((4, 4, 16, 16), 5)
    t = torch.tensor([999.0, 500.25, 37.5, 1.0])
    ctx = tiny["cond"]
    shapes = []
    hooks = [m.register_forward_hook(lambda mod, i, o: shapes.append(tuple(o.shape))) for m in list(om.unet.input_blocks) + [om.unet.middle_block]]
    ref_plain = om.unet(x.half().float(), t, ctx.half().float())
    for h in hooks:
        h.remove()
    control = [0.3 * seeded(sh, 40 + i) for i, sh in enumerate(shapes)]
    ref = om.unet(x.half().float(), t, ctx.half().float(), control=[c.half().float() for c in control])
    ref_mid = om.unet(x.half().float(), t, ctx.half().float(), control=[c.half().float() for c in control], only_mid_control=True)
    assert rel_l2(ref, ref_plain) > 5e-2 and rel_l2(ref_mid, ref) > 1e-2         # the residuals matter
    plain = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
    for dt, tol in ((torch.float32, 5e-3), (torch.float16, 8e-3)):
        ctl = [c.to(dev, dt) for c in control]
        got = eng.unet_forward(x.to(dev, dt), t.to(dev, dt), ctx.to(dev, dt), control=ctl).float().cpu()
        mid = eng.unet_forward(x.to(dev, dt), t.to(dev, dt), None, control=ctl, only_mid_control=True).float().cpu()
        assert rel_l2(got, ref) < tol and rel_l2(mid, ref_mid) < tol, (dt, rel_l2(got, ref), rel_l2(mid, ref_mid))
    assert torch.equal(eng.unet_forward(x.to(dev), t.to(dev), None).cpu(), plain)            # consumed: the next call is the plain forward
    # through the SdUnet adapter (B1), as the webui's patched UNetModel.forward calls it
    unet = sub("sd_unet").Mi355xUnet(lambda: None, unet_cfg=tiny["model"].unet_cfg, device_index=0)
    unet.engine = eng
    via = unet.forward(x.to(dev), t.to(dev), ctx.to(dev), control=[c.to(dev) for c in control]).float().cpu()
    assert rel_l2(via, ref) < 5e-3
    with pytest.raises(NotImplementedError, match="extra UNet inputs"):
        unet.forward(x.to(dev), t.to(dev), ctx.to(dev), some_other_input=1)
    with pytest.raises(lib.SdmiError, match="control"):
        eng.unet_forward(x.to(dev), t.to(dev), None, control=[c.to(dev) for c in control[:-1]])
    bad = [c.to(dev) for c in control]
    bad[3] = bad[3][:, :, :-1]
    with pytest.raises(lib.SdmiError, match="shape"):
        eng.unet_forward(x.to(dev), t.to(dev), None, control=bad)
    assert torch.equal(eng.unet_forward(x.to(dev), t.to(dev), None).cpu(), plain)            # a refused call leaves nothing behind
    ref32 = om.unet(x, t, ctx.half().float(), control=control)
    eng.set_option("residual_fp32", 1)
    try:
        acc = eng.unet_forward(x.to(dev), t.to(dev), None, control=[c.to(dev) for c in control]).cpu()
    finally:
        eng.set_option("residual_fp32", 0)
    assert rel_l2(acc, ref32) < 4e-3


def test_engine_promise_options_are_checkable(dev, tiny, monkeypatch):
    """cfg_pairs / uniform_t are promises of the caller about x and t; SDMI_CHECK_PROMISES=1 makes the engine verify them."""
    eng = tiny["model"].engine
    lib = sub("_lib")
    x = seeded((2, 4, 16, 16), 3)
    xx, t, ctx = torch.cat([x, x]).to(dev), torch.full((4,), 500.0).to(dev), tiny["cond"].to(dev)
    monkeypatch.setenv("SDMI_CHECK_PROMISES", "1")
    ok = eng.unet_forward(xx, t, ctx, uniform_t=True, cfg_pairs=True)
    assert torch.isfinite(ok).all()
    bad_x = xx.clone()
    bad_x[3, 0, 0, 0] += 1.0
    with pytest.raises(lib.SdmiError, match="cfg_pairs"):
        eng.unet_forward(bad_x, t, ctx, uniform_t=True, cfg_pairs=True)
    bad_t = t.clone()
    bad_t[1] = 400.0
    with pytest.raises(lib.SdmiError, match="uniform_t"):
        eng.unet_forward(xx, bad_t, ctx, uniform_t=True, cfg_pairs=False)
    monkeypatch.delenv("SDMI_CHECK_PROMISES")
    eng.unet_forward(xx, t, ctx, uniform_t=False, cfg_pairs=False)


def test_engine_derives_the_cfg_batch_promises_itself_when_asked(dev, tiny):
    """Engine option "auto_promises" (Mi355xUnet.forward behind the webui's stock CFG denoiser, opts.mi355x_auto_cfg_pairs): cfg_pairs /
    uniform_t are derived from the call's x and t — a [x | x] batch at one timestep takes the shared-prefix path (the bits of the promised
    form), anything else the per-row path (the bits of the plain call) —, and the caller's own settings are back afterwards."""
    eng = tiny["model"].engine
    x = seeded((2, 4, 16, 16), 3)
    xx, t, ctx = torch.cat([x, x]).to(dev), torch.full((4,), 500.0).to(dev), tiny["cond"].to(dev)
    plain = eng.unet_forward(xx, t, ctx)
    promised = eng.unet_forward(xx, t, ctx, uniform_t=True, cfg_pairs=True)
    auto = eng.unet_forward(xx, t, ctx, auto_promises=True)
    assert torch.equal(auto, promised)
    other = xx.clone()
    other[3, 0, 0, 0] += 1.0                                   # not a repeated half any more: per-row, nothing overwritten
    assert torch.equal(eng.unet_forward(other, t, ctx, auto_promises=True), eng.unet_forward(other, t, ctx))
    ramp = torch.tensor([500.0, 400.0, 500.0, 400.0]).to(dev)     # halves repeat, but two timesteps: neither promise holds
    assert torch.equal(eng.unet_forward(xx, ramp, ctx, auto_promises=True), eng.unet_forward(xx, ramp, ctx))
    assert torch.equal(eng.unet_forward(xx, t, ctx), plain)       # option off again: the plain call's bits


def test_unet_generic_and_mfma_paths_agree(dev, tiny):
    """Independent HIP implementations (MFMA+LDS vs one-thread-per-output) of every GEMM / attention in the UNet."""
    eng = tiny["model"].engine
    lib = sub("_lib")
    x, t, ctx = seeded((2, 4, 16, 16), 2).to(dev), torch.tensor([700.0, 20.0]).to(dev), tiny["cond"][:2].to(dev)
    a = eng.unet_forward(x, t, ctx)
    eng.set_option("force_generic", 1)
    try:
        b = eng.unet_forward(x, t, ctx)
    finally:
        eng.set_option("force_generic", 0)
    assert rel_l2(a.cpu(), b.cpu()) < 3e-3
    # direct-to-LDS vs register-staged loads: the same MFMA sequence, so bit-equal once both take the GroupNorm statistics the
    # same way (the epilogue-fused statistics exist in the direct-to-LDS kernels only; their summation order differs from the
    # stats pass in the last bits)
    lib.check(lib.lib.sdmi_debug_set(b"gn_fuse", 0))
    try:
        a0 = eng.unet_forward(x, t, ctx)
        eng.set_option("glds", 0)
        try:
            c = eng.unet_forward(x, t, ctx)
        finally:
            eng.set_option("glds", 1)
    finally:
        lib.check(lib.lib.sdmi_debug_set(b"gn_fuse", 1))
    assert torch.equal(a0, c)
    assert rel_l2(a.cpu(), a0.cpu()) < 5e-3              # chaotic random-weight toy: last-bit statistics differences grow to ~2e-3


def test_unet_wide_and_8_byte_epilogues_give_the_same_bits(dev, tiny):
    """Every GEMM epilogue of the UNet (incl. the GroupNorm-statistics one) with 16-byte accesses vs the 8-byte form."""
    eng = tiny["model"].engine
    lib = sub("_lib")
    x, t, ctx = seeded((2, 4, 16, 16), 2).to(dev), torch.tensor([700.0, 20.0]).to(dev), tiny["cond"][:2].to(dev)
    a = eng.unet_forward(x, t, ctx)
    lib.check(lib.lib.sdmi_debug_set(b"ep_wide", 0))
    try:
        b = eng.unet_forward(x, t, ctx)
    finally:
        lib.check(lib.lib.sdmi_debug_set(b"ep_wide", 1))
    assert torch.equal(a, b)


def test_unet_layernorm_folded_into_the_consuming_gemms(dev, tiny):
    """Engine option "ln_fold": norm1 / norm2 / norm3 of every transformer block finished inside the q|k, V^T, attn2.to_q and GEGLU
    GEMMs (folded weights + per-row statistics) against the separate LayerNorm kernel: the same function with one fp16 rounding of
    the normalised tensor replaced by one of the folded weights; and the folded copies follow an in-place weight / norm update."""
    eng = tiny["model"].engine
    x, t, ctx = seeded((2, 4, 16, 16), 2).to(dev), torch.tensor([700.0, 20.0]).to(dev), tiny["cond"][:2].to(dev)
    a = eng.unet_forward(x, t, ctx)
    eng.set_option("ln_fold", 1)
    try:
        b = eng.unet_forward(x, t, ctx)
        b2 = eng.unet_forward(x, t, ctx)
    finally:
        eng.set_option("ln_fold", 0)
    print(f"[ln_fold] tiny UNet forward, folded vs separate LayerNorm: {rel_l2(b.cpu(), a.cpu()):.3e}")
    assert torch.equal(b, b2)
    assert rel_l2(b.cpu(), a.cpu()) < 3e-3


def test_unet_batch_invariance_and_determinism(dev, tiny):
    eng = tiny["model"].engine
    x, t, ctx = seeded((4, 4, 16, 16), 3).to(dev), torch.tensor([300.0] * 4).to(dev), tiny["cond"].to(dev)
    full = eng.unet_forward(x, t, ctx)
    again = eng.unet_forward(x, t, ctx)
    assert torch.equal(full, again)                            # no atomics anywhere: bit-reproducible
    solo = eng.unet_forward(x[2:3].contiguous(), t[2:3].contiguous(), ctx[2:3].contiguous())
    # tile / split-K configuration follows the problem size, so the K-accumulation order (not the math) differs
    # between batch sizes: equal to fp16 rounding, not bitwise
    assert rel_l2(solo.cpu(), full[2:3].cpu()) < 5e-3


def test_vae_decode_and_encode_tiny_vs_oracle(dev, tiny):
    model, om = tiny["model"], tiny["oracle"]
    z = seeded((3, 4, 16, 16), 5) * 0.8
    ref = torch.stack([om.vae.decode_first_stage(z[i:i + 1])[0] for i in range(3)])
    got = model.decode_first_stage(z.to(dev))
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert rel_l2(got.cpu(), ref) < 5e-3
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(6)) * 2 - 1
    mref = om.vae.encode_moments(img.half().float())
    mgot = model.encode_first_stage(img.to(dev))
    assert rel_l2(mgot.cpu(), mref) < 5e-3
    lat = model.get_first_stage_encoding(mgot)
    assert rel_l2(lat.cpu(), om.vae.encode_first_stage_mean(img.half().float())) < 5e-3


def test_vae_attention_in_blocks_of_query_rows(dev, tiny):
    """The VAE's mid-block attention materialises its scores (one head, d = C); beyond `vae_attn_rows` query rows the product runs in
    row blocks over the whole key set (engine.cpp run_vae_attn, round 6: a 4096x4096 decode would need 275 GB of fp32 scores; the
    reference chunks the same product, modules/sd_hijack_optimizations.py:554-610).  Softmax rows are independent: the blocked decode
    is the unblocked one up to the rounding of another GEMM dispatch, it meets the oracle, and batch rows are kept apart."""
    lib = sub("_lib")
    eng, om = tiny["model"].engine, tiny["oracle"]
    z = seeded((2, 4, 16, 16), 31)                             # 256 tokens in the mid block
    whole = eng.vae_decode(z.to(dev)).cpu()
    ref = om.vae.decode_first_stage(z)
    try:
        lib.check(lib.lib.sdmi_debug_set(b"vae_attn_rows", 64))        # 4 blocks per image
        blocked = eng.vae_decode(z.to(dev)).cpu()
        lib.check(lib.lib.sdmi_debug_set(b"vae_attn_rows", 96))        # a ragged last block (96 + 96 + 64)
        ragged = eng.vae_decode(z.to(dev)).cpu()
        enc_b = tiny["model"].encode_first_stage(torch.tanh(seeded((1, 3, 32, 32), 32)).to(dev)).cpu()
    finally:
        lib.check(lib.lib.sdmi_debug_set(b"vae_attn_rows", 16384))
    enc = tiny["model"].encode_first_stage(torch.tanh(seeded((1, 3, 32, 32), 32)).to(dev)).cpu()
    assert torch.isfinite(blocked).all() and rel_l2(blocked, whole) < 1.5e-3 and rel_l2(ragged, whole) < 1.5e-3
    assert rel_l2(blocked, ref) < 6e-3 and rel_l2(ragged, ref) < 6e-3 and rel_l2(enc_b, enc) < 1.5e-3
    assert torch.equal(eng.vae_decode(z.to(dev)).cpu(), whole)          # the knob is back: the unblocked bits


def test_vae_decoder_against_reference_class_fixture(dev, golden_dir):
    """HIP decoder vs the output of the reference's own VAEDecoder class (modules/models/sd3/sd3_impls.py:305-355)."""
    import os
    from oracle import vae as ov
    from helpers import seeded_module_weights
    schema = sub("schema")
    z = np.load(os.path.join(golden_dir, "vae_decoder.npz"))
    dec = ov.Decoder(ov.tiny_vae_config())
    seeded_module_weights(dec, 779)                 # same seeded weights as tests/golden/make_golden.py
    sd = {schema.VAE_PREFIX + "decoder." + k: v for k, v in dec.state_dict().items()}
    zc = 4
    sd[schema.VAE_PREFIX + "post_quant_conv.weight"] = torch.eye(zc).reshape(zc, zc, 1, 1)
    sd[schema.VAE_PREFIX + "post_quant_conv.bias"] = torch.zeros(zc)
    cfg = schema.tiny_vae(scale_factor=1.0)
    eng = sub("engine").Engine(0)
    eng.load_vae(cfg, sd, decoder_only=True)
    got = eng.vae_decode(seeded((2, 4, 16, 16), 780).to(dev))
    assert rel_l2(got.cpu(), z["small_out"]) < 5e-3


@pytest.mark.parametrize("sampler,name,steps", [("euler_a", "Euler a", 5), ("dpmpp_2m", "DPM++ 2M", 6), ("ddim", "DDIM", 5),
                                                ("euler", "Euler", 4), ("heun", "Heun", 4), ("dpm_2", "DPM2", 4),
                                                ("dpm_2_a", "DPM2 a", 4), ("lms", "LMS", 6), ("dpmpp_2s_a", "DPM++ 2S a", 4),
                                                ("plms", "PLMS", 5), ("ddim_cfgpp", "DDIM CFG++", 5), ("restart", "Restart", 22),
                                                ("unipc", "UniPC", 6), ("lcm", "LCM", 4), ("dpm_fast", "DPM fast", 6),
                                                ("dpmpp_sde", "DPM++ SDE", 4), ("dpmpp_2m_sde", "DPM++ 2M SDE", 6),
                                                ("dpmpp_2m_sde_heun", "DPM++ 2M SDE Heun", 6), ("dpmpp_3m_sde", "DPM++ 3M SDE", 7),
                                                ("dpm_adaptive", "DPM adaptive", 6)])
def test_txt2img_tiny_end_to_end_vs_oracle(dev, tiny, sampler, name, steps):
    from oracle import pipeline as opipe
    processing = sub("processing")
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    # DPM adaptive: the PID step-size controller reacts to the (fp16-perturbed) error norm, so trial step sizes differ in the last
    # digits; at cfg 7 the chaotic random-weight model amplifies that to anything between 1e-2 and 8e-2 depending on the last bits of
    # the UNet, so this sampler runs at cfg 2 where the comparison means something — and even there a change in the fifth digit of
    # one activation function (round 5: the GEGLU gate, 2.5e-5 from the exact erf form) moved the result from 0.6e-2 to 1.34e-2: an
    # accepted / rejected trial step flips.  Its cap is therefore 3e-2; every fixed-step sampler keeps 1e-2.
    cfg = 2.0 if sampler == "dpm_adaptive" else 7.0
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=1000, batch_size=2,
                                                    steps=steps, cfg_scale=cfg, width=128, height=128, sampler_name=name)
    res = processing.process_images(p)
    lat, img, u8 = opipe.txt2img(tiny["oracle"], cond, uncond, [1000, 1001], steps, sampler, cfg, (16, 16))
    print(f"[e2e {sampler}] final latent rel-L2 {rel_l2(res.latents.cpu(), lat):.3e}")
    assert rel_l2(res.latents.cpu(), lat) < (3e-2 if sampler == "dpm_adaptive" else 1e-2), sampler
    # the tiny VAE has 2 levels: 16x16 latent -> 32x32 image
    assert len(res.images) == 2 and res.images[0].shape == (32, 32, 3) and res.images[0].dtype == np.uint8
    diff = np.abs(np.stack(res.images).astype(np.int32) - u8.astype(np.int32))
    assert diff.mean() < 2.0          # uint8 images agree to rounding of a few levels


@pytest.mark.parametrize("sampler,name,steps", [("euler_a", "Euler a", 3), ("dpmpp_2m", "DPM++ 2M", 3), ("ddim", "DDIM", 3), ("heun", "Heun", 2)])
def test_txt2img_smallest_job_end_to_end_vs_oracle(dev, tiny, sampler, name, steps):
    """One image, 8 x 8 latent, a few steps: the whole job (noise, CFG batch, UNet, sampler steps, VAE decode, uint8) at the smallest shape the
    kernels take — the end-to-end case that is also cheap on the host-emulated library (tests/test_cpu_emulated_library.py)."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    cond, uncond = tiny["cond"][:1], tiny["uncond"][:1]
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=77, batch_size=1, steps=steps, cfg_scale=6.0,
                                                    width=64, height=64, sampler_name=name)
    res = processing.process_images(p)
    lat, img, u8 = opipe.txt2img(tiny["oracle"], cond, uncond, [77], steps, sampler, 6.0, (8, 8))
    assert rel_l2(res.latents.cpu(), lat) < 1e-2, sampler
    assert len(res.images) == 1 and res.images[0].shape == (16, 16, 3) and res.images[0].dtype == np.uint8
    assert np.abs(res.images[0].astype(np.int32) - u8[0].astype(np.int32)).mean() < 2.0


@pytest.mark.parametrize("sampler,name", [("euler", "Euler"), ("heun", "Heun"), ("dpm_2", "DPM2")])
def test_txt2img_stochastic_churn_vs_oracle(dev, tiny, sampler, name):
    """opts.s_churn / s_tmin / s_tmax / s_noise (modules/sd_samplers_kdiffusion.py:36-39, 164-183; Karras et al. Algorithm 2): the
    steps whose sigma lies in [s_tmin, s_tmax] first raise the noise level with fresh noise from the job's ImageRNG.  The churned
    steps must draw from the generators in the oracle's order, the others must not draw at all."""
    from oracle import pipeline as opipe
    processing, shared = sub("processing"), sub("shared")
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    keep = (shared.opts.s_churn, shared.opts.s_tmin, shared.opts.s_tmax, shared.opts.s_noise)
    try:
        shared.opts.s_churn, shared.opts.s_tmin, shared.opts.s_tmax, shared.opts.s_noise = 8.0, 0.3, 9.0, 1.003
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=555, batch_size=2, steps=6,
                                                        cfg_scale=5.0, width=128, height=128, sampler_name=name)
        res = processing.process_images(p)
        shared.opts.s_churn = 0.0
        p0 = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=555, batch_size=2, steps=6,
                                                         cfg_scale=5.0, width=128, height=128, sampler_name=name)
        plain = processing.process_images(p0)
    finally:
        shared.opts.s_churn, shared.opts.s_tmin, shared.opts.s_tmax, shared.opts.s_noise = keep
    lat = opipe.sample(tiny["oracle"], cond, uncond, [555, 556], 6, sampler, 5.0, (16, 16), s_churn=8.0, s_tmin=0.3, s_tmax=9.0, s_noise=1.003)
    e = rel_l2(res.latents.cpu(), lat)
    print(f"[churn {sampler}] final latent rel-L2 {e:.3e}; churned vs plain {rel_l2(res.latents.cpu(), plain.latents.cpu()):.3e}")
    assert e < 1e-2, sampler
    assert rel_l2(res.latents.cpu(), plain.latents.cpu()) > 5e-2         # the churn really changed the trajectory


@pytest.mark.parametrize("variant,skip,order", [("vary_coeff", "time_uniform", 3), ("vary_coeff", "logSNR", 2), ("bh2", "time_quadratic", 3)])
def test_txt2img_unipc_option_variants_vs_oracle(dev, tiny, variant, skip, order):
    """opts.uni_pc_variant / uni_pc_skip_type / uni_pc_order (modules/shared_options.py:402-405): the vary_coeff solver
    (modules/models/diffusion/uni_pc/uni_pc.py:522-623 — the oracle's restatement is pinned to the reference at batch 1, the only batch
    size the reference's own code runs it at) and a non-default B(h) configuration, each update folded into sdmi_lincomb calls."""
    from oracle import pipeline as opipe
    processing, shared = sub("processing"), sub("shared")
    cond, uncond = tiny["cond"][:1], tiny["uncond"][:1]
    keep = (shared.opts.uni_pc_variant, shared.opts.uni_pc_skip_type, shared.opts.uni_pc_order)
    try:
        shared.opts.uni_pc_variant, shared.opts.uni_pc_skip_type, shared.opts.uni_pc_order = variant, skip, order
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=321, batch_size=1, steps=7,
                                                        cfg_scale=4.0, width=128, height=128, sampler_name="UniPC")
        res = processing.process_images(p)
    finally:
        shared.opts.uni_pc_variant, shared.opts.uni_pc_skip_type, shared.opts.uni_pc_order = keep
    lat = opipe.sample(tiny["oracle"], cond, uncond, [321], 7, "unipc", 4.0, (16, 16),
                       unipc_options=dict(variant=variant, skip_type=skip, order=order))
    e = rel_l2(res.latents.cpu(), lat)
    print(f"[unipc {variant} {skip} order {order}] final latent rel-L2 {e:.3e}")
    assert e < 1e-2


@pytest.mark.parametrize("sched,key", [("SGM Uniform", "sgm_uniform"), ("KL Optimal", "kl_optimal"), ("Exponential", "exponential"),
                                       ("Beta", "beta")])
def test_txt2img_scheduler_choice_vs_oracle(dev, tiny, sched, key):
    """p.scheduler routes through the scheduler table (modules/sd_samplers_kdiffusion.py:87-126) to the same sigmas as the oracle."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=77, batch_size=2, steps=5,
                                                    cfg_scale=6.0, width=128, height=128, sampler_name="Euler", scheduler=sched)
    res = processing.process_images(p)
    lat = opipe.sample(tiny["oracle"], cond, uncond, [77, 78], 5, "euler", 6.0, (16, 16), scheduler=key)
    assert rel_l2(res.latents.cpu(), lat) < 1e-2, sched


@pytest.mark.parametrize("sampler,name", [("euler_a", "Euler a"), ("ddim", "DDIM"), ("plms", "PLMS"), ("unipc", "UniPC"), ("lcm", "LCM")])
def test_inpainting_mask_paths_vs_oracle(dev, tiny, sampler, name):
    """img2img with a latent mask: k-diffusion samplers blend AFTER denoising (cfg_denoiser.py:292-293, fused into the CFG
    combine kernel), timestep samplers BEFORE (:186-187, sdmi_mask_blend on a copy); both end with processing.py:1776-1784."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    model, om = tiny["model"], tiny["oracle"]
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(11))
    mask = torch.zeros(2, 4, 16, 16)
    mask[:, :, 4:12, 2:9] = 1.0                          # 1 = keep the original latent there
    mask[1, :, 0:3, :] = 0.5                             # soft mask values blend
    p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=3000, batch_size=2, steps=5, cfg_scale=7.0,
                                                    width=128, height=128, sampler_name=name, init_images=img,
                                                    denoising_strength=0.6, latent_mask=mask)
    res = processing.process_images(p)
    init = om.vae.encode_first_stage_mean(img.half().float() * 2 - 1)
    lat = opipe.sample(om, cond, uncond, [3000, 3001], 5, sampler, 7.0, (16, 16), init_latent=init, denoising_strength=0.6,
                       img2img_steps_given=False, mask=mask)
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2, sampler
    keep = mask == 1.0
    assert rel_l2(res.latents.cpu()[keep], init[keep]) < 5e-3            # masked region = the encoded original


def _tiny_lora(cfg_schema, seed, rank=4):
    """A kohya-style LoRA for the tiny UNet: self-attention q / k (stacked inside the engine), cross-attention k / v (cached
    projections), GEGLU feed-forward, 1x1 proj_in, the time-embedding projection of a ResBlock and a 3x3 LoCon conv."""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: s for k, s, _ in cfg_schema}
    targets = {
        "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q": "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight",
        "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_k": "input_blocks.1.1.transformer_blocks.0.attn1.to_k.weight",
        "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_k": "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight",
        "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_v": "input_blocks.1.1.transformer_blocks.0.attn2.to_v.weight",
        "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_ff_net_0_proj": "input_blocks.1.1.transformer_blocks.0.ff.net.0.proj.weight",
        "lora_unet_down_blocks_0_attentions_0_proj_in": "input_blocks.1.1.proj_in.weight",
        "lora_unet_down_blocks_0_resnets_0_time_emb_proj": "input_blocks.1.0.emb_layers.1.weight",
        "lora_unet_mid_block_resnets_0_conv1": "middle_block.0.in_layers.2.weight",
    }
    sd = {}
    for lk, ck in targets.items():
        shp = shapes[ck]
        out_c, in_c = shp[0], shp[1]
        if len(shp) == 4 and shp[2] == 3:
            up, down = torch.randn(out_c, rank, 1, 1, generator=g), torch.randn(rank, in_c, 3, 3, generator=g) * (in_c * 9) ** -0.5
        elif len(shp) == 4:
            up, down = torch.randn(out_c, rank, 1, 1, generator=g), torch.randn(rank, in_c, 1, 1, generator=g) * in_c ** -0.5
        else:
            up, down = torch.randn(out_c, rank, generator=g), torch.randn(rank, in_c, generator=g) * in_c ** -0.5
        sd[lk + ".lora_up.weight"] = (up * 0.3).half()
        sd[lk + ".lora_down.weight"] = down.half()
        sd[lk + ".alpha"] = torch.tensor(float(rank) / 2)
    sd["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_up.weight"] = torch.randn(8, rank, generator=g).half()
    return sd


def test_lora_merge_into_engine_vs_oracle_and_restore(dev, tiny):
    """networks.load_networks rewrites the packed engine weights (incl. the stacked q|k, the cached cross-attention K / V and
    the interleaved GEGLU rows); the UNet then matches the oracle built from oracle.lora.merge'd weights, two networks
    accumulate, and unloading restores the original output bit for bit."""
    schema, nets = sub("schema"), sub("networks")
    from oracle import lora as olora, unet as ou
    model, sd = tiny["model"], tiny["sd"]
    eng = model.engine
    x = seeded((4, 4, 16, 16), 21).to(dev)
    t = torch.tensor([900.0, 900.0, 120.0, 120.0], device=dev)
    ctx = seeded((4, 77, 64), 22).to(dev)

    def fwd():
        eng.set_context(ctx)
        return eng.unet_forward(x, t, None, None).float().cpu()
    base = fwd()
    la, lb = _tiny_lora(schema.unet_schema(schema.tiny_unet()), 5), _tiny_lora(schema.unet_schema(schema.tiny_unet()), 6, rank=8)
    try:
        loaded = nets.load_networks(model, ["a"], [la], unet_multipliers=[0.9])
        assert len(loaded[0].modules) == 8 and len(loaded[0].keys_failed_to_match) == 1
        got = fwd()
        ref_sd = olora.merge({k: v.float() for k, v in sd.items()}, [(la, 0.9)])
        ref = ou.build_unet(ou.tiny_config(), ref_sd)(x.cpu(), t.cpu(), ctx.cpu())
        assert rel_l2(got, ref) < 8e-3
        assert rel_l2(got, base) > 5e-2                                   # the LoRA really changed the output
        nets.load_networks(model, ["a", "b"], [la, lb], unet_multipliers=[0.9, -0.4])
        got2 = fwd()
        ref_sd2 = olora.merge({k: v.float() for k, v in sd.items()}, [(la, 0.9), (lb, -0.4)])
        ref2 = ou.build_unet(ou.tiny_config(), ref_sd2)(x.cpu(), t.cpu(), ctx.cpu())
        assert rel_l2(got2, ref2) < 8e-3
    finally:
        nets.load_networks(model, [], [])
    assert torch.equal(fwd(), base)


def test_lycoris_module_types_vs_reference_fixture(dev, golden_dir):
    """Every module type of networks.module_types on the reference-generated cases of tests/golden/lyco.npz (LoRA / LoCon with
    cp-decomposition, DoRA and dyn_dim, LoHa with and without Tucker cores, LoKr in its four forms, GLoRA, IA3, full diff with a
    bias difference, norm, OFT / COFT / old-LyCORIS OFT / BOFT with rescale, modules with the dense "bias" entry): W + updown computed through the HIP kernels equals
    W + the reference's calc_updown, and the bias deltas equal its ex_bias."""
    from tests.test_oracle_pins import _golden_module
    nets = sub("networks")
    mg = _golden_module()
    z = np.load(os.path.join(golden_dir, "lyco.npz"))
    seen = set()
    cases = list(mg.lyco_cases().items()) + list(mg.lyco_oft_cases().items()) + list(mg.lyco_bias_cases().items())   # same indexing as gen_lyco
    for k, (name, (kind, spec, build)) in enumerate(cases):
        orig, w = mg.lyco_orig_weight(spec, k), build(9000 + 10 * k)
        net = nets.Network("n", unet_multiplier=0.8, te_multiplier=0.3, dyn_dim=3 if name == "lora_dyn" else None)
        weights = nets.NetworkWeights(network_key="lora_unet_x", sd_key="diffusion_model_x", w=dict(w), engine_key="x.weight")
        module = None
        for mt in nets.module_types:
            module = mt.create_module(net, weights, tuple(orig.shape))
            if module is not None:
                break
        assert module is not None and module.kind == kind, name
        got = nets._merge_on_device(orig.to(dev), module, dev)
        torch.cuda.synchronize()
        want = orig + torch.from_numpy(z[name + "_updown"])
        assert got.shape == want.shape and float((got.cpu() - want).abs().max()) < 2e-6, name
        if name + "_ex_bias" in z.files:                     # bias deltas: full diff_b, norm b_norm (x multiplier)
            eb = module.ex_bias(dev)
            assert float((eb.cpu() - torch.from_numpy(z[name + "_ex_bias"])).abs().max()) < 1e-7, name
        else:
            assert module.ex_bias(dev) is None
        seen.add(kind)
    assert seen == {"lora", "hada", "lokr", "glora", "ia3", "full", "norm", "oft"}


def test_lycoris_networks_into_engine_vs_oracle(dev, tiny):
    """A LoHa + LoKr + IA3 + DoRA network and a plain LoRA loaded together: the rewritten engine matches the oracle UNet built from
    oracle.lora.merge'd weights, and unloading restores the original bits."""
    schema, nets = sub("schema"), sub("networks")
    from oracle import lora as olora, unet as ou
    model, sd = tiny["model"], tiny["sd"]
    eng = model.engine
    x = seeded((2, 4, 16, 16), 31).to(dev)
    t = torch.tensor([700.0, 80.0], device=dev)
    ctx = seeded((2, 77, 64), 32).to(dev)

    def fwd():
        eng.set_context(ctx)
        return eng.unet_forward(x, t, None, None).float().cpu()
    base = fwd()
    g = torch.Generator().manual_seed(77)
    r = lambda *shape: torch.randn(*shape, generator=g) * 0.25
    blk = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_"
    lyco = {
        # LoHa on the self-attention v projection (64 -> 64)
        blk + "attn1_to_v.hada_w1_a": r(64, 4), blk + "attn1_to_v.hada_w1_b": r(4, 64), blk + "attn1_to_v.hada_w2_a": r(64, 4),
        blk + "attn1_to_v.hada_w2_b": r(4, 64), blk + "attn1_to_v.alpha": torch.tensor(4.0),
        # LoKr on the feed-forward output (256 -> 64): kron([8,16], [8,16])
        blk + "ff_net_2.lokr_w1": r(8, 16), blk + "ff_net_2.lokr_w2": r(8, 16), blk + "ff_net_2.alpha": torch.tensor(1.0),
        # IA3 on the cross-attention k projection (64 <- 64), per output row
        blk + "attn2_to_k.weight": r(64) * 0.5, blk + "attn2_to_k.on_input": torch.tensor(False),
        # DoRA LoCon on a 3x3 conv of the middle block
        "lora_unet_mid_block_resnets_0_conv1.lora_up.weight": r(128, 4, 1, 1), "lora_unet_mid_block_resnets_0_conv1.lora_down.weight": r(4, 128, 3, 3) * 0.3,
        "lora_unet_mid_block_resnets_0_conv1.alpha": torch.tensor(4.0),
        "lora_unet_mid_block_resnets_0_conv1.dora_scale": torch.rand(1, 128, 1, 1, generator=g) * 0.2 + 0.55,
        # full diff on the 1x1 proj_out, with a bias difference
        "lora_unet_down_blocks_0_attentions_0_proj_out.diff": r(64, 64, 1, 1) * 0.2,
        "lora_unet_down_blocks_0_attentions_0_proj_out.diff_b": r(64) * 0.3,
        # norm modules: a ResBlock GroupNorm and a transformer LayerNorm (gain and shift differences)
        "lora_unet_down_blocks_0_resnets_0_norm1.w_norm": r(64) * 0.4, "lora_unet_down_blocks_0_resnets_0_norm1.b_norm": r(64) * 0.4,
        blk + "norm2.w_norm": r(64) * 0.4, blk + "norm2.b_norm": r(64) * 0.4,
        # OFT (4 blocks of 16 rows) on the cross-attention q projection, BOFT (2 butterfly factors, blocks of 8) on attn1 to_q
        blk + "attn2_to_q.oft_blocks": r(4, 16, 16) * 0.4,
        blk + "attn1_to_q.oft_blocks": r(2, 8, 8, 8) * 0.4,
    }
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes[schema.UNET_PREFIX + "middle_block.0.in_layers.2.weight"] == (128, 128, 3, 3)
    la = _tiny_lora(schema.unet_schema(schema.tiny_unet()), 9)
    try:
        loaded = nets.load_networks(model, ["lyco", "a"], [lyco, la], unet_multipliers=[0.7, 0.5])
        assert sorted(m.kind for m in loaded[0].modules.values()) == ["full", "hada", "ia3", "lokr", "lora", "norm", "norm", "oft", "oft"]
        got = fwd()
        ref_sd = olora.merge({k: v.float() for k, v in sd.items()}, [(lyco, 0.7), (la, 0.5)])
        ref = ou.build_unet(ou.tiny_config(), ref_sd)(x.cpu(), t.cpu(), ctx.cpu())
        assert rel_l2(got, ref) < 8e-3 and rel_l2(got, base) > 5e-2
    finally:
        nets.load_networks(model, [], [])
    assert torch.equal(fwd(), base)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_clip_text_encoder_tiny_vs_oracle(dev, act):
    """sdmi_clip_forward behind encode_with_transformers: last hidden state, clip skip 2 (+ final norm), SDXL-style
    hidden_states[-2] without the norm, pooled row, textual-inversion style inputs_embeds; MFMA and generic kernels agree."""
    schema, hc, eng_mod = sub("schema"), sub("sd_hijack_clip"), sub("engine")
    from oracle import clip as oclip
    cfg = schema.tiny_clip(act=act)
    sd = schema.synthetic_state_dict(clip_cfg=cfg, dtype=torch.float16)
    om = oclip.build_clip(oclip.ClipConfig(vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                                           intermediate=cfg.intermediate, act=act), sd)
    eng = eng_mod.Engine(0)
    enc = hc.Mi355xClipTextEncoder(eng, cfg, sd)
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 998, (3, 77), generator=g)
    tok[:, 0] = 998
    tok[0, 12:] = 999
    tok[1, 60:] = 999
    tok[2, 76] = 999
    shared = sub("shared")
    got = enc.encode_with_transformers(tok.to(dev))
    assert got.shape == (3, 77, cfg.hidden) and got.dtype == torch.float32
    assert rel_l2(got.cpu(), om(tok)) < 4e-3
    try:
        shared.opts.CLIP_stop_at_last_layers = 2
        assert rel_l2(enc.encode_with_transformers(tok.to(dev)).cpu(), om(tok, skip=2)) < 4e-3
    finally:
        shared.opts.CLIP_stop_at_last_layers = 1
    enc.layer, enc.layer_idx = "hidden", 2                       # SDXL CLIP-L style: hidden_states[layer_idx], no final norm
    want = om.hidden_states(tok)[2]
    assert rel_l2(enc.encode_with_transformers_sdxl(tok.to(dev)).cpu(), want) < 4e-3
    out, pooled = eng.clip_forward(tok.to(dev), return_pooled=True)
    _, opooled = om(tok, return_pooled=True)
    assert rel_l2(pooled.cpu(), opooled) < 4e-3
    emb = om.embeddings.token_embedding(tok).detach().clone()
    emb[1, 5:9] = torch.randn(4, cfg.hidden, generator=g) * 0.5   # a 4-vector textual-inversion embedding spliced in
    got_e = eng.clip_forward(tok.to(dev), inputs_embeds=emb.to(dev))
    assert rel_l2(got_e.cpu(), om(tok, inputs_embeds=emb)) < 4e-3
    assert rel_l2(got_e.cpu()[0], got.cpu()[0]) < 1e-6            # image 0 untouched by the splice in image 1
    eng.set_option("force_generic", 1)
    try:
        gen = eng.clip_forward(tok.to(dev))
    finally:
        eng.set_option("force_generic", 0)
    assert rel_l2(gen.cpu(), got.cpu()) < 2e-3
    # causality: changing tokens after position 30 must not change positions <= 30
    tok2 = tok.clone()
    tok2[:, 31:] = torch.randint(0, 998, (3, 46), generator=g)
    got2 = eng.clip_forward(tok2.to(dev))
    assert torch.equal(got2[:, :31], got[:, :31])


def test_openclip_layout_penultimate_and_pooled_projection_vs_oracle(dev):
    """An open_clip-layout text tower (packed in_proj, ln_1/ln_2, c_fc/c_proj, positional_embedding, text_projection [C, P]) is
    translated to the engine's layout; SD 2.x semantics (penultimate + ln_final) and SDXL bigG semantics (penultimate without
    ln_final, pooled = ln_final(last)[EOS] @ text_projection) match the oracle."""
    schema, hc, eng_mod = sub("schema"), sub("sd_hijack_clip"), sub("engine")
    from oracle import clip as oclip
    C, P, layers = 128, 192, 3
    g = torch.Generator().manual_seed(17)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    pre = "conditioner.embedders.1.model."
    oc = {pre + "token_embedding.weight": rn(1000, C, sc=0.5), pre + "positional_embedding": rn(77, C, sc=0.5),
          pre + "ln_final.weight": 1 + rn(C, sc=0.02), pre + "ln_final.bias": rn(C, sc=0.02), pre + "text_projection": rn(C, P, sc=C ** -0.5)}
    for i in range(layers):
        b = pre + f"transformer.resblocks.{i}."
        oc.update({b + "ln_1.weight": 1 + rn(C, sc=0.02), b + "ln_1.bias": rn(C, sc=0.02), b + "ln_2.weight": 1 + rn(C, sc=0.02),
                   b + "ln_2.bias": rn(C, sc=0.02), b + "attn.in_proj_weight": rn(3 * C, C, sc=C ** -0.5),
                   b + "attn.in_proj_bias": rn(3 * C, sc=0.02), b + "attn.out_proj.weight": rn(C, C, sc=C ** -0.5),
                   b + "attn.out_proj.bias": rn(C, sc=0.02), b + "mlp.c_fc.weight": rn(2 * C, C, sc=C ** -0.5),
                   b + "mlp.c_fc.bias": rn(2 * C, sc=0.02), b + "mlp.c_proj.weight": rn(C, 2 * C, sc=(2 * C) ** -0.5),
                   b + "mlp.c_proj.bias": rn(C, sc=0.02)})
    oc = {k: v.half() for k, v in oc.items()}
    sd = schema.openclip_to_transformers_keys(oc, pre)
    cfg = schema.ClipConfig(vocab_size=1000, hidden=C, layers=layers, heads=2, intermediate=2 * C, act="gelu", proj_dim=P)
    om = oclip.build_clip(oclip.ClipConfig(vocab_size=1000, hidden=C, layers=layers, heads=2, intermediate=2 * C, act="gelu", proj_dim=P), sd)
    enc = hc.Mi355xClipTextEncoder(eng_mod.Engine(0), cfg, sd)
    tok = torch.randint(1, 990, (2, 77), generator=g)
    tok[:, 0] = 998
    tok[0, 15] = 999; tok[0, 16:] = 0                       # open_clip pads with 0 after <end_of_text>
    tok[1, 40] = 999; tok[1, 41:] = 0
    z2 = enc.encode_with_transformer_openclip(tok.to(dev))
    assert rel_l2(z2.cpu(), om(tok, skip=2, apply_final_ln=True)) < 4e-3
    z = enc.encode_with_transformer_openclip2(tok.to(dev))
    want, wpool = om(tok, skip=2, apply_final_ln=False, return_pooled=True)
    assert z.shape == (2, 77, C) and z.pooled.shape == (2, P)
    assert rel_l2(z.cpu(), want) < 4e-3 and rel_l2(z.pooled.cpu(), wpool) < 5e-3


def test_clip_l_full_size_vs_oracle(dev):
    """CLIP-L geometry (12 layers x 768, 12 heads of 64, 3072 MLP, vocab 49408) with seeded synthetic weights, B = 2."""
    schema, eng_mod = sub("schema"), sub("engine")
    from oracle import clip as oclip
    cfg = schema.sd15_clip()
    sd = schema.synthetic_state_dict(clip_cfg=cfg, dtype=torch.float16)
    eng = eng_mod.Engine(0)
    eng.load_clip(cfg, sd)
    tok = torch.randint(0, 49405, (2, 77), generator=torch.Generator().manual_seed(5))
    tok[:, 0] = 49406
    tok[0, 9:] = 49407
    tok[1, 70:] = 49407
    got = eng.clip_forward(tok.to(dev))
    ref = oclip.build_clip(oclip.ClipConfig(), sd)(tok)
    assert rel_l2(got.cpu(), ref) < 5e-3


@pytest.mark.parametrize("sampler,name,steps", [("euler_a", "Euler a", 4), ("dpmpp_2m", "DPM++ 2M", 5), ("ddim", "DDIM", 5),
                                                ("ddim_cfgpp", "DDIM CFG++", 5)])
def test_v_prediction_model_vs_oracle(dev, sampler, name, steps):
    """parameterization == "v" (SD 2.x 768-v): CompVisVDenoiser scalings in sigma space, v -> eps conversion in timestep
    space (modules/sd_samplers_timesteps.py:33-45), fused into sdmi_cfg_combine_affine; SD2-style UNet (linear proj_in/out)."""
    from oracle import pipeline as opipe, unet as ou
    schema, processing = sub("schema"), sub("processing")
    ucfg = schema.tiny_unet(use_linear_in_transformer=True)
    sd = schema.synthetic_state_dict(ucfg, None, dtype=torch.float16)
    model = sub("sd_models").SdModel(sd, ucfg, None, device=0, load_vae=False, parameterization="v")
    om = opipe.OracleModel(sd, ou.tiny_config(use_linear_in_transformer=True), None)
    g = torch.Generator().manual_seed(12)
    cond, uncond = torch.randn(2, 77, 64, generator=g), torch.randn(2, 77, 64, generator=g)
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=500, batch_size=2, steps=steps,
                                                    cfg_scale=5.0, width=128, height=128, sampler_name=name)
    p.decode = False
    sampler_obj = sub("sd_samplers").create_sampler(name, model)
    p.rng = sub("rng").ImageRNG((4, 16, 16), [500, 501], device=dev)
    p.seeds = [500, 501]
    got = sampler_obj.sample(p, p.rng.next(), cond.to(dev), uncond.to(dev))
    lat = opipe.sample(om, cond, uncond, [500, 501], steps, sampler, 5.0, (16, 16), parameterization="v")
    assert rel_l2(got.cpu(), lat) < 1e-2, sampler
    eps_lat = opipe.sample(om, cond, uncond, [500, 501], steps, sampler, 5.0, (16, 16))
    assert rel_l2(got.cpu(), eps_lat) > 5e-2                 # and it is not the eps-parameterised answer


CFG_VARIANTS = {
    # name: (conds_list, T_cond, T_uncond, s_min_uncond, step, opts)
    "and": ([[(0, 1.0), (1, 0.6)], [(2, 0.8)]], 77, 77, 0.0, 0, {}),
    "weight": ([[(0, 1.3)], [(1, 0.7)]], 77, 77, 0.0, 0, {}),
    "ngms_odd": (None, 77, 77, 5.0, 1, {}),
    "ngms_even": (None, 77, 77, 5.0, 2, {}),
    "ngms_all": (None, 77, 77, 5.0, 2, {"s_min_uncond_all": True}),
    "skip_early_and": ([[(0, 1.0), (1, 0.6)], [(2, 0.8)]], 77, 77, 0.0, 1, {"skip_early_cond": 0.3}),
    "long_cond": (None, 154, 77, 0.0, 0, {}),
    "long_uncond": (None, 77, 231, 0.0, 0, {}),
    "long_cond_pad": (None, 154, 77, 0.0, 0, {"pad_cond_uncond": True}),
    "long_uncond_pad_v0": (None, 77, 231, 0.0, 0, {"pad_cond_uncond_v0": True}),
    "long_cond_skip": (None, 154, 77, 5.0, 1, {}),
}


@pytest.mark.parametrize("mode", ["sigma", "timestep"])
@pytest.mark.parametrize("variant", sorted(CFG_VARIANTS))
def test_cfg_denoiser_variants_vs_oracle(dev, tiny, variant, mode):
    """One CFGDenoiser.forward per scenario of modules/sd_samplers_cfg_denoiser.py:156-311 beyond plain CFG — AND composition,
    prompt weights, skip-uncond (NGMS odd / even / all steps, skip-early), cond / uncond of different token counts (two UNet
    calls; the two padding options) — in sigma space (k-diffusion samplers) and timestep space (DDIM family), against the
    oracle's CFGDenoiser (itself pinned to the reference class by tests/golden/cfg_denoiser.npz)."""
    from oracle import kdiffusion as okd
    ss, shared = sub("sd_samplers"), sub("shared")
    conds_list, t_c, t_u, s_min, step, o = CFG_VARIANTS[variant]
    model, om = tiny["model"], tiny["oracle"]
    b = 2
    g = torch.Generator().manual_seed(321)
    n_cond = b if conds_list is None else sum(len(c) for c in conds_list)
    cond, uncond = torch.randn(n_cond, t_c, 64, generator=g), torch.randn(b, t_u, 64, generator=g)
    empty = torch.randn(1, 77, 64, generator=g)
    x = seeded((b, 4, 16, 16), 77) * 2.0
    sig = 2.0 if mode == "sigma" else 401.0
    if mode == "timestep" and s_min > 0:
        s_min = 500.0                                         # there "sigma" is the timestep the threshold is compared with
    sigma = torch.full((b,), sig)
    keep = {k: getattr(shared.opts, k) for k in o}
    model.cond_stage_model_empty_prompt = empty.to(dev)
    try:
        for k, v in o.items():
            setattr(shared.opts, k, v)
        sampler = ss.create_sampler("Euler a" if mode == "sigma" else "DDIM", model)
        cfg = sampler.model_wrap_cfg
        cfg.step, cfg.total_steps = step, 10
        c_arg = cond.to(dev) if conds_list is None else (conds_list, cond.to(dev))
        got = cfg(x.to(dev), sigma.to(dev), uncond.to(dev), c_arg, 7.0, s_min_uncond=s_min)
        torch.cuda.synchronize()
    finally:
        for k, v in keep.items():
            setattr(shared.opts, k, v)
    if mode == "sigma":
        inner = okd.CompVisDenoiser(lambda xi, t, c: om.apply_model(xi, t, c), om.alphas_cumprod)
    else:
        inner = lambda xi, t, c: om.apply_model(xi, t, c)
    oc = okd.CFGDenoiser(inner)
    oc.step, oc.total_steps, oc.empty_prompt = step, 10, empty
    for k, v in o.items():
        setattr(oc, k, v)
    c_arg = cond if conds_list is None else (conds_list, cond)
    want = oc(x, sigma, uncond, c_arg, 7.0, s_min_uncond=s_min)
    assert oc.skipped_uncond == (variant in ("ngms_odd", "ngms_all", "skip_early_and", "long_cond_skip"))
    assert rel_l2(got.cpu(), want) < 1e-2, (variant, mode)
    assert cfg.step == step + 1 and cfg.padded_cond_uncond == oc.padded_cond_uncond and cfg.padded_cond_uncond_v0 == oc.padded_cond_uncond_v0


def test_txt2img_ngms_end_to_end_vs_oracle(dev, tiny):
    """p.s_min_uncond reaches the denoiser through sampler_extra_args (modules/sd_samplers_kdiffusion.py:197-203): alternate
    low-sigma steps run the UNet on the cond rows only."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=1000, batch_size=2, steps=6,
                                                    cfg_scale=7.0, width=128, height=128, sampler_name="Euler a", s_min_uncond=20.0)
    res = processing.process_images(p)
    lat = opipe.sample(tiny["oracle"], cond, uncond, [1000, 1001], 6, "euler_a", 7.0, (16, 16), s_min_uncond=20.0)
    plain = opipe.sample(tiny["oracle"], cond, uncond, [1000, 1001], 6, "euler_a", 7.0, (16, 16))
    assert rel_l2(res.latents.cpu(), lat) < 1e-2 and rel_l2(plain, lat) > 5e-2


def _concat_model(in_channels, **kw):
    from oracle import pipeline as opipe, unet as ou, vae as ov
    schema = sub("schema")
    ucfg, vcfg = schema.tiny_unet(in_channels=in_channels), schema.tiny_vae()
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0x1A9 + in_channels)
    assert sub("sd_models").guess_unet_config({schema.UNET_PREFIX + "input_blocks.0.0.weight": sd[schema.UNET_PREFIX + "input_blocks.0.0.weight"]}).in_channels == in_channels
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0, **kw)
    om = opipe.OracleModel(sd, ou.tiny_config(in_channels=in_channels), ov.tiny_vae_config())
    g = torch.Generator().manual_seed(13)
    return model, om, torch.randn(2, 77, 64, generator=g), torch.randn(2, 77, 64, generator=g)


@pytest.mark.parametrize("sampler,name", [("euler_a", "Euler a"), ("ddim", "DDIM")])
def test_inpainting_checkpoint_vs_oracle(dev, sampler, name):
    """9-channel inpainting checkpoints (conditioning_key "hybrid"): c_concat = [mask | masked-image latent] is concatenated to
    every UNet input row (sdmi_cfg_prepare_concat).  txt2img conditions on an all-masked flat image (processing.py:100-111);
    img2img on lerp(image, image * (1 - mask), weight) encoded + the mask at latent size (processing.py:332-374), together with
    the latent-mask blends."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    model, om, cond, uncond = _concat_model(9)
    assert model.model.conditioning_key == "hybrid" and model.cond_stage_key == "txt"
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=900, batch_size=2, steps=4, cfg_scale=6.0,
                                                    width=128, height=128, sampler_name=name)
    res = processing.process_images(p)
    ic = opipe.txt2img_image_conditioning(om, 2, 32, 32)      # the tiny VAE has f = 2: a 16x16 latent is a 32x32 image
    assert ic.shape == (2, 5, 16, 16)
    lat = opipe.sample(om, cond, uncond, [900, 901], 4, sampler, 6.0, (16, 16), image_cond=ic)
    assert rel_l2(res.latents.cpu(), lat) < 1e-2
    other = opipe.sample(om, cond, uncond, [900, 901], 4, sampler, 6.0, (16, 16), image_cond=torch.zeros_like(ic))
    assert rel_l2(other, lat) > 3e-2                          # the conditioning channels matter

    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(21)).half().float()
    image_mask = torch.zeros(1, 1, 32, 32)
    image_mask[:, :, 8:24, 4:20] = 1.0
    image_mask[:, :, 0:4, :] = 0.6                            # rounds to 1
    image_mask[:, :, 28:, :] = 0.4                            # rounds to 0
    latent_mask = 1.0 - torch.nn.functional.interpolate(torch.round(image_mask), size=(16, 16)).expand(2, 4, 16, 16)
    for weight in (1.0, 0.7):
        p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=910, batch_size=2, steps=5, cfg_scale=6.0,
                                                        width=128, height=128, sampler_name=name, init_images=img,
                                                        denoising_strength=0.7, latent_mask=latent_mask, image_mask=image_mask,
                                                        inpainting_mask_weight=weight)
        res = processing.process_images(p)
        init = om.vae.encode_first_stage_mean(img * 2 - 1)
        ic = opipe.inpainting_image_conditioning(om, img * 2 - 1, (16, 16), image_mask, mask_weight=weight)
        lat = opipe.sample(om, cond, uncond, [910, 911], 5, sampler, 6.0, (16, 16), init_latent=init, denoising_strength=0.7,
                           img2img_steps_given=False, mask=latent_mask, image_cond=ic)
        assert rel_l2(res.latents.cpu(), lat) < 1.5e-2, weight


def test_instruct_pix2pix_checkpoint_vs_oracle(dev):
    """8-channel InstructPix2Pix checkpoints (cond_stage_key "edit"): three UNet rows per image — [cond, image], [uncond, image],
    [uncond, no image] — and u + s (c - i) + s_img (i - u) (sd_samplers_cfg_denoiser.py:84-88, 207-209); the image conditioning
    is the unscaled posterior mode (processing.py:321-324).  At image_cfg_scale 1.0 it is ordinary two-way CFG."""
    from oracle import pipeline as opipe
    processing = sub("processing")
    model, om, cond, uncond = _concat_model(8)
    assert model.cond_stage_key == "edit" and model.model.conditioning_key == "hybrid"
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(22)).half().float()
    init = om.vae.encode_first_stage_mean(img * 2 - 1)
    ic = opipe.edit_image_conditioning(om, img * 2 - 1)
    outs = {}
    for s_img in (1.5, 1.0):
        p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=920, batch_size=2, steps=5, cfg_scale=6.0,
                                                        width=128, height=128, sampler_name="Euler a", init_images=img,
                                                        denoising_strength=0.8, image_cfg_scale=s_img)
        res = processing.process_images(p)
        lat = opipe.sample(om, cond, uncond, [920, 921], 5, "euler_a", 6.0, (16, 16), init_latent=init, denoising_strength=0.8,
                           img2img_steps_given=False, image_cond=ic, image_cfg_scale=s_img)
        assert rel_l2(res.latents.cpu(), lat) < 1.5e-2, s_img
        outs[s_img] = lat
    assert rel_l2(outs[1.5], outs[1.0]) > 3e-2


def test_depth2img_checkpoint_conditioning_vs_oracle(dev, monkeypatch):
    """5-channel depth2img checkpoints (LatentDepth2ImageDiffusion, conditioning_key "hybrid"): the host's MiDaS module and its
    ldm.data.util.AddMiDaS input transform (both stubbed here: they are the webui's torch code, run once per job) give a depth map that
    processing.depth2img_image_conditioning resizes to the latent grid (bicubic) and normalises to [-1, 1] over the batch
    (modules/processing.py:304-320); it is the fifth input channel of every UNet row."""
    import sys
    import types
    from oracle import pipeline as opipe
    processing = sub("processing")
    wd = torch.tensor([0.5, -0.3, 0.8])

    class AddMiDaS:                                           # stand-in for ldm.data.util.AddMiDaS("dpt_hybrid"): [-1, 1] HWC -> CHW numpy
        def __init__(self, model_type):
            assert model_type == "dpt_hybrid"

        def __call__(self, sample):
            x = ((sample["jpg"] + 1.0) * .5).detach().cpu().numpy()
            sample["midas_in"] = np.ascontiguousarray(x.transpose(2, 0, 1)).astype(np.float32)
            return sample

    ldm, data, util = types.ModuleType("ldm"), types.ModuleType("ldm.data"), types.ModuleType("ldm.data.util")
    util.AddMiDaS, data.util, ldm.data = AddMiDaS, util, data
    for k, m in (("ldm", ldm), ("ldm.data", data), ("ldm.data.util", util)):
        monkeypatch.setitem(sys.modules, k, m)
    depth_model = lambda t: torch.tanh((t * wd.to(t.device)[None, :, None, None]).sum(1, keepdim=True) * 3.0 + torch.linspace(-1, 1, t.shape[-1], device=t.device))
    model, om, cond, uncond = _concat_model(5, depth_model=depth_model)
    assert model.is_depth2img and model.model.conditioning_key == "hybrid"
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(23)).half().float()
    p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=930, batch_size=2, steps=5, cfg_scale=6.0,
                                                    width=128, height=128, sampler_name="Euler a", init_images=img, denoising_strength=0.8)
    res = processing.process_images(p)
    # the reference's arithmetic on the CPU: the FIRST image's MiDaS input repeated over the batch (:307-309), bicubic, aminmax
    src = img * 2 - 1
    midas_in = ((src[0].permute(1, 2, 0) + 1.0) * .5).permute(2, 0, 1)[None].repeat(2, 1, 1, 1)
    d = torch.nn.functional.interpolate(depth_model(midas_in), size=(16, 16), mode="bicubic", align_corners=False)
    lo, hi = torch.aminmax(d)
    ic = 2. * (d - lo) / (hi - lo) - 1.
    assert tuple(p.image_conditioning_all.shape) == (2, 1, 16, 16) and rel_l2(p.image_conditioning_all.cpu(), ic) < 1e-5
    init = om.vae.encode_first_stage_mean(src)
    lat = opipe.sample(om, cond, uncond, [930, 931], 5, "euler_a", 6.0, (16, 16), init_latent=init, denoising_strength=0.8,
                       img2img_steps_given=False, image_cond=ic)
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2
    flat = opipe.sample(om, cond, uncond, [930, 931], 5, "euler_a", 6.0, (16, 16), init_latent=init, denoising_strength=0.8,
                        img2img_steps_given=False, image_cond=torch.zeros_like(ic))
    assert rel_l2(flat, lat) > 1e-2                           # the depth channel matters
    model.depth_model = None
    with pytest.raises(NotImplementedError):
        processing.process_images(processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=930, batch_size=2, steps=2,
                                                                              width=128, height=128, sampler_name="Euler a", init_images=img))
    model.engine.close()


@pytest.mark.parametrize("and_prompts", [False, True])
def test_unclip_checkpoint_conditioning_vs_oracle(dev, and_prompts):
    """unCLIP checkpoints (SD 2.1-unclip, conditioning_key "crossattn-adm"): c_adm = the host's CLIP image embedder + noise augmentor at level 0
    (modules/processing.py:327-333; stubs here) goes to the UNet's vector input on the cond rows and zeros on the uncond rows
    (modules/sd_samplers_cfg_denoiser.py:192-194; the oracle CFG denoiser is pinned on it, tests/golden/cfg_denoiser.npz "unclip*"); txt2img
    feeds a zero vector of 2 x time_embed.dim (:113-115).  With AND prompts the vector is repeated per sub-prompt."""
    import types
    from oracle import pipeline as opipe, unet as ou, vae as ov
    schema, processing = sub("schema"), sub("processing")
    ucfg, vcfg = schema.tiny_unet(adm_in_channels=24), schema.tiny_vae()
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0x2B7)
    we = torch.randn(3, 12, generator=torch.Generator().manual_seed(31))
    embedder = lambda im: torch.tanh(im.mean(dim=(2, 3)) @ we.to(im.device) * 4.0)
    augment = types.SimpleNamespace(time_embed=types.SimpleNamespace(dim=12))
    noise_augmentor = lambda c, noise_level: (c * 0.9 + 0.01 * noise_level[:, None], torch.sin(3.0 * c))
    noise_augmentor_obj = type("NA", (), {"time_embed": augment.time_embed, "__call__": staticmethod(noise_augmentor)})()
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0, conditioning_key="crossattn-adm", embedder=embedder, noise_augmentor=noise_augmentor_obj)
    assert not model.is_sdxl and model.model.conditioning_key == "crossattn-adm"
    om = opipe.OracleModel(sd, ou.tiny_config(adm_in_channels=24), ov.tiny_vae_config())
    g = torch.Generator().manual_seed(14)
    cond, uncond = torch.randn(3 if and_prompts else 2, 77, 64, generator=g), torch.randn(2, 77, 64, generator=g)
    conds_list = [[(0, 1.0), (1, 0.7)], [(2, 1.0)]] if and_prompts else None
    c_arg = (conds_list, cond) if and_prompts else cond       # what the oracle's CFG denoiser takes
    c_job = cond
    if and_prompts:                                           # ... and the reference's container for the same thing (prompt_parser.py)
        hp = sub("prompt_parser")
        one = lambda i, w: hp.ComposableScheduledPromptConditioning([hp.ScheduledPromptConditioning(99, cond[i])], w)
        c_job = hp.MulticondLearnedConditioning((2,), [[one(0, 1.0), one(1, 0.7)], [one(2, 1.0)]])
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(24)).half().float()
    p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=c_job, uc=uncond, seed=940, batch_size=2, steps=5, cfg_scale=6.0,
                                                    width=128, height=128, sampler_name="Euler a", init_images=img, denoising_strength=0.8)
    res = processing.process_images(p)
    e = embedder(img * 2 - 1)
    c_adm = torch.cat([e * 0.9, torch.sin(3.0 * e)], 1)
    assert tuple(p.image_conditioning_all.shape) == (2, 24) and rel_l2(p.image_conditioning_all.cpu(), c_adm) < 1e-5
    init = om.vae.encode_first_stage_mean(img * 2 - 1)
    y = c_adm if not and_prompts else torch.stack([c_adm[0], c_adm[0], c_adm[1]])
    lat = opipe.sample(om, c_arg, uncond, [940, 941], 5, "euler_a", 6.0, (16, 16), init_latent=init, denoising_strength=0.8,
                       img2img_steps_given=False, y=y, uy=torch.zeros_like(c_adm))
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2
    same_uy = opipe.sample(om, c_arg, uncond, [940, 941], 5, "euler_a", 6.0, (16, 16), init_latent=init, denoising_strength=0.8,
                           img2img_steps_given=False, y=y, uy=c_adm)
    assert rel_l2(same_uy, lat) > 1e-2                        # zeros on the uncond rows, not the embedding
    if not and_prompts:                                       # txt2img: zero c_adm of 2 x time_embed.dim
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=950, batch_size=2, steps=4, cfg_scale=6.0,
                                                        width=128, height=128, sampler_name="Euler a")
        res = processing.process_images(p)
        z = torch.zeros(2, 24)
        lat = opipe.sample(om, cond, uncond, [950, 951], 4, "euler_a", 6.0, (16, 16), y=z, uy=z)
        assert rel_l2(res.latents.cpu(), lat) < 1e-2
    model.engine.close()


def test_img2img_masked_content_fills_and_noise_multiplier(dev, tiny):
    """inpainting_fill 2 / 3 ("latent noise" / "latent nothing", processing.py:1747-1753) rewrite the masked part of the init
    latent before sampling; initial_noise_multiplier scales the img2img noise (:1762-1764)."""
    from oracle import pipeline as opipe
    from oracle.rng import ImageRNG as ORNG
    processing = sub("processing")
    model, om = tiny["model"], tiny["oracle"]
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(23)).half().float()
    mask = torch.zeros(2, 4, 16, 16)
    mask[:, :, 3:11, 5:14] = 1.0
    init = om.vae.encode_first_stage_mean(img * 2 - 1)
    for fill in (2, 3):
        p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=3100, batch_size=2, steps=5, cfg_scale=7.0,
                                                        width=128, height=128, sampler_name="Euler a", init_images=img,
                                                        denoising_strength=0.6, latent_mask=mask, inpainting_fill=fill)
        res = processing.process_images(p)
        filled = init * mask + (ORNG((4, 16, 16), [3100, 3101]).next() * (1 - mask) if fill == 2 else 0.0)
        lat = opipe.sample(om, cond, uncond, [3100, 3101], 5, "euler_a", 7.0, (16, 16), init_latent=filled, denoising_strength=0.6,
                           img2img_steps_given=False, mask=mask)
        assert rel_l2(res.latents.cpu(), lat) < 1.5e-2, fill
    p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=3100, batch_size=2, steps=5, cfg_scale=7.0,
                                                    width=128, height=128, sampler_name="Euler a", init_images=img,
                                                    denoising_strength=0.6, initial_noise_multiplier=1.1)
    res = processing.process_images(p)
    lat = opipe.sample(om, cond, uncond, [3100, 3101], 5, "euler_a", 7.0, (16, 16), init_latent=init, denoising_strength=0.6,
                       img2img_steps_given=False, noise_multiplier=1.1)
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2


def test_prompt_editing_and_composition_containers_vs_oracle(dev, tiny):
    """The reference's conditioning containers straight into the sampler: p.c = MulticondLearnedConditioning
    with prompt-editing schedules and an AND-ed sub-prompt of twice the token count, p.uc = per-image schedules; the denoiser
    reconstructs them per step (modules/sd_samplers_cfg_denoiser.py:169-170) and re-projects K / V only when the selection changes."""
    from oracle import pipeline as opipe, prompt_cond as opc, kdiffusion as okd
    hp, processing, ss = sub("prompt_parser"), sub("processing"), sub("sd_samplers")
    g = torch.Generator().manual_seed(55)
    T = lambda tokens=77: torch.randn(tokens, 64, generator=g)
    S = hp.ScheduledPromptConditioning
    c0a, c0b, c1a, c1b1, c1b2, u0, u1a, u1b = T(), T(), T(), T(154), T(154), T(154), T(154), T(154)
    c = hp.MulticondLearnedConditioning((2,), [
        [hp.ComposableScheduledPromptConditioning([S(2, c0a), S(6, c0b)], 1.0)],
        [hp.ComposableScheduledPromptConditioning([S(6, c1a)], 1.0), hp.ComposableScheduledPromptConditioning([S(3, c1b1), S(6, c1b2)], 0.6)]])
    uc = [[S(6, u0)], [S(1, u1a), S(6, u1b)]]
    calls = []
    eng = tiny["model"].engine
    orig_set = eng.set_context
    eng.set_context = lambda ctx: (calls.append(tuple(ctx.shape)), orig_set(ctx))[1]
    try:
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=c, uc=uc, seed=5000, batch_size=2, steps=6, cfg_scale=6.0,
                                                        width=128, height=128, sampler_name="Euler")
        res = processing.process_images(p)
    finally:
        eng.set_context = orig_set
    assert len(calls) == 4 and all(s == (5, 154, 64) for s in calls)      # the selection changes at steps 2 (uncond), 3 and 4 (cond)

    batch = [[opc.Composable([opc.Scheduled(e.end_at_step, e.cond) for e in cp.schedules], cp.weight) for cp in img] for img in c.batch]
    unc = [[opc.Scheduled(e.end_at_step, e.cond) for e in sch] for sch in uc]
    om = tiny["oracle"]
    wrap = okd.CompVisDenoiser(lambda xi, t, cc: om.apply_model(xi, t, cc), om.alphas_cumprod)
    cfg = okd.CFGDenoiser(wrap)

    def model(x, sigma, **kw):                                            # the reference reconstructs inside forward, per step
        step = cfg.step
        u = opc.reconstruct_cond_batch(unc, step)
        pair = opc.reconstruct_multicond_batch(batch, step)
        return cfg(x, sigma, u, pair, 6.0)
    from oracle.rng import ImageRNG as ORNG
    sig = wrap.get_sigmas(6)
    x = ORNG((4, 16, 16), [5000, 5001]).next() * sig[0]
    lat = okd.sample_euler(model, x, sig, {})
    assert rel_l2(res.latents.cpu(), lat) < 1e-2


def test_txt2img_batch_split_matches(dev, tiny):
    """Sharding contract of the multi-GPU runner: images [0,4) generated as 4, as 2+2 (n_iter) or as the tail pair are the
    same images — per-image Philox streams (modules/rng.py:108) + per-image arithmetic everywhere.  Bitwise when the per-call
    batch size is equal (same tile configuration), to fp16 rounding otherwise."""
    processing = sub("processing")
    def run(c, uc, seed, bs, n_iter=1):
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=c, uc=uc, seed=seed, batch_size=bs, n_iter=n_iter,
                                                        steps=3, cfg_scale=5.0, width=128, height=128, sampler_name="Euler a")
        return processing.process_images(p).latents.cpu()
    full = run(tiny["cond"], tiny["uncond"], 1000, 4)
    split = run(tiny["cond"], tiny["uncond"], 1000, 2, n_iter=2)
    tail = run(tiny["cond"][2:], tiny["uncond"][2:], 1002, 2)
    assert rel_l2(split, full) < 1e-2 and rel_l2(tail, full[2:]) < 1e-2
    assert torch.equal(tail, split[2:])                       # same batch size (2) => same bits, whatever the batch position


def test_img2img_and_hires_paths_vs_oracle(dev, tiny):
    from oracle import pipeline as opipe
    processing = sub("processing")
    model, om = tiny["model"], tiny["oracle"]
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    # plain img2img: no explicit steps -> t_enc = int(0.75 * steps) (modules/sd_samplers_common.py:28-29)
    img = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(9))     # tiny VAE: /2 -> 16x16 latent
    p = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=2000, batch_size=2, steps=4, cfg_scale=7.0,
                                                    width=128, height=128, sampler_name="Euler a", init_images=img,
                                                    denoising_strength=0.75)
    res = processing.process_images(p)
    init = om.vae.encode_first_stage_mean(img.half().float() * 2 - 1)
    lat = opipe.sample(om, cond, uncond, [2000, 2001], 4, "euler_a", 7.0, (16, 16), init_latent=init, denoising_strength=0.75,
                       img2img_steps_given=False)
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2
    # txt2img + latent hires fix x2: second pass is sample_img2img with steps given (26/19-style arithmetic)
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=3000, batch_size=2, steps=4, cfg_scale=7.0,
                                                    width=64, height=64, sampler_name="Euler a", enable_hr=True, hr_scale=2.0,
                                                    denoising_strength=0.75)
    res = processing.process_images(p)
    lat = opipe.txt2img_hires(om, cond, uncond, [3000, 3001], 4, "euler_a", 7.0, (8, 8), hr_scale=2.0, denoising_strength=0.75)
    assert res.latents.shape == lat.shape == (2, 4, 16, 16)
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2


@pytest.mark.parametrize("upscaler,kw", [("Lanczos", {}), ("Nearest", {}), ("None", {}), ("Lanczos", {"hr_resize_x": 160, "hr_resize_y": 128})])
def test_hires_fix_image_space_upscaler_vs_oracle(dev, upscaler, kw):
    """Non-latent hires fix (modules/processing.py:1353-1354, 1400-1427): decode -> uint8 PIL -> images.resize_image -> encode ->
    truncate -> second pass, with an 8x first stage so the image and latent sizes relate as in the real models."""
    from oracle import pipeline as opipe, unet as ou, vae as ov
    schema, processing = sub("schema"), sub("processing")
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae(ch_mult=(1, 1, 2, 2))
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0x77)
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0)
    om = opipe.OracleModel(sd, ou.tiny_config(), ov.tiny_vae_config(ch_mult=(1, 1, 2, 2)))
    g = torch.Generator().manual_seed(14)
    cond, uncond = torch.randn(2, 77, 64, generator=g), torch.randn(2, 77, 64, generator=g)
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=3300, batch_size=2, steps=4, cfg_scale=5.0,
                                                    width=64, height=64, sampler_name="Euler a", enable_hr=True, hr_scale=2.0,
                                                    denoising_strength=0.6, hr_upscaler=upscaler, **kw)
    res = processing.process_images(p)
    lat = opipe.txt2img_hires_image(om, cond, uncond, [3300, 3301], 4, "euler_a", 5.0, 64, 64, hr_scale=2.0, denoising_strength=0.6,
                                    upscaler=upscaler, **kw)
    assert res.latents.shape == lat.shape == ((2, 4, 16, 20) if kw else (2, 4, 16, 16))
    # the uint8 quantisation of the decoded first pass can flip a level where the engine and the oracle differ by rounding
    assert rel_l2(res.latents.cpu(), lat) < 2e-2, upscaler
    assert res.images[0].shape == ((128, 160, 3) if kw else (128, 128, 3))


@pytest.mark.parametrize("sampler,name,by_steps", [("euler_a", "Euler a", False), ("ddim", "DDIM", False), ("dpmpp_2m", "DPM++ 2M", True)])
def test_refiner_switch_vs_oracle(dev, tiny, sampler, name, by_steps):
    """p.refiner_checkpoint / refiner_switch_at (modules/sd_samplers_common.py:158-202): from the switch point on the second,
    resident checkpoint and ITS conds drive the same sampler loop; the final decode uses the refiner's first stage."""
    from oracle import pipeline as opipe, unet as ou, vae as ov
    schema, processing, shared = sub("schema"), sub("processing"), sub("shared")
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae()
    sd2 = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16, seed=0xBEEF)
    refiner = sub("sd_models").SdModel(sd2, ucfg, vcfg, device=0)
    om2 = opipe.OracleModel(sd2, ou.tiny_config(), ov.tiny_vae_config())
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]
    g = torch.Generator().manual_seed(99)
    rc, ruc = torch.randn(2, 77, 64, generator=g), torch.randn(2, 77, 64, generator=g)
    keep = shared.opts.refiner_switch_by_sample_steps
    shared.opts.refiner_switch_by_sample_steps = by_steps
    try:
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=tiny["model"], c=cond, uc=uncond, seed=4000, batch_size=2, steps=8,
                                                        cfg_scale=6.0, width=128, height=128, sampler_name=name,
                                                        refiner_sd_model=refiner, refiner_switch_at=0.5, refiner_c=rc, refiner_uc=ruc)
        res = processing.process_images(p)
    finally:
        shared.opts.refiner_switch_by_sample_steps = keep
    assert shared.sd_model is tiny["model"]
    ref = dict(model=om2, cond=rc, uncond=ruc, switch_at=0.5, by_sample_steps=by_steps)
    lat = opipe.sample(tiny["oracle"], cond, uncond, [4000, 4001], 8, sampler, 6.0, (16, 16), refiner=ref)
    base_only = opipe.sample(tiny["oracle"], cond, uncond, [4000, 4001], 8, sampler, 6.0, (16, 16))
    assert rel_l2(res.latents.cpu(), lat) < 1.5e-2 and rel_l2(base_only, lat) > 5e-2
    u8 = opipe.to_uint8_hwc(opipe.decode(om2, lat))
    assert np.abs(np.stack(res.images).astype(np.int32) - u8.astype(np.int32)).mean() < 2.5


def test_sd15_full_size_unet_single_forward_vs_oracle(dev):
    """The real SD1.5 architecture (859,520,964 parameters), 32x32 latent, batch 2: one forward vs the fp32 oracle."""
    schema = sub("schema")
    from oracle import unet as ou
    cfg = schema.sd15_unet()
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    net = ou.build_unet(ou.sd15_config(), sd)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    x = seeded((2, 4, 32, 32), 1)
    t = torch.tensor([981.0, 211.5])
    ctx = seeded((2, 77, 768), 2)
    torch.set_num_threads(max(1, torch.get_num_threads()))
    with torch.no_grad():
        ref = net(x, t, ctx.half().float())
    got = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev))
    torch.cuda.synchronize()
    assert rel_l2(got.cpu(), ref) < 5e-3
    eng.close()


def test_sdxl_shaped_unet_vs_oracle(dev):
    """SDXL-style UNet features (configs/sd_xl_inpaint.yaml:19-37; modules/sd_models_xl.py:12-43): vector conditioning y ->
    label_emb, Linear proj_in/proj_out, per-level transformer depth > 1, head size 64, no attention at level 0."""
    schema = sub("schema")
    from oracle import unet as ou
    kw = dict(model_channels=64, channel_mult=(1, 2, 4), num_res_blocks=2, attention_resolutions=(2, 4), num_heads=-1,
              num_head_channels=64, transformer_depth=(1, 2, 3), context_dim=128, use_linear_in_transformer=True,
              adm_in_channels=192)
    cfg = schema.UNetConfig(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    net = ou.build_unet(ou.UNetConfig(**kw), sd)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    x, t = seeded((2, 4, 32, 32), 1), torch.tensor([911.0, 45.5])
    ctx, y = seeded((2, 77, 128), 2), seeded((2, 192), 3)
    with torch.no_grad():
        ref = net(x, t, ctx.half().float(), y)
    got = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev), y.to(dev))
    torch.cuda.synchronize()
    assert rel_l2(got.cpu(), ref) < 5e-3
    eng.close()


@pytest.mark.parametrize("s_min_uncond", [0.0, 20.0])
def test_sdxl_shaped_sampling_with_vector_conditioning_vs_oracle(dev, s_min_uncond):
    """C3-shaped path at test size: the SDXL vector conditioning (y | uy -> label_emb) travels through sampler_extra_args and the
    CFG denoiser for every UNet row, also when skip-uncond drops the uncond rows (and their uy) on alternate steps."""
    from oracle import pipeline as opipe, unet as ou
    schema, processing = sub("schema"), sub("processing")
    kw = dict(model_channels=64, channel_mult=(1, 2, 4), num_res_blocks=2, attention_resolutions=(2, 4), num_heads=-1,
              num_head_channels=64, transformer_depth=(1, 2, 3), context_dim=128, use_linear_in_transformer=True,
              adm_in_channels=192)
    cfg = schema.UNetConfig(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    model = sub("sd_models").SdModel(sd, cfg, None, device=0, load_vae=False)
    assert model.is_sdxl
    om = opipe.OracleModel(sd, ou.UNetConfig(**kw), None)
    g = torch.Generator().manual_seed(15)
    cond, uncond = torch.randn(2, 77, 128, generator=g), torch.randn(2, 77, 128, generator=g)
    y, uy = torch.randn(2, 192, generator=g), torch.randn(2, 192, generator=g)
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond, uc=uncond, seed=600, batch_size=2, steps=5, cfg_scale=5.0,
                                                    width=256, height=256, sampler_name="Euler a", s_min_uncond=s_min_uncond)
    p.y, p.uy = y.to(dev), uy.to(dev)
    p.rng = sub("rng").ImageRNG((4, 32, 32), [600, 601], device=dev)
    p.seeds = [600, 601]
    sampler_obj = sub("sd_samplers").create_sampler("Euler a", model)
    got = sampler_obj.sample(p, p.rng.next(), cond.to(dev), uncond.to(dev))
    lat = opipe.sample(om, cond, uncond, [600, 601], 5, "euler_a", 5.0, (32, 32), y=y, uy=uy, s_min_uncond=s_min_uncond)
    assert rel_l2(got.cpu(), lat) < 1e-2
    model.engine.close()


def test_c0_shape_sd15_256px_b1_euler_a_5_steps(dev):
    """BASELINE.json configs[0]: SD1.5 txt2img 256x256, 5-step Euler-a, batch 1 — full architecture, final latent vs oracle."""
    schema, processing = sub("schema"), sub("processing")
    from oracle import pipeline as opipe, unet as ou
    cfg = schema.sd15_unet()
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    model = sub("sd_models").SdModel(sd, cfg, None, device=0, load_vae=False)
    om = opipe.OracleModel(sd, ou.sd15_config(), None)
    g = torch.Generator().manual_seed(21)
    cond, uncond = torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)
    sampler = sub("sd_samplers").create_sampler("Euler a", model)

    class P:
        steps, cfg_scale, eta, scheduler, is_hr_pass = 5, 7.0, None, None, False
        sampler_noise_scheduler_override, extra_generation_params = None, {}
        rng = sub("rng").ImageRNG((4, 32, 32), [1000], device=dev)
    p = P()
    got = sampler.sample(p, p.rng.next(), cond.to(dev), uncond.to(dev))
    ref = opipe.sample(om, cond, uncond, [1000], 5, "euler_a", 7.0, (32, 32))
    assert rel_l2(got.cpu(), ref) < 1e-2
    model.engine.close()


def test_nan_check_and_vae_range_extended_retry(dev, tiny):
    """modules/processing.py:625-672 + modules/devices.py:236-265: NaN latents raise NansException("... Unet"); a decoder whose fp16
    activations overflow (the real SD VAEs do on some images — why the reference re-runs the VAE in fp32 / bf16) produces a NaN
    image, which triggers the engine's equivalent of that fallback: the range-extended decode (residual stream at 1/64 scale),
    whose result matches the fp32 oracle; with opts.auto_vae_precision off the NansException propagates."""
    from oracle import vae as ov
    schema, processing, shared, devices = sub("schema"), sub("processing"), sub("shared"), sub("devices")
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae()
    sd = dict(tiny["sd"])
    key = schema.VAE_PREFIX + "decoder.mid.block_1.conv2.weight"
    sd[key] = (sd[key].float() * 2.0e5).half()              # residual stream ~1e5 and beyond after this block: past fp16's 65504
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0)
    okl = ov.build_vae(ov.tiny_vae_config(), sd)
    z = (seeded((2, 4, 16, 16), 8) * 0.18215 * 4).to(dev)
    with torch.no_grad():
        ref = okl.decode_first_stage(z.cpu())
    assert torch.isfinite(ref).all()
    plain = model.decode_first_stage(z)
    assert torch.isnan(plain).any()                          # fp16 storage overflowed -> inf -> NaN after the next GroupNorm
    with pytest.raises(devices.NansException, match="Unet"):
        processing.decode_latent_batch(model, torch.full_like(z, float("nan")), check_for_nans=True)
    keep = shared.opts.auto_vae_precision
    try:
        shared.opts.auto_vae_precision = False
        with pytest.raises(devices.NansException, match="VAE"):
            processing.decode_latent_batch(model, z, check_for_nans=True)
        shared.opts.auto_vae_precision = True
        out = processing.decode_latent_batch(model, z, check_for_nans=True)
    finally:
        shared.opts.auto_vae_precision = keep
    assert model.vae_range_extended and torch.isfinite(out).all()
    assert rel_l2(out.cpu(), ref) < 5e-3
    # on an ordinary checkpoint the range-extended decode is the same function to fp16 rounding
    m2 = tiny["model"]
    a = m2.decode_first_stage(z)
    m2.set_vae_range_extended(True)
    try:
        b = m2.decode_first_stage(z)
    finally:
        m2.set_vae_range_extended(False)
    assert rel_l2(b.cpu(), a.cpu()) < 3e-3
    model.engine.close()


def test_tiling_circular_padding_unet_and_vae_vs_oracle(dev, tiny):
    """p.tiling (modules/processing.py:879-895 -> sd_hijack.apply_circular): every Conv2d of the UNet and the VAE switches to
    padding_mode='circular'.  Oracle = the same torch modules with that attribute set, exactly what the reference does."""
    import copy
    processing = sub("processing")
    model, om = tiny["model"], tiny["oracle"]
    unet_c, vae_c = copy.deepcopy(om.unet), copy.deepcopy(om.vae)
    for net in (unet_c, vae_c):
        for layer in net.modules():
            if type(layer) == torch.nn.Conv2d:
                layer.padding_mode = "circular"
                layer._reversed_padding_repeated_twice = torch.nn.modules.utils._reverse_repeat_tuple(layer.padding, 2)
    x, t, ctx = seeded((2, 4, 16, 16), 21), torch.tensor([640.0, 77.0]), tiny["cond"][:2]
    z = seeded((2, 4, 16, 16), 22) * 0.8
    with torch.no_grad():
        ref_u = unet_c(x, t, ctx.half().float())
        ref_v = vae_c.decode_first_stage(z)
        plain_u = om.unet(x, t, ctx.half().float())
    eng = model.engine
    eng.set_option("tiling", 1)
    try:
        got_u = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev))
        got_v = model.decode_first_stage(z.to(dev))
    finally:
        eng.set_option("tiling", 0)
    assert rel_l2(got_u.cpu(), ref_u) < 5e-3 and rel_l2(got_v.cpu(), ref_v) < 5e-3
    assert rel_l2(plain_u, ref_u) > 2e-2
    # through process_images: p.tiling switches it on for the job and the next job (tiling None -> opts.tiling False) off again
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=tiny["cond"][:1], uc=tiny["uncond"][:1], seed=9, batch_size=1, steps=2,
                                                    cfg_scale=3.0, width=128, height=128, sampler_name="Euler", tiling=True)
    a = processing.process_images(p).latents
    p2 = processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=tiny["cond"][:1], uc=tiny["uncond"][:1], seed=9, batch_size=1, steps=2,
                                                     cfg_scale=3.0, width=128, height=128, sampler_name="Euler")
    b = processing.process_images(p2).latents
    assert not torch.equal(a, b)


def _hn_state(dims, ls, act, ln, ao, ds, seed, name):
    """A hypernetwork file's content (what torch.load returns, modules/hypernetworks/hypernetwork.py:246-300) with seeded weights."""
    from oracle import hypernetwork as ohn
    from helpers import seeded_module_weights
    sd = {"layer_structure": ls, "activation_func": act, "is_layer_norm": ln, "activate_output": ao, "dropout_structure": ds, "name": name}
    for j, dim in enumerate(dims):
        pair = []
        for w in (0, 1):
            m = ohn.HypernetworkModule(dim, None, ls, act, ln, ao, ds)
            seeded_module_weights(m, seed + 10 * j + w)
            with torch.no_grad():
                for p in m.parameters():                     # trained hypernetworks are small perturbations of the identity map
                    if p.dim() == 2:
                        p.mul_(0.5)
            pair.append({k: v.clone() for k, v in m.state_dict().items()})
        sd[dim] = tuple(pair)
    return sd


def test_hypernetworks_in_engine_vs_oracle(dev, tiny):
    """shared.loaded_hypernetworks inside the engine's attention layers (modules/hypernetworks/hypernetwork.py:358-379): two
    networks chained, modules for the self-attention widths (64, 128) and the text-context width (64 in the tiny model), different
    structures (activation, LayerNorm, activate_output, dropout index shift), multipliers; unloading restores the original bits."""
    from oracle import hypernetwork as ohn, unet as ou
    hn_mod = sub("hypernetwork")
    model, om = tiny["model"], tiny["oracle"]
    eng = model.engine
    x, t, ctx = seeded((2, 4, 16, 16), 61).to(dev), torch.tensor([650.0, 40.0], device=dev), seeded((2, 77, 64), 62).to(dev)

    def fwd():
        eng.set_context(ctx)
        return eng.unet_forward(x, t, None, None).float().cpu()
    base = fwd()
    a = _hn_state([64, 128], [1, 2, 1], "relu", False, False, None, 7000, "hn_a")
    b = _hn_state([64], [1, 2, 2, 1], "swish", True, True, [0, 0.3, 0.3, 0], 7100, "hn_b")
    try:
        loaded = hn_mod.load_hypernetworks(model, [a, b], [0.8, 0.5])
        assert [h.name for h in loaded] == ["hn_a", "hn_b"] and loaded[0].multiplier == 0.8
        got = fwd()
        ou.LOADED_HYPERNETWORKS[:] = [ohn.Hypernetwork(a, 0.8), ohn.Hypernetwork(b, 0.5)]
        with torch.no_grad():
            ref = om.unet(x.cpu(), t.cpu(), ctx.cpu().half().float())
        assert rel_l2(got, ref) < 8e-3 and rel_l2(got, base) > 3e-2
        # the SdUnet adapter's device-side context cache must not skip the hypernetwork pass over the text context
        eng.set_context_cached(ctx)
        assert torch.equal(eng.unet_forward(x, t, None, None).float().cpu(), got)
    finally:
        ou.LOADED_HYPERNETWORKS[:] = []
        hn_mod.load_hypernetworks(model, [], [])
    assert torch.equal(fwd(), base)


def test_a_forward_refused_in_its_sizing_walk_leaves_the_engine_usable(dev, tiny):
    """A forward is one walk twice (csrc/engine.cpp two_pass): dry to size the arena, then the launches.  A hypernetwork module whose last
    linear does not return to its width — only the C ABI lets one in, hypernetwork.py refuses such a file — is refused by the self-attention
    of that width inside the dry walk: the call fails before anything is launched.  With the hypernetworks cleared the same call gives the
    bits it gave before."""
    import ctypes
    import json
    lib, hn_mod = sub("_lib"), sub("hypernetwork")
    model = tiny["model"]
    eng = model.engine
    x, t, ctx = seeded((2, 4, 16, 16), 61).to(dev), torch.tensor([650.0, 40.0], device=dev), seeded((2, 77, 64), 62).to(dev)

    def fwd():
        eng.set_context(ctx)
        return eng.unet_forward(x, t, None, None).float().cpu()
    base = fwd()
    w, b = torch.zeros((64, 128)), torch.zeros(64)               # 128 -> 64 as the whole K module of width 128 (the text context is 64 wide)
    try:
        lib.check(lib.lib.sdmi_unet_hypernet_begin(eng.handle, 1.0), "hypernet_begin")
        lib.check(lib.lib.sdmi_unet_hypernet_linear(eng.handle, 128, 0, w.data_ptr(), b.data_ptr(), lib.F32, 64, 128, 0), "hypernet_linear")
        eng.set_context(ctx)
        lib.check(lib.lib.sdmi_profile_begin(), "profile_begin")
        with pytest.raises(lib.SdmiError, match="hypernetwork output width must equal its input width"):
            eng.unet_forward(x, t, None, None)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.check(lib.lib.sdmi_profile_end(buf, len(buf)), "profile_end")
        assert json.loads(buf.value.decode())["kernels"] == []   # refused in the dry walk: nothing was launched
    finally:
        hn_mod.load_hypernetworks(model, [], [])
    assert torch.equal(fwd(), base)


def test_arena_reuse_gives_the_same_bits(dev, tiny):
    """Engine option "arena_reuse": the temporaries of every ResBlock / transformer block are released when the block returns and the next
    block's launches write over them (same stream: ordered behind every reader).  Only addresses change — UNet forward (tiny, and an
    SDXL-shaped one with two transformer blocks per level: the ping-pong buffers), VAE decode and a whole sampled job must give the
    bits of the bump-only arena, call after call."""
    processing, schema = sub("processing"), sub("schema")
    model = tiny["model"]
    eng = model.engine
    x, t, ctx = seeded((4, 4, 16, 16), 1).to(dev), torch.tensor([999.0, 500.25, 37.5, 1.0], device=dev), tiny["cond"].to(dev)
    z = seeded((2, 4, 16, 16), 5).to(dev)

    def run_all(e, xx, tt, cc, yy=None):
        e.set_context(cc)
        return e.unet_forward(xx, tt, None, yy).clone()
    base_u, base_v = run_all(eng, x, t, ctx), model.decode_first_stage(z).clone()
    job = lambda: processing.process_images(processing.StableDiffusionProcessingTxt2Img(
        sd_model=model, c=tiny["cond"][:2], uc=tiny["uncond"][:2], seed=31, batch_size=2, steps=4, cfg_scale=5.0, width=128, height=128, sampler_name="Euler a"))
    base_imgs = job().images
    ucfg2 = schema.tiny_unet(transformer_depth=2)
    sd2 = schema.synthetic_state_dict(ucfg2, None, dtype=torch.float16, seed=0x51)
    m2 = sub("sd_models").SdModel(sd2, ucfg2, None, device=0, load_vae=False)
    base_u2 = run_all(m2.engine, x, t, ctx)
    try:
        eng.set_option("arena_reuse", 1); m2.engine.set_option("arena_reuse", 1)
        for _ in range(2):
            assert torch.equal(run_all(eng, x, t, ctx), base_u)
            assert torch.equal(model.decode_first_stage(z), base_v)
            assert torch.equal(run_all(m2.engine, x, t, ctx), base_u2)
        assert all(np.array_equal(a, b) for a, b in zip(job().images, base_imgs))
    finally:
        eng.set_option("arena_reuse", 0); m2.engine.set_option("arena_reuse", 0)
    assert torch.equal(run_all(eng, x, t, ctx), base_u)


def test_hypernetwork_with_layernorm_at_sd15_widths(dev):
    """The widths a real SD1.5 hypernetwork carries (320 / 768 / 1280; 640 has the same code path as 320) with the default [1, 2, 1]
    structure AND LayerNorm: the hidden layer of the 1280-wide modules is 2560 wide — LayerNorm rows the engine used to reject — on a
    two-level UNet with those channel counts (320 -> 1280, text context 768) against the oracle's HypernetworkModule chain."""
    from oracle import hypernetwork as ohn, pipeline as opipe, unet as ou
    schema, hn_mod = sub("schema"), sub("hypernetwork")
    kw = dict(model_channels=320, channel_mult=(1, 4), context_dim=768)
    ucfg = schema.tiny_unet(**kw)
    sd = schema.synthetic_state_dict(ucfg, None, dtype=torch.float16, seed=0x4A11)
    model = sub("sd_models").SdModel(sd, ucfg, None, device=0, load_vae=False)
    om = opipe.OracleModel(sd, ou.tiny_config(**kw), None)
    eng = model.engine
    x, t, ctx = seeded((2, 4, 8, 8), 81).to(dev), torch.tensor([700.0, 90.0], device=dev), seeded((2, 77, 768), 82).to(dev)

    def fwd():
        eng.set_context(ctx)
        return eng.unet_forward(x, t, None, None).float().cpu()
    base = fwd()
    hn = _hn_state([320, 768, 1280], [1, 2, 1], "relu", True, False, None, 7300, "hn_sd15_widths")
    try:
        hn_mod.load_hypernetworks(model, [hn], [0.3])
        got = fwd()
        ou.LOADED_HYPERNETWORKS[:] = [ohn.Hypernetwork(hn, 0.3)]
        with torch.no_grad():
            ref = om.unet(x.cpu(), t.cpu(), ctx.cpu().half().float())
        assert rel_l2(got, ref) < 8e-3 and rel_l2(got, base) > 2e-2, (rel_l2(got, ref), rel_l2(got, base))
    finally:
        ou.LOADED_HYPERNETWORKS[:] = []
        hn_mod.load_hypernetworks(model, [], [])
    assert torch.equal(fwd(), base)


def test_sharded_job_replayed_rank_by_rank_equals_the_single_process_job(dev, tiny):
    """SURVEY.md section 8e on ONE GPU with the REAL engine: parallel.process_images_sharded(p, world=2, rank=r) for r = 0, 1 run one
    after the other in this process — what rank r of a 2-GPU job computes — and concatenated must be BIT-identical to the single-process
    job at the same per-call batch size (global seeds, per-image generators, per-image CFG combine and decode): tiny model incl. a hires
    job and a ragged split, then a C1-shaped full-size SD1.5 job (512x512, batch 2 x 2 iterations, 3 steps)."""
    par, processing, schema = sub("parallel"), sub("processing"), sub("schema")

    def check(model, cond, uncond, bs, n_iter, world=2, **kw):
        n = bs * n_iter
        mk = lambda: processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond[:n], uc=uncond[:n], seed=4321, batch_size=bs, n_iter=n_iter,
                                                                 cfg_scale=6.0, sampler_name="Euler a", **kw)
        whole = processing.process_images(mk())
        parts = [par.process_images_sharded(mk(), world=world, rank=r) for r in range(world)]
        imgs = [im for part in parts for im in part.images]
        assert [part.shard for part in parts] == [par.shard_range(n, world, r) for r in range(world)]
        assert len(imgs) == len(whole.images) == n
        for i, (a, b) in enumerate(zip(imgs, whole.images)):
            assert np.array_equal(a, b), (bs, n_iter, world, i, kw.get("enable_hr", False))
        return whole

    g = torch.Generator().manual_seed(13)
    cond, uncond = torch.randn(6, 77, 64, generator=g), torch.randn(6, 77, 64, generator=g)
    check(tiny["model"], cond, uncond, 2, 2, steps=3, width=128, height=128)
    check(tiny["model"], cond, uncond, 1, 4, steps=3, width=128, height=128)
    check(tiny["model"], cond, uncond, 2, 3, world=3, steps=2, width=128, height=128)
    w = check(tiny["model"], cond, uncond, 1, 2, steps=2, width=64, height=64, enable_hr=True, hr_scale=2.0, hr_upscaler="Latent", denoising_strength=0.6)
    assert w.images[0].shape[:2] == (32, 32)                  # 64 / 8 = 8x8 latent, hires x2 = 16x16, the two-level tiny VAE decodes x2
    ucfg, vcfg = schema.sd15_unet(), schema.sd15_vae()
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16)
    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0, vae_decoder_only=True)
    del sd
    try:
        c, uc = torch.randn(4, 77, 768, generator=g), torch.randn(4, 77, 768, generator=g)
        check(model, c, uc, 2, 2, steps=3, width=512, height=512)
    finally:
        model.engine.close()
        sub("shared").sd_model = tiny["model"]


def test_one_process_device_pool_reproduces_the_single_device_job(dev, tiny):
    """SURVEY.md section 8e, the form a webui needs (ONE process behind queue_lock, modules/call_queue.py:8-13, driving N devices with one
    host thread per device): parallel.DevicePool keeps an engine per device — replicas packed from the first model's checkpoint dict — and
    cuts the job as shard_job does.  The boxes this suite runs on have one GPU, so the pool gets that device TWICE: two engines, two worker
    threads launching concurrently on two streams of one device (the threads, the per-thread device binding, the replica packing and the
    merge are what is under test; serial workers under the host-emulated tier, whose "device" is not re-entrant).  The merged job must be
    the single-device job image for image and bit for bit — through the pool directly and through process_images with opts.mi355x_devices."""
    par, processing, shared = sub("parallel"), sub("processing"), sub("shared")
    serial = os.environ.get("SDMI_HOSTEMU") == "1"
    g = torch.Generator().manual_seed(17)
    cond, uncond = torch.randn(6, 77, 64, generator=g), torch.randn(6, 77, 64, generator=g)
    model = tiny["model"]

    def mk(bs, n_iter, **kw):
        n = bs * n_iter
        return processing.StableDiffusionProcessingTxt2Img(sd_model=model, c=cond[:n], uc=uncond[:n], seed=777, batch_size=bs, n_iter=n_iter,
                                                           cfg_scale=6.0, sampler_name="Euler a", steps=3, **kw)
    pool = par.DevicePool(model, [0, 0], serial=serial)
    try:
        assert pool.replica(model, 0) is model and pool.replica(model, 1) is not model and pool.replica(model, 1).engine.handle != model.engine.handle
        assert [m.engine.handle for m in pool.for_each_model(lambda m: None)] == [model.engine.handle, pool.replica(model, 1).engine.handle]
        assert shared.sd_model is model                        # the replica's constructor did not take over the reference's global
        cases = ((2, 2, dict(width=64, height=64)), (1, 3, dict(width=64, height=64)),
                 (1, 2, dict(width=64, height=64, enable_hr=True, hr_scale=2.0, hr_upscaler="Latent", denoising_strength=0.6)))
        for bs, n_iter, kw in (cases[:1] if serial else cases):      # (the emulated tier runs one case here and the entry-point case below: host time)
            whole = processing.process_images_one_device(mk(bs, n_iter, **kw))
            pooled = pool.process_images(mk(bs, n_iter, **kw))
            assert len(pooled.images) == len(whole.images) == bs * n_iter and pooled.all_seeds == whole.all_seeds and pooled.shard == (0, bs * n_iter)
            for i, (a, b) in enumerate(zip(pooled.images, whole.images)):
                assert np.array_equal(a, b), (bs, n_iter, i)
            assert torch.equal(pooled.latents.cpu(), whole.latents.cpu())
        # the same through the entry point, switched by the option
        shared.opts.mi355x_devices, shared.opts.mi355x_devices_serial = "0,0", serial
        try:
            whole = processing.process_images_one_device(mk(2, 2, width=64, height=64))
            via_opts = processing.process_images(mk(2, 2, width=64, height=64))
        finally:
            shared.opts.mi355x_devices, shared.opts.mi355x_devices_serial = "", False
        assert getattr(via_opts, "devices", None) == [0, 0] and all(np.array_equal(a, b) for a, b in zip(via_opts.images, whole.images))
        if serial:
            return
        # an accuracy-mode job: the replica follows the first model's setting
        shared.opts.sdmi_accuracy_mode = True
        try:
            whole = processing.process_images_one_device(mk(1, 2, width=64, height=64))       # (bit-identity holds at equal per-call batch size)
            pooled = pool.process_images(mk(1, 2, width=64, height=64))
        finally:
            shared.opts.sdmi_accuracy_mode = False
            model.set_accuracy_mode(False)
        assert all(np.array_equal(a, b) for a, b in zip(pooled.images, whole.images))
    finally:
        pool.close()
        par._POOLS.clear()
        shared.sd_model = model


def test_img2img_pil_front_end_fill_only_masked_and_overlay(dev, tiny):
    """The reference's PIL front-end of img2img / inpainting (modules/processing.py:1608-1745, 1063-1086) on the tiny model: mask
    from an RGBA layer, blur, "fill" masked content, whole-picture and "only masked" modes, overlay compositing.  Checked: the job run
    from PIL inputs equals the job run from the tensors the front-end derived (the tensor path is the one pinned against the oracle);
    the unmasked part of every output IS the original image; "only masked" returns the full-size picture; an all-black mask turns the
    job into plain img2img."""
    from PIL import Image
    processing, schema, sd_models = sub("processing"), sub("schema"), sub("sd_models")
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae(ch_mult=(1, 1, 2, 2))       # the PIL front-end works at width x height: needs the x8 VAE
    model = sd_models.SdModel(schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16), ucfg, vcfg, device=0)
    g = np.random.RandomState(12)
    W = H = 128
    base = Image.fromarray(g.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
    m = np.zeros((H, W), np.uint8)
    m[40:90, 30:100] = 255
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., 3] = m
    mask = Image.fromarray(rgba, "RGBA")
    cond, uncond = tiny["cond"][:2], tiny["uncond"][:2]

    def job(**kw):
        return processing.StableDiffusionProcessingImg2Img(sd_model=model, c=cond, uc=uncond, seed=77, batch_size=2, steps=4, cfg_scale=4.0,
                                                           width=W, height=H, sampler_name="Euler a", denoising_strength=0.6, **kw)
    # whole picture, masked content "fill", no blur: unmasked output pixels are the original's
    p = job(init_images=[base], mask_image=mask, inpainting_fill=0, inpaint_full_res=False, mask_blur=0)
    res = processing.process_images(p)
    assert len(res.images) == 2 and res.images[0].shape == (H, W, 3)
    keep = m == 0
    for im in res.images:
        assert np.array_equal(im[keep], np.array(base)[keep])
        assert not np.array_equal(im[~keep], np.array(base)[~keep])
    assert p.extra_generation_params.get("Masked content") == "fill"
    # the same job through the tensor API, from the tensors the front-end derived: identical latents
    p2 = job(init_images=p.init_images.clone(), latent_mask=p.latent_mask.clone(), image_mask=p.image_mask.clone(), inpainting_fill=1)
    res2 = processing.process_images(p2)
    assert torch.equal(res.latents, res2.latents)
    # masked content "original" starts from a different latent
    p3 = job(init_images=[base], mask_image=mask, inpainting_fill=1, inpaint_full_res=False, mask_blur=0)
    assert not torch.equal(processing.process_images(p3).latents, res.latents)
    # blurred mask: soft edge, the far field still untouched
    p4 = job(init_images=[base], mask_image=mask, inpainting_fill=1, inpaint_full_res=False, mask_blur=4)
    r4 = processing.process_images(p4)
    far = np.zeros((H, W), bool)
    far[:20] = True
    assert np.array_equal(r4.images[0][far], np.array(base)[far]) and p4.extra_generation_params["Mask blur"] == 4
    # "only masked" on a larger picture: the crop is processed at 128x128 and pasted back into the full-size image
    big = Image.fromarray(g.randint(0, 256, size=(192, 256, 3)).astype(np.uint8))
    mb = np.zeros((192, 256), np.uint8)
    mb[60:100, 100:180] = 255
    p5 = job(init_images=[big], mask_image=Image.fromarray(mb), inpainting_fill=1, inpaint_full_res=True, inpaint_full_res_padding=8, mask_blur=0)
    r5 = processing.process_images(p5)
    assert r5.images[0].shape == (192, 256, 3) and p5.paste_to is not None and p5.extra_generation_params["Inpaint area"] == "Only masked"
    assert np.array_equal(r5.images[0][mb == 0], np.array(big)[mb == 0])
    # inverted mask mode and a blank mask
    p6 = job(init_images=[base], mask_image=mask, inpainting_fill=1, inpaint_full_res=False, mask_blur=0, inpainting_mask_invert=1)
    r6 = processing.process_images(p6)
    assert np.array_equal(r6.images[0][~keep], np.array(base)[~keep]) and p6.extra_generation_params["Mask mode"] == "Inpaint not masked"
    p7 = job(init_images=[base], mask_image=Image.fromarray(np.zeros((H, W), np.uint8)), inpaint_full_res=True)
    r7 = processing.process_images(p7)
    assert p7.latent_mask is None and p7.overlay_images == [] or p7.latent_mask is None
    assert r7.images[0].shape == (H, W, 3)
    # resize_mode 3 ("latent upscale"): a 64x64 init image is encoded as it is and its 8x8 latent resized (bilinear) to the job's 16x16
    small = Image.fromarray(g.randint(0, 256, size=(64, 64, 3)).astype(np.uint8))
    p8 = job(init_images=[small], resize_mode=3)
    r8 = processing.process_images(p8)
    assert r8.images[0].shape == (H, W, 3) and tuple(p8.init_latent_all.shape) == (2, 4, H // 8, W // 8)
    lat = sub("ops").latent_resize(model.get_first_stage_encoding(model.encode_first_stage(
        (torch.from_numpy(np.moveaxis(np.array(small).astype(np.float32) / 255.0, 2, 0))[None].to(dev) * 2 - 1).contiguous())), (H // 8, W // 8), "bilinear")
    assert rel_l2(p8.init_latent_all[0].cpu(), lat[0].cpu()) < 2e-3      # batch 2 vs batch 1 encode: other tile configuration, fp16 rounding apart
    # one init image per image of the batch; fewer images than the batch size shrink the batch (:1718-1720)
    other = Image.fromarray(g.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
    p9 = job(init_images=[base, other])
    r9 = processing.process_images(p9)
    assert len(r9.images) == 2 and not np.array_equal(r9.images[0], r9.images[1]) and p9.extra_generation_params["Denoising strength"] == 0.6
    p10 = processing.StableDiffusionProcessingImg2Img(sd_model=model, c=tiny["cond"][:3], uc=tiny["uncond"][:3], seed=77, batch_size=3, steps=4, cfg_scale=4.0,
                                                      width=W, height=H, sampler_name="Euler a", denoising_strength=0.6, init_images=[base, other])
    r10 = processing.process_images(p10)
    assert p10.batch_size == 2 and len(r10.images) == 2
    assert all(np.array_equal(a, b) for a, b in zip(r10.images, r9.images))      # same seeds, same conds rows, same images
    # a VAE of another downscale factor cannot meet the (4, height // 8, width // 8) noise: a loud error, never an out-of-bounds read
    with pytest.raises(ValueError, match="does not match the noise shape"):
        processing.process_images(processing.StableDiffusionProcessingImg2Img(
            sd_model=tiny["model"], c=cond, uc=uncond, seed=77, batch_size=2, steps=4, cfg_scale=4.0, width=W, height=H, sampler_name="Euler a",
            denoising_strength=0.6, init_images=[base]))


# ------------------------------------------------------------------------------------------------------------
# a checkpoint whose biases put GroupNorm inputs far off zero
# ------------------------------------------------------------------------------------------------------------
OFFSET_BIAS = 20.0            # per-group bias offset; sized from the oracle alone (the precondition asserted below)
VAE_OFFSET_DECODE_MEASURED = 2.616e-03      # engine decode vs fp32 oracle decode on this checkpoint, MI355X (profiles/gn_offset_groups.md)


def _offset_heavy_state_dict(schema, ucfg, vcfg):
    """schema.synthetic_state_dict with one offset of +-OFFSET_BIAS per group of 1/32 of the channels added to the ResBlock conv and
    embedding biases, conv_in, and the VAE decoder's conv biases: what trained checkpoints have and 0.02 * randn biases do not."""
    import re
    sd = schema.synthetic_state_dict(ucfg, vcfg, dtype=torch.float16)
    hit = 0
    for i, key in enumerate(sorted(sd)):
        if not key.endswith(".bias") or sd[key].numel() % 32:
            continue
        unet = key.startswith("model.diffusion_model.") and (re.search(r"\.(in_layers\.2|out_layers\.3|emb_layers\.1)\.bias$", key)
                                                              or key.endswith("input_blocks.0.0.bias"))
        vae = key.startswith("first_stage_model.decoder.") and re.search(r"(conv1|conv2|conv_in|upsample\.conv|nin_shortcut)\.bias$", key)
        if unet or vae:
            sign = torch.where(seeded((32,), 1000 + i) >= 0, 1.0, -1.0)
            sd[key] = (sd[key].float() + (sign * OFFSET_BIAS).repeat_interleave(sd[key].numel() // 32)).half()
            hit += 1
    assert hit >= 30, hit
    return sd


def test_offset_heavy_checkpoint_unet_and_vae_vs_oracle(dev):
    """Model-level twin of tests/test_gpu_ops.py::test_groupnorm_offset_dominated_groups_vs_fp64: every synthetic checkpoint has biases of
    0.02 * randn, so no model test ever normalised a group whose mean is large against its spread.  Here the biases carry per-group
    offsets; hooks on the fp32 oracle assert the precondition (a GroupNorm input with |group mean| / std >= 100 in the UNet and in the
    VAE decoder), the engine's per-launch profile asserts that the two-launch form and the epilogue-statistics form both ran, and then
      * the UNet forward, default mode and `residual_fp32`, against the fp32 oracle: within 1.25 x the distance that the ENGINE'S ROUNDING
        PATTERN EMULATED ON THE ORACLE (tests/emu_engine_rounding.py: fp32 arithmetic, an fp16 rounding wherever the engine stores a
        tensor) has from the same oracle on the same weights and inputs — a reference-side prediction, computed here;
      * the VAE decode against the oracle decode: within 1.25 x the measured distance, VAE_OFFSET_DECODE_MEASURED (the rounding-pattern
        emulation covers the UNet only; the figure so far comes from the host-emulated kernels, whose fp32 arithmetic is the source's).
    A variance that cancels (sum x^2 / n - mean^2 in fp32) shows here as a distance the rounding pattern does not explain."""
    import ctypes
    import json
    from emu_engine_rounding import Emu
    from oracle import pipeline as opipe, unet as ou, vae as ov
    schema, lib = sub("schema"), sub("_lib")
    ucfg, vcfg = schema.tiny_unet(), schema.tiny_vae()
    sd = _offset_heavy_state_dict(schema, ucfg, vcfg)
    om = opipe.OracleModel(sd, ou.tiny_config(), ov.tiny_vae_config())
    ratios = {}

    def hook(name):
        def pre(m, inp):
            g = inp[0].reshape(inp[0].shape[0], m.num_groups, -1).double()
            ratios[name] = float((g.mean(-1).abs() / g.std(-1)).max())
        return pre
    handles = [m.register_forward_pre_hook(hook(p + n)) for p, net in (("unet.", om.unet), ("vae.", om.vae)) for n, m in net.named_modules()
               if isinstance(m, torch.nn.GroupNorm)]
    x, t, ctx = seeded((2, 4, 32, 32), 1), torch.tensor([999.0, 37.5]), seeded((2, 77, 64), 2).half().float()
    z = seeded((1, 4, 32, 32), 5) * 0.8
    with torch.no_grad():
        ref = om.unet(x.half().float(), t, ctx)
        ref32 = om.unet(x, t, ctx)                             # the accuracy mode hands conv_in the fp32 latent as a (hi, lo) pair
        vref = om.vae.decode_first_stage(z)
        for h_ in handles:
            h_.remove()
        e_emu = rel_l2(Emu(om.unet, stream_fp32=False)(x, t, ctx), ref)
        e_emu_acc = rel_l2(Emu(om.unet, stream_fp32=True, skip_fp32=True, h1_fp32=True, xin_fp32=True)(x, t, ctx), ref32)
    worst = {p: max(v for k, v in ratios.items() if k.startswith(p)) for p in ("unet.", "vae.")}
    assert worst["unet."] >= 100 and worst["vae."] >= 100, worst

    model = sub("sd_models").SdModel(sd, ucfg, vcfg, device=0)
    eng = model.engine

    def profiled(fn):
        lib.check(lib.lib.sdmi_profile_begin(), "profile_begin")
        out = fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 21)
        lib.check(lib.lib.sdmi_profile_end(buf, len(buf)), "profile_end")
        return out, [k["name"] for k in json.loads(buf.value.decode())["kernels"]]
    got, names = profiled(lambda: eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu())
    vgot, vnames = profiled(lambda: model.decode_first_stage(z.to(dev)).cpu())
    for path, nm in (("unet", names), ("vae", vnames)):
        assert any(n.startswith("groupnorm_silu B") for n in nm) and any(n.startswith("groupnorm_silu_apply B") for n in nm), (path, sorted(set(nm)))
    eng.set_option("residual_fp32", 1)
    try:
        acc = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
    finally:
        eng.set_option("residual_fp32", 0)
    e, e_acc, e_vae = rel_l2(got, ref), rel_l2(acc, ref32), rel_l2(vgot, vref)
    print(f"[offset checkpoint] worst |group mean| / std: unet {worst['unet.']:.0f}, vae {worst['vae.']:.0f}; unet default {e:.3e} (pattern emulated "
          f"{e_emu:.3e}), residual_fp32 {e_acc:.3e} (pattern emulated {e_emu_acc:.3e}); vae decode {e_vae:.3e}")
    assert torch.isfinite(got).all() and torch.isfinite(acc).all() and torch.isfinite(vgot).all()
    assert e <= 1.25 * e_emu, (e, e_emu)
    assert e_acc <= 1.25 * e_emu_acc, (e_acc, e_emu_acc)
    assert e_vae <= 1.25 * VAE_OFFSET_DECODE_MEASURED, e_vae


# ------------------------------------------------------------------------------------------------------------
# teacher-forced per-block parity (tests/teacher_forcing.py): the oracle's module N runs on the engine's own tap of block N - 1
# ------------------------------------------------------------------------------------------------------------
TF_T = [999.0, 37.5, 500.25]                    # the first two for B = 2; the ragged B = 3 case adds the third


def _traced(eng, fn):
    """fn() under engine option "trace" -> (its result, {tap name: NCHW fp32 on the CPU})."""
    eng.set_option("trace", 1)
    try:
        out = fn()
        torch.cuda.synchronize()
        taps = {k: v.float().cpu() for k, v in eng.taps().items()}
    finally:
        eng.set_option("trace", 0)
    return (tuple(o.float().cpu() for o in out) if isinstance(out, tuple) else out.float().cpu()), taps


def _tf_summary(net, rows, label):
    """One line per kind of segment: what profiles/teacher_forced_blocks.md records."""
    import teacher_forcing as tf
    kinds = {}
    for r in rows:
        kinds.setdefault(tf.segment_kind(net, r["block"]), []).append(r)
    for kind, rs in sorted(kinds.items()):
        ratio = [r["engine"] / r["yard"] for r in rs]
        worst = max(max(r[s][0] for s, _ in tf.SLICINGS) / r["yard"] for r in rs)
        print(f"[teacher_forced summary] {label} | {kind} | n {len(rs)} | engine {min(r['engine'] for r in rs):.2e}-{max(r['engine'] for r in rs):.2e} "
              f"| ratio {min(ratio):.2f}-{max(ratio):.2f} | worst slice {worst:.2f}")


def _teacher_forced_unet(dev, eng, net, x, t, ctx, y=None, label="unet"):
    """One traced engine forward, then every tap — and the output, as the tap of the module `out` — against the oracle module that
    produces it, run on the engine's previous tap: each segment within 1.25 x its own fp16 yardstick, per tensor and per slice."""
    import teacher_forcing as tf
    x, ctx = x.half().float(), ctx.half().float()
    y = None if y is None else y.half().float()
    got, taps = _traced(eng, lambda: eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev), None if y is None else y.to(dev)))
    assert torch.isfinite(got).all()
    taps["out"] = got
    assert set(taps) == set(tf.unet_tap_names(net)), sorted(set(taps) ^ set(tf.unet_tap_names(net)))
    rows = tf.segment_errors(net, lambda n: n(x, t, ctx, y), taps)
    _tf_summary(net, rows, label)
    tf.assert_segments(rows, label)
    return rows


TF_TINY_OPTIONS = {"default": {}, "ln_fold1": {"ln_fold": (1, 0)}, "ln_fold2": {"ln_fold": (2, 0)}, "force_generic": {"force_generic": (1, 0)},
                   "no_glds": {"glds": (0, 1)}, "tiling": {"tiling": (1, 0)}}          # option: (value, value to restore)


@pytest.mark.parametrize("case", list(TF_TINY_OPTIONS))
def test_teacher_forced_tiny_unet_options(dev, tiny, case):
    """The tiny UNet, 16x16 latent, B = 2, under each engine option that changes which launches a block is made of."""
    import copy
    eng, net = tiny["model"].engine, tiny["oracle"].unet
    opts = TF_TINY_OPTIONS[case]
    if case == "tiling":                                       # (as test_tiling_circular_padding_unet_and_vae_vs_oracle builds its oracle)
        net = copy.deepcopy(net)
        for layer in net.modules():
            if type(layer) == torch.nn.Conv2d:
                layer.padding_mode = "circular"
                layer._reversed_padding_repeated_twice = torch.nn.modules.utils._reverse_repeat_tuple(layer.padding, 2)
    for k, (v, _) in opts.items():
        eng.set_option(k, v)
    try:
        _teacher_forced_unet(dev, eng, net, seeded((2, 4, 16, 16), 301), torch.tensor(TF_T[:2]), seeded((2, 77, 64), 302), label="tiny/" + case)
    finally:
        for k, (_, v0) in opts.items():
            eng.set_option(k, v0)


def test_teacher_forced_tiny_unet_ragged(dev, tiny):
    """12x20 latent, B = 3: HW = 240 (60 at the second level) is no multiple of 64 — V^T gets zero-filled padding columns, the last
    query and key tiles are ragged, and 64-row GEMM tiles straddle images."""
    _teacher_forced_unet(dev, tiny["model"].engine, tiny["oracle"].unet, seeded((3, 4, 12, 20), 303), torch.tensor(TF_T), seeded((3, 77, 64), 304),
                         label="tiny/ragged")


def test_teacher_forced_unet_320_wide_with_and_without_the_row_chain(dev):
    """model_channels = 320, 8 heads: d = 40 / 80 heads, 10-channel groups, the 320-column tiles, and at level 0 (C = 320, HW = 256) the
    row-chain feed-forward — asserted from the per-launch profile: it ran with the default `fuse_rows` and did not with `fuse_rows` = 0.
    Then `ln_fold` = 1: the three LayerNorms of every block inside the GEMMs that read them."""
    import ctypes
    import json
    from oracle import unet as ou
    schema, lib = sub("schema"), sub("_lib")
    kw = dict(model_channels=320, num_heads=8, num_head_channels=-1, context_dim=768)
    cfg = schema.tiny_unet(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    net = ou.build_unet(ou.tiny_config(**kw), sd)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    x, t, ctx = seeded((2, 4, 16, 16), 305), torch.tensor(TF_T[:2]), seeded((2, 77, 768), 306)

    def profiled(label):
        lib.check(lib.lib.sdmi_profile_begin(), "profile_begin")
        try:
            _teacher_forced_unet(dev, eng, net, x, t, ctx, label=label)
        finally:
            buf = ctypes.create_string_buffer(1 << 21)
            lib.check(lib.lib.sdmi_profile_end(buf, len(buf)), "profile_end")
        return {k["name"]: k["launches"] for k in json.loads(buf.value.decode())["kernels"]}       # (one entry per launch name)
    try:
        names = profiled("wide320/fuse_rows_default")
        assert any(n.startswith("rowchain_ff") for n in names), sorted(set(names))
        eng.set_option("fuse_rows", 0)
        names = profiled("wide320/fuse_rows_0")
        assert names and not any(n.startswith("rowchain_ff") for n in names), sorted(set(names))
        eng.set_option("fuse_rows", 2)
        # `ln_fold` at these widths (d = 40 / 80 heads behind the folded q|k and V^T GEMMs).  Level 1 only: at the row counts a test can
        # afford, no GEMM tile that leaves LayerNorm row sums in its epilogue is chosen — measured here and on the tiny model, `ln_fold` = 2
        # makes the launches of `ln_fold` = 1, all 21 statistics launches included — so a second run would repeat the first.
        eng.set_option("ln_fold", 1)
        names = profiled("wide320/ln_fold1")
        assert any(" ln" in n for n in names), sorted(names)
        assert sum(k for n, k in names.items() if n.startswith("ln_rowstats")) == 3 * 7, names
    finally:
        eng.close()


def test_teacher_forced_sdxl_shaped_unet(dev):
    """The configuration of test_sdxl_shaped_unet_vs_oracle: Linear proj_in / proj_out, transformer depth 2 and 3 (block k + 1 reads
    block k's output), no attention at level 0, vector conditioning y -> label_emb."""
    from oracle import unet as ou
    schema = sub("schema")
    kw = dict(model_channels=64, channel_mult=(1, 2, 4), num_res_blocks=2, attention_resolutions=(2, 4), num_heads=-1,
              num_head_channels=64, transformer_depth=(1, 2, 3), context_dim=128, use_linear_in_transformer=True,
              adm_in_channels=192)
    cfg = schema.UNetConfig(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    net = ou.build_unet(ou.UNetConfig(**kw), sd)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    try:
        _teacher_forced_unet(dev, eng, net, seeded((2, 4, 16, 16), 307), torch.tensor(TF_T[:2]), seeded((2, 77, 128), 308), seeded((2, 192), 309),
                             label="sdxl_shaped")
    finally:
        eng.close()


def test_teacher_forced_tiny_unet_with_hypernetworks(dev, tiny):
    """The set-up of test_hypernetworks_in_engine_vs_oracle: with modules for the self-attention widths loaded, q and k are projected
    separately (`ldq = ldk = C`) from the normalised tokens and their transformed copy, and the cached cross-attention K / V^T come
    from the transformed text context."""
    from oracle import hypernetwork as ohn, unet as ou
    hn_mod = sub("hypernetwork")
    model, om = tiny["model"], tiny["oracle"]
    a = _hn_state([64, 128], [1, 2, 1], "relu", False, False, None, 7000, "hn_a")
    b = _hn_state([64], [1, 2, 2, 1], "swish", True, True, [0, 0.3, 0.3, 0], 7100, "hn_b")
    try:
        hn_mod.load_hypernetworks(model, [a, b], [0.8, 0.5])
        ou.LOADED_HYPERNETWORKS[:] = [ohn.Hypernetwork(a, 0.8), ohn.Hypernetwork(b, 0.5)]
        _teacher_forced_unet(dev, model.engine, om.unet, seeded((2, 4, 16, 16), 310), torch.tensor(TF_T[:2]), seeded((2, 77, 64), 311),
                             label="tiny/hypernetworks")
    finally:
        ou.LOADED_HYPERNETWORKS[:] = []
        hn_mod.load_hypernetworks(model, [], [])


@pytest.mark.parametrize("hw", [(16, 16), (12, 20)], ids=["16x16", "12x20"])
def test_teacher_forced_tiny_vae_decode(dev, tiny, hw):
    """The `decoder.*` taps of one decode (and the image, as the tap of `decoder.conv_out`) against the oracle VAE's modules of the same
    names; 12x20: HW = 240 in the attention block, 960 after the upsampling."""
    import teacher_forcing as tf
    model, vae = tiny["model"], tiny["oracle"].vae
    z = (seeded((2, 4) + hw, 312) * 0.8).half().float()
    got, taps = _traced(model.engine, lambda: model.decode_first_stage(z.to(dev)))
    assert torch.isfinite(got).all()
    taps["decoder.conv_out"] = got
    expected = set(tf.vae_tap_names(vae))
    assert set(taps) == expected, sorted(set(taps) ^ expected)
    label = "vae/%dx%d" % hw
    rows = tf.segment_errors(vae, lambda n: n.decode_first_stage(z), taps)
    _tf_summary(vae, rows, label)
    tf.assert_segments(rows, label)


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 24, 40), (1, 3, 26, 34)], ids=["32x32", "24x40", "26x34"])
def test_teacher_forced_tiny_vae_encode(dev, tiny, shape):
    """The `encoder.*` taps of one encode (and the fp32 moments, `quant_conv` folded into `conv_out` by the engine, as the tap of the
    AutoencoderKL's `quant_conv`) against the oracle VAE's modules of the same names.  24x40: HW = 960 at level 0 and 12 x 20 = 240 tokens
    in the mid attention; 26x34: the zero column and row that `Downsample` pads on the right and at the bottom only are read by the last
    output column and row of an odd half-size, 13 x 17.  (The image is rounded to fp16 first: that is what the engine's first launch
    reads.)"""
    import teacher_forcing as tf
    model, vae = tiny["model"], tiny["oracle"].vae
    x = torch.tanh(seeded(shape, 313)).half().float()
    got, taps = _traced(model.engine, lambda: model.encode_first_stage(x.to(dev)))
    assert torch.isfinite(got).all() and got.shape == (shape[0], 8, shape[2] // 2, shape[3] // 2)
    assert torch.equal(model.encode_first_stage(x.to(dev)).cpu(), got) and model.engine.taps() == {}     # without "trace": same bits, no taps left
    taps["quant_conv"] = got
    expected = tf.vae_encoder_tap_names(vae)
    assert set(taps) == set(expected) and len(expected) == 8, sorted(set(taps) ^ set(expected))
    label = "vae_enc/%dx%d" % shape[2:]
    rows = tf.segment_errors(vae, lambda n: n.encode_moments(x), taps)
    _tf_summary(vae, rows, label)
    tf.assert_segments(rows, label)


def _clip_engine_and_oracle(cfg):
    """-> (Engine with the tower loaded, the oracle ClipTextModel, the state dict): seeded synthetic fp16 weights."""
    import dataclasses
    from oracle import clip as oclip
    schema = sub("schema")
    sd = schema.synthetic_state_dict(clip_cfg=cfg, dtype=torch.float16)
    om = oclip.build_clip(oclip.ClipConfig(**dataclasses.asdict(cfg)), sd)
    eng = sub("engine").Engine(0)
    eng.load_clip(cfg, sd)
    return eng, om, sd


def _teacher_forced_clip(dev, eng, om, tok, skip, final_ln, label):
    """One traced engine forward without the pooled row, then every tap against the oracle's module or `+ x` point that produces it, run
    on the engine's previous tap; the returned fp32 state must be the last tap, converted, bit for bit."""
    import teacher_forcing as tf
    got, taps = _traced(eng, lambda: eng.clip_forward(tok.to(dev), skip=skip, apply_final_ln=final_ln))
    assert torch.isfinite(got).all()
    layers_run = len(om.encoder.layers) - skip + 1
    expected = tf.clip_tap_names(om, layers_run, final_ln)
    assert set(taps) == set(expected) and len(taps) == 1 + 2 * layers_run + int(final_ln), sorted(set(taps) ^ set(expected))
    last = taps["final_layer_norm" if final_ln else f"encoder.layers.{layers_run - 1}"]
    assert last.shape == (tok.shape[0], om.cfg.hidden, tok.shape[1], 1)
    assert torch.equal(got, last[:, :, :, 0].transpose(1, 2))
    # without "trace": the same bits, and the taps of the traced run are gone
    assert torch.equal(eng.clip_forward(tok.to(dev), skip=skip, apply_final_ln=final_ln).cpu(), got) and eng.taps() == {}
    rows = tf.segment_errors(om, lambda n: n(tok, skip=skip, apply_final_ln=final_ln), taps)
    _tf_summary(om, rows, label)
    tf.assert_segments(rows, label)
    return rows


TF_CLIP_TINY = [(b, act, skip, 0) for b in (1, 3) for act in ("quick_gelu", "gelu") for skip in (1, 2)] + [(3, "quick_gelu", 1, 1)]


@pytest.mark.parametrize("batch,act,skip,generic", TF_CLIP_TINY, ids=["B%d-%s-skip%d%s" % (c[0], c[1], c[2], "-generic" * c[3]) for c in TF_CLIP_TINY])
def test_teacher_forced_tiny_clip(dev, batch, act, skip, generic):
    """The tiny tower (3 layers, hidden 128, 2 heads of 64), L = 77: 77 and 231 rows are ragged against the 64- and 128-row GEMM tiles
    and the 128-query attention block, and the second 64-key tile holds 13 keys.  `skip` = 1 returns the final norm of the last layer,
    `skip` = 2 the penultimate layer without it (the SDXL CLIP-L form).  One case under `force_generic`: the generic attention kernel's
    causal path and the generic GEMM."""
    cfg = sub("schema").tiny_clip(act=act)
    eng, om, _ = _clip_engine_and_oracle(cfg)
    try:
        eng.set_option("force_generic", generic)
        _teacher_forced_clip(dev, eng, om, clip_tokens(batch, cfg.vocab_size, 320 + batch), skip, skip == 1,
                             "clip/tiny B%d %s skip%d%s" % (batch, act, skip, " generic" * generic))
    finally:
        eng.close()


def _pooled_row_checks(dev, eng, om, sd, tok, label):
    """`return_pooled` with `skip` = 2: the pooled row comes from a LayerNorm of the LAST layer that the returned state does not use
    (tap `pooled.final_layer_norm`).  That norm against the oracle's on the engine's last-layer tap; without a projection the pooled row
    is the norm's row at the first arg-max token, bit for bit; with `text_projection` every element is within the rounding of the
    kernel's own summation of the float64 product of that same row: 8 * ceil(K / 512) sequential FMAs per lane and a 6-level butterfly
    (the products of two fp16 values are exact in fp32), one unit of slack: (8 * ceil(K / 512) + 7) * 2^-24 * sum_k |w_k x_k|."""
    import math
    import teacher_forcing as tf
    from helpers import worst_slice_rel_l2
    from fp16_emu import r16
    layers, K = len(om.encoder.layers), om.cfg.hidden
    (out, pooled), taps = _traced(eng, lambda: eng.clip_forward(tok.to(dev), skip=2, apply_final_ln=False, return_pooled=True))
    expected = tf.clip_tap_names(om, layers, False) + ["pooled.final_layer_norm"]
    assert set(taps) == set(expected) and len(taps) == len(expected), sorted(set(taps) ^ set(expected))
    assert torch.equal(out, taps[f"encoder.layers.{layers - 2}"][:, :, :, 0].transpose(1, 2))
    norm = taps["pooled.final_layer_norm"]
    n32 = tf.as_nchw(om.final_layer_norm(taps[f"encoder.layers.{layers - 1}"][:, :, :, 0].transpose(1, 2)).detach(), tok.shape[1])
    row = {"block": "pooled.final_layer_norm", "shape": tuple(norm.shape), "engine": rel_l2(norm, n32), "yard": rel_l2(r16(n32), n32)}
    for name, keep in tf.SLICINGS:
        row[name] = worst_slice_rel_l2(norm, n32, keep)
    tf.assert_segments([row], label)
    pos = tok.to(torch.int).argmax(dim=-1)                        # the first of equal maxima
    rows = norm[torch.arange(tok.shape[0]), :, pos, 0]
    if om.text_projection is None:
        assert pooled.shape == rows.shape and torch.equal(pooled, rows)
        return
    w = sd[sub("schema").CLIP_PREFIX + "text_projection.weight"].double()
    ref = rows.double() @ w.T
    bound = (8 * math.ceil(K / 512) + 7) * 2.0 ** -24 * (rows.double().abs() @ w.abs().T)
    err = (pooled.double() - ref).abs()
    print(f"[pooled projection] {label}: K {K} N {w.shape[0]} worst |err| / bound {float((err / bound).max()):.3f}")
    assert pooled.shape == ref.shape and bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("batch", [3, 5])
@pytest.mark.parametrize("proj_dim", [None, 192, 320])
def test_clip_pooled_row_and_projection_against_the_engines_own_norm_tap(dev, proj_dim, batch):
    """The tiny tower's pooled row (clip_pool_kernel, small_linear).  `proj_dim` 192 (< 256 columns) runs small_linear's wave-per-column
    form, 320 the form that stages the rows in LDS: 4 rows at B = 3, 16 rows at B = 5."""
    cfg = sub("schema").tiny_clip(proj_dim=proj_dim)
    eng, om, sd = _clip_engine_and_oracle(cfg)
    try:
        _pooled_row_checks(dev, eng, om, sd, clip_tokens(batch, cfg.vocab_size, 330 + batch), "clip/tiny pooled B%d proj %s" % (batch, proj_dim))
    finally:
        eng.close()


@pytest.mark.parametrize("hidden,heads,act,proj_dim,batch", [(768, 12, "quick_gelu", None, 2), (1280, 20, "gelu", 1280, 3)], ids=["768", "1280"])
def test_teacher_forced_clip_at_real_widths(dev, hidden, heads, act, proj_dim, batch):
    """Two layers at CLIP-L's and OpenCLIP-bigG's widths (12 / 20 heads of 64, MLP 4 x hidden, vocabulary 1000): every segment is forced,
    so depth adds nothing.  `skip` = 1 with the final norm, then `skip` = 2 without; at 1280 also the pooled row through the 1280-column
    projection (K = 1280: three passes of 512 per lane)."""
    cfg = sub("schema").ClipConfig(vocab_size=1000, hidden=hidden, layers=2, heads=heads, intermediate=4 * hidden, act=act, proj_dim=proj_dim)
    eng, om, sd = _clip_engine_and_oracle(cfg)
    tok = clip_tokens(batch, cfg.vocab_size, 340 + batch)
    try:
        _teacher_forced_clip(dev, eng, om, tok, 1, True, "clip/%d B%d skip1" % (hidden, batch))
        _teacher_forced_clip(dev, eng, om, tok, 2, False, "clip/%d B%d skip2" % (hidden, batch))
        if proj_dim:
            _pooled_row_checks(dev, eng, om, sd, tok, "clip/%d pooled B%d" % (hidden, batch))
    finally:
        eng.close()


@pytest.mark.parametrize("batch", [2, 5, 16])
def test_small_linear_lds_forms_give_the_bits_of_the_wave_per_column_form_320_wide(dev, batch):
    """small_linear_lds_kernel (csrc/elementwise.hip) claims the bits of small_linear_kernel: same lane -> k assignment, FMA order and
    shuffle tree.  On the 320-wide UNet (time-embedding MLP: K = 320 and 1280; the fused ResBlock embedding projection: K = 1280, all
    blocks' columns at once) one forward with the knob off and one with it on — B = 2: the 4-row LDS form, 5 and 16: the 16-row form."""
    schema, lib = sub("schema"), sub("_lib")
    cfg = schema.tiny_unet(model_channels=320, num_heads=8, num_head_channels=-1, context_dim=768)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    x, t, ctx = seeded((batch, 4, 16, 16), 350), torch.linspace(999.0, 1.0, batch), seeded((batch, 77, 768), 351)
    outs = {}
    try:
        for mode in (0, 1):
            lib.check(lib.lib.sdmi_debug_set(b"small_linear_lds", mode))
            outs[mode] = eng.unet_forward(x.to(dev), t.to(dev), ctx.to(dev)).cpu()
    finally:
        lib.check(lib.lib.sdmi_debug_set(b"small_linear_lds", 1))
        eng.close()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
