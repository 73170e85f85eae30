"""CPU self-test of tests/teacher_forcing.py: the "engine" is the oracle itself under the reference's fp16 rounding pattern, so every
segment sits exactly on its yardstick; a planted one-pixel error and a renamed tap must each be caught and named."""
import importlib

import pytest
import torch

import teacher_forcing as tf
from helpers import clip_tokens, seeded

BLOCK, PIXEL = "middle_block.1", (1, 3, 5)        # a mid-network SpatialTransformer output [2, 128, 8, 8] and one (b, y, x) of it


@pytest.fixture(scope="module")
def forced():
    from oracle import unet as ou, vae as ov
    schema = importlib.import_module("stable-diffusion-webui_amd.schema")
    sd = schema.synthetic_state_dict(schema.tiny_unet(), schema.tiny_vae(), dtype=torch.float16)
    net = ou.build_unet(ou.tiny_config(), sd)
    vae = ov.build_vae(ov.tiny_vae_config(), sd)
    x, t, ctx = seeded((2, 4, 16, 16), 301).half().float(), torch.tensor([999.0, 37.5]), seeded((2, 77, 64), 302).half().float()
    z = (seeded((2, 4, 12, 20), 312) * 0.8).half().float()
    call, vcall = (lambda n: n(x, t, ctx)), (lambda n: n.decode_first_stage(z))
    plain = ou.BasicTransformerBlock.forward
    taps = tf.recorded_outputs(net, call, tf.unet_tap_names(net), fp16=True)
    vtaps = tf.recorded_outputs(vae, vcall, tf.vae_tap_names(vae), fp16=True)
    assert ou.BasicTransformerBlock.forward is plain         # both patches of the block forward are gone again
    return dict(net=net, call=call, taps=taps, vae=vae, vcall=vcall, vtaps=vtaps)


def test_segments_of_the_fp16_pattern_sit_on_their_own_yardstick(forced):
    """Forced with the fp16 pattern's own free-running tensors, the fp16 forced pass reproduces them — up to the fp32 summation order of a
    convolution or matrix product whose input now arrives in another memory layout, which moves a few results in a hundred to the
    neighbouring fp16 value: engine / yard = 1 within 1 % for every tap, the three `+ x` points of every transformer block included."""
    for net, call, taps, n_expected in ((forced["net"], forced["call"], forced["taps"], 40), (forced["vae"], forced["vcall"], forced["vtaps"], 10)):
        assert len(taps) == n_expected
        o16 = tf.forced_outputs(net, call, taps, fp16=True)
        assert all(float((o16[n] != taps[n]).float().mean()) < 0.15 for n in taps)
        rows = tf.assert_segments(tf.segment_errors(net, call, taps), "self", verbose=False)
        assert [r["block"] for r in rows] == list(taps)
        assert all(abs(r["engine"] / r["yard"] - 1) < 0.01 and r["yard"] >= 2e-4 for r in rows)
    # the free-running fp32 pass is NOT what the forced one computes: forcing really replaces (a hook that only recorded would pass the above)
    free32 = tf.recorded_outputs(forced["net"], forced["call"], list(forced["taps"]))
    o32 = tf.forced_outputs(forced["net"], forced["call"], forced["taps"])
    assert torch.equal(free32["input_blocks.0.0"], o32["input_blocks.0.0"]) and not torch.equal(free32["out"], o32["out"])


def test_one_scaled_pixel_is_named_with_its_block(forced):
    taps = dict(forced["taps"])
    t = taps[BLOCK].clone()
    b, y, x = PIXEL
    t[b, :, y, x] *= 1.01
    taps[BLOCK] = t
    with pytest.raises(AssertionError) as ei:
        tf.assert_segments(tf.segment_errors(forced["net"], forced["call"], taps), "planted", verbose=False)
    msg = str(ei.value)
    lines = [ln for ln in msg.splitlines() if ln.startswith("block ")]
    assert any(ln.startswith(f"block {BLOCK}: worst pixel (b, y, x) slice at {PIXEL}:") for ln in lines), msg
    # (1 % of one pixel in 128 is 8.8e-4 of the tensor: the whole-tensor cap sees it too, the pixel slicing sees it at full size and says
    # where.)  The only other segment that may complain is the one that READ the planted tensor: its tap came from the unplanted one
    order = list(taps)
    named = {ln.split(":")[0][len("block "):] for ln in lines}
    assert named <= {BLOCK, order[order.index(BLOCK) + 1]}, msg
    assert any(ln.startswith(f"block {BLOCK}: engine ") and "x yardstick" in ln for ln in lines), msg


def test_a_tap_without_an_oracle_counterpart_is_an_error(forced):
    taps = dict(forced["taps"])
    taps["middle_block.1.transformer_blocks.0.attn3+x"] = taps.pop("middle_block.1.transformer_blocks.0.attn2+x")
    with pytest.raises(tf.UnmatchedTap, match=r"1 of 40 taps match no oracle module or sub-tap point: \['middle_block.1.transformer_blocks.0.attn3\+x'\]"):
        tf.segment_errors(forced["net"], forced["call"], taps)
    vtaps = dict(forced["vtaps"])
    vtaps["decoder.up.1.block.9"] = vtaps.pop("decoder.up.1.block.1")
    with pytest.raises(tf.UnmatchedTap, match="decoder.up.1.block.9"):
        tf.segment_errors(forced["vae"], forced["vcall"], vtaps)


# ------------------------------------------------------------------------------------------------------------
# the CLIP text tower and the VAE encoder
# ------------------------------------------------------------------------------------------------------------
CLIP_TAP, CLIP_TOKEN = "encoder.layers.1.self_attn+x", (2, 40)       # the first `+ x` of the middle layer [3, 128, 77, 1] and one (b, l) of it


@pytest.fixture(scope="module")
def forced_text_and_encoder():
    import dataclasses
    from oracle import clip as oclip, vae as ov
    schema = importlib.import_module("stable-diffusion-webui_amd.schema")
    out = {}
    for act in ("quick_gelu", "gelu"):
        cfg = schema.tiny_clip(act=act)
        om = oclip.build_clip(oclip.ClipConfig(**dataclasses.asdict(cfg)), schema.synthetic_state_dict(clip_cfg=cfg, dtype=torch.float16))
        tok = clip_tokens(3, cfg.vocab_size, 323)
        for skip, final_ln in ((1, True), (2, False)):
            call = lambda n, tok=tok, skip=skip, final_ln=final_ln: n(tok, skip=skip, apply_final_ln=final_ln)
            names = tf.clip_tap_names(om, cfg.layers - skip + 1, final_ln)
            out["clip", act, skip] = (om, call, tf.recorded_outputs(om, call, names, fp16=True), names)
    plain = oclip.ClipLayer.forward
    vae = ov.build_vae(ov.tiny_vae_config(), schema.synthetic_state_dict(None, schema.tiny_vae(), dtype=torch.float16))
    for shape in ((2, 3, 24, 40), (1, 3, 26, 34)):
        x = torch.tanh(seeded(shape, 313)).half().float()
        call = lambda n, x=x: n.encode_moments(x)
        names = tf.vae_encoder_tap_names(vae)
        out["enc", shape] = (vae, call, tf.recorded_outputs(vae, call, names, fp16=True), names)
    assert oclip.ClipLayer.forward is plain
    return out


def test_clip_and_encoder_segments_sit_on_their_own_yardstick(forced_text_and_encoder):
    """The oracle under the fp16 pattern as its own engine, on the tiny CLIP tower (both activations; with the final norm, and the
    penultimate layer without it) and the tiny VAE encoder: every new segment within 1 % of its yardstick — and every yardstick, which
    comes from the oracle alone, at or above YARD_FLOOR, so that no cap of the GPU tests is vacuous."""
    for key, (net, call, taps, names) in forced_text_and_encoder.items():
        assert list(taps) == names and len(names) == (8 if key[0] == "enc" else 8 if key[2] == 1 else 5), key
        rows = tf.assert_segments(tf.segment_errors(net, call, taps), "self", verbose=False)
        assert [r["block"] for r in rows] == names
        assert all(abs(r["engine"] / r["yard"] - 1) < 0.01 and r["yard"] >= tf.YARD_FLOOR for r in rows), (key, rows)
    # a token tensor is filed with one row of the NCHW tensor per token, and forcing really replaces
    net, call, taps, _ = forced_text_and_encoder["clip", "gelu", 1]
    assert taps["embeddings"].shape == (3, 128, 77, 1)
    free32, o32 = tf.recorded_outputs(net, call, list(taps)), tf.forced_outputs(net, call, taps)
    assert torch.equal(free32["embeddings"], o32["embeddings"]) and not torch.equal(free32["final_layer_norm"], o32["final_layer_norm"])


def test_one_scaled_token_is_named_with_its_layer(forced_text_and_encoder):
    net, call, taps, _ = forced_text_and_encoder["clip", "quick_gelu", 1]
    taps = dict(taps)
    t = taps[CLIP_TAP].clone()
    b, l = CLIP_TOKEN
    t[b, :, l, 0] *= 1.01
    taps[CLIP_TAP] = t
    with pytest.raises(AssertionError) as ei:
        tf.assert_segments(tf.segment_errors(net, call, taps), "planted", verbose=False)
    msg = str(ei.value)
    lines = [ln for ln in msg.splitlines() if ln.startswith("block ")]
    assert any(ln.startswith(f"block {CLIP_TAP}: worst pixel (b, y, x) slice at {(b, l, 0)}:") for ln in lines), msg
    order = list(taps)
    named = {ln.split(":")[0][len("block "):] for ln in lines}
    assert named <= {CLIP_TAP, order[order.index(CLIP_TAP) + 1]}, msg


def test_a_renamed_clip_or_encoder_tap_is_an_error(forced_text_and_encoder):
    net, call, taps, _ = forced_text_and_encoder["clip", "quick_gelu", 1]
    taps = dict(taps)
    taps["encoder.layers.1.mlp+x"] = taps.pop("encoder.layers.1.self_attn+x")
    with pytest.raises(tf.UnmatchedTap, match=r"1 of 8 taps match no oracle module or sub-tap point: \['encoder.layers.1.mlp\+x'\]"):
        tf.segment_errors(net, call, taps)
    # a layer the pass never records a tap for: `pooled.final_layer_norm` is no module of the tower
    taps = dict(forced_text_and_encoder["clip", "quick_gelu", 1][2])
    taps["pooled.final_layer_norm"] = taps.pop("final_layer_norm")
    with pytest.raises(tf.UnmatchedTap, match="pooled.final_layer_norm"):
        tf.segment_errors(net, call, taps)
    vae, vcall, vtaps, _ = forced_text_and_encoder["enc", (1, 3, 26, 34)]
    vtaps = dict(vtaps)
    vtaps["encoder.down.1.downsample"] = vtaps.pop("encoder.down.0.downsample")       # the last level has no Downsample
    with pytest.raises(tf.UnmatchedTap, match="encoder.down.1.downsample"):
        tf.segment_errors(vae, vcall, vtaps)
