"""The cross-attention chain inside the UNet (engine option `fuse_rows` bit 0, csrc/engine.cpp run_st): the 320-wide tiny UNet of
tests/test_gpu_models.py::test_teacher_forced_unet_320_wide_with_and_without_the_row_chain (16x16 latent, B = 2: 256 token rows per image at
level 0) teacher-forced block by block with the chain on and off, and — from the per-launch profile — which launches each setting makes."""
import ctypes
import importlib
import json
import types

import pytest
import torch

import teacher_forcing as tf
from helpers import seeded

pytestmark = pytest.mark.gpu

TF_T = [999.0, 37.5]


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def wide():
    from oracle import unet as ou
    sub("_lib").require_device()
    schema = sub("schema")
    kw = dict(model_channels=320, num_heads=8, num_head_channels=-1, context_dim=768)
    cfg = schema.tiny_unet(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    yield dict(eng=eng, net=ou.build_unet(ou.tiny_config(**kw), sd), dev=torch.device("cuda", 0),
               x=seeded((2, 4, 16, 16), 305).half().float(), t=torch.tensor(TF_T), ctx=seeded((2, 77, 768), 306).half().float())
    eng.close()


def profiled(fn):
    """fn() under the per-launch profiler -> {launch name: launches}."""
    lib = sub("_lib")
    lib.check(lib.lib.sdmi_profile_begin(), "profile_begin")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        buf = ctypes.create_string_buffer(1 << 21)
        lib.check(lib.lib.sdmi_profile_end(buf, len(buf)), "profile_end")
    return {k["name"]: k["launches"] for k in json.loads(buf.value.decode())["kernels"]}


def count(names, prefix):
    return sum(n for k, n in names.items() if k.startswith(prefix))


def teacher_forced(w, label):
    """One traced engine forward; every tap against the oracle module that produces it, run on the engine's previous tap, under
    tests/teacher_forcing.py's own rule."""
    eng, net, dev = w["eng"], w["net"], w["dev"]
    eng.set_option("trace", 1)
    try:
        got = eng.unet_forward(w["x"].to(dev), w["t"].to(dev), w["ctx"].to(dev), None).float().cpu()
        torch.cuda.synchronize()
        taps = {k: v.float().cpu() for k, v in eng.taps().items()}
    finally:
        eng.set_option("trace", 0)
    assert torch.isfinite(got).all()
    taps["out"] = got
    assert set(taps) == set(tf.unet_tap_names(net)), sorted(set(taps) ^ set(tf.unet_tap_names(net)))
    rows = tf.segment_errors(net, lambda n: n(w["x"], w["t"], w["ctx"], None), taps)
    tf.assert_segments(rows, label)


def test_teacher_forced_with_and_without_the_cross_attention_chain(wide):
    """`fuse_rows` 3 and 2: every segment — the `attn2+x` tap among them, which the chain still feeds — passes the teacher-forcing rule.
    With 3 the profile shows one rowchain_xattn launch per 320-wide block, and neither that block's norm2 LayerNorm nor its
    cross-attention launch (the 640-wide level keeps both); with 2 none of the new launches."""
    eng = wide["eng"]
    try:
        eng.set_option("fuse_rows", 2)
        off = profiled(lambda: teacher_forced(wide, "wide320/fuse_rows_2"))
        eng.set_option("fuse_rows", 3)
        on = profiled(lambda: teacher_forced(wide, "wide320/fuse_rows_3"))
    finally:
        eng.set_option("fuse_rows", 3)
    ln320 = "layernorm rows512 C320"
    assert count(off, "rowchain_xattn") == 0, sorted(off)
    blocks = count(on, "rowchain_xattn")
    assert blocks >= 1, sorted(on)
    assert count(off, ln320) == 2 * blocks and count(on, ln320) == blocks, (off, on)          # norm1 + norm2 (norm3 is in the ff chain) | norm1
    assert count(on, "attention_mfma_cross") == count(off, "attention_mfma_cross") - blocks, (off, on)
    assert count(on, "rowchain_ff") == count(off, "rowchain_ff") == blocks, (off, on)


def test_chain_stays_off_with_a_hypernetwork_of_its_width_or_residual_fp32(wide):
    """A hypernetwork loaded for width 320 transforms the normalised tokens of the 320-wide blocks, and `residual_fp32` carries the token
    stream as (hi, lo) pairs: in both cases the four launches run, not the chain."""
    from oracle import hypernetwork as ohn
    from helpers import seeded_module_weights
    hn_mod = sub("hypernetwork")
    eng, dev = wide["eng"], wide["dev"]
    model = types.SimpleNamespace(engine=eng)

    def forward():
        out = eng.unet_forward(wide["x"].to(dev), wide["t"].to(dev), wide["ctx"].to(dev), None)
        assert torch.isfinite(out.float()).all()
    eng.set_option("fuse_rows", 3)
    assert count(profiled(forward), "rowchain_xattn") >= 1
    try:
        # a hypernetwork file's content (what torch.load returns) for width 320, structure [1, 2, 1], seeded weights near the identity map
        state = {"layer_structure": [1, 2, 1], "activation_func": "relu", "is_layer_norm": False, "activate_output": False,
                 "dropout_structure": None, "name": "hn_320"}
        pair = []
        for w in (0, 1):
            m = ohn.HypernetworkModule(320, None, [1, 2, 1], "relu", False, False, None)
            seeded_module_weights(m, 7400 + w)
            with torch.no_grad():
                for prm in m.parameters():
                    if prm.dim() == 2:
                        prm.mul_(0.5)
            pair.append({k: v.clone() for k, v in m.state_dict().items()})
        state[320] = tuple(pair)
        hn_mod.load_hypernetworks(model, [state], [0.5])
        names = profiled(forward)
        assert count(names, "rowchain_xattn") == 0 and count(names, "attention_mfma_cross") >= 2, sorted(names)
    finally:
        hn_mod.load_hypernetworks(model, [], [])
    try:
        eng.set_option("residual_fp32", 1)
        names = profiled(forward)
        assert count(names, "rowchain_xattn") == 0 and count(names, "attention_mfma_cross") >= 2, sorted(names)
    finally:
        eng.set_option("residual_fp32", 0)
    assert count(profiled(forward), "rowchain_xattn") >= 1
