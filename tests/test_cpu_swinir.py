"""CPU tier of the SwinIR path: the host-only parts (checkpoint loader and dispatcher, webui hook, the reference restatement itself,
pinned to an independent implementation and to answers worked out by hand), the fitness of the GPU tests' inputs for their comparison
rule, the compiled kernels' metadata, and one run of tests/test_gpu_swinir.py on the host-emulated library."""
import importlib
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import compact_reference as CR
import rrdb_reference as RR
import swinir_reference as R
from helpers import rel_l2, worst_slice_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE_CASES = 8 + 1 + 1 + 6 + 1 + 2 + 1 + 5 + 1 + 1 + 1 + 1 + 1          # the cases of tests/test_gpu_swinir.py


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_swinir_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_swinir.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= GPU_FILE_CASES, out[-2000:]


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def zeros_state_dict(c=60, depths=(2,), heads=2, hidden=None, resi3=False, scale=4, table_rows=225, in_ch=3, upsampler="nearest+conv"):
    """The key layout of a SwinIR checkpoint, all zeros, with the two buffers the loader ignores."""
    hidden = hidden or 2 * c
    z = torch.zeros
    sd = {"conv_first.weight": z(c, in_ch, 3, 3), "conv_first.bias": z(c), "patch_embed.norm.weight": z(c), "patch_embed.norm.bias": z(c)}

    def resi(stem):
        if not resi3:
            sd[stem + ".weight"], sd[stem + ".bias"] = z(c, c, 3, 3), z(c)
        else:
            for k, shape in ((0, (c // 4, c, 3, 3)), (2, (c // 4, c // 4, 1, 1)), (4, (c, c // 4, 3, 3))):
                sd[f"{stem}.{k}.weight"], sd[f"{stem}.{k}.bias"] = z(*shape), z(shape[0])
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            for n in ("norm1", "norm2"):
                sd[b + n + ".weight"], sd[b + n + ".bias"] = z(c), z(c)
            sd[b + "attn.relative_position_bias_table"] = z(table_rows, heads)
            sd[b + "attn.relative_position_index"] = z(64, 64, dtype=torch.long)
            if j % 2:
                sd[b + "attn_mask"] = z(64, 64, 64)
            for n, (o, k) in (("attn.qkv", (3 * c, c)), ("attn.proj", (c, c)), ("mlp.fc1", (hidden, c)), ("mlp.fc2", (c, hidden))):
                sd[b + n + ".weight"], sd[b + n + ".bias"] = z(o, k), z(o)
        resi(f"layers.{i}.conv")
    sd["norm.weight"], sd["norm.bias"] = z(c), z(c)
    resi("conv_after_body")
    if upsampler == "nearest+conv":
        names = ["conv_before_upsample.0", "conv_up1"] + (["conv_up2"] if scale == 4 else []) + ["conv_hr"]
        for n in names:
            sd[n + ".weight"], sd[n + ".bias"] = z(64, c if n.startswith("conv_before") else 64, 3, 3), z(64)
    elif upsampler == "pixelshuffle":
        sd["conv_before_upsample.0.weight"], sd["conv_before_upsample.0.bias"] = z(64, c, 3, 3), z(64)
        sd["upsample.0.weight"], sd["upsample.0.bias"] = z(256, 64, 3, 3), z(256)
    sd["conv_last.weight"], sd["conv_last.bias"] = z(3, 64, 3, 3), z(3)
    return sd


def blob_of(sd, cfg):
    """The documented order (include/sdmi.h at sdmi_swinir_config), written out independently of the loader."""
    def wb(n):
        return [sd[n + ".weight"].flatten(), sd[n + ".bias"].flatten()]

    def resi(stem):
        return sum((wb(f"{stem}.{k}") for k in (0, 2, 4)), []) if cfg["resi_3conv"] else wb(stem)
    parts = wb("conv_first") + wb("patch_embed.norm")
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            parts += wb(b + "norm1") + [sd[b + "attn.relative_position_bias_table"].flatten()] + wb(b + "attn.qkv") + wb(b + "attn.proj")
            parts += wb(b + "norm2") + wb(b + "mlp.fc1") + wb(b + "mlp.fc2")
        parts += resi(f"layers.{i}.conv")
    parts += wb("norm") + resi("conv_after_body") + wb("conv_before_upsample.0") + wb("conv_up1")
    parts += (wb("conv_up2") if cfg["scale"] == 4 else []) + wb("conv_hr") + wb("conv_last")
    return torch.cat(parts).float().numpy()


def test_loader_reads_the_config_of_the_shipped_shapes():
    parse = sub("upscaler").parse_swinir_state_dict
    blob, cfg = parse(zeros_state_dict(240, (6,) * 9, 8, 480, True, 4))                      # SwinIR-L x4 GAN
    assert cfg == dict(embed_dim=240, depths=(6,) * 9, num_heads=8, mlp_hidden=480, resi_3conv=1, scale=4)
    assert blob.dtype == np.float32 and blob.ndim == 1
    for scale in (4, 2):                                                                     # the M models
        blob, cfg = parse(zeros_state_dict(180, (6,) * 6, 6, 360, False, scale))
        assert cfg == dict(embed_dim=180, depths=(6,) * 6, num_heads=6, mlp_hidden=360, resi_3conv=0, scale=scale)


@pytest.mark.parametrize("args", [(60, (2, 2), 2, "3conv", 4), (60, (2,), 2, "1conv", 2), (240, (2,), 8, "3conv", 4), (180, (2,), 6, "1conv", 4),
                                  (60, (1, 3, 2), 2, "1conv", 4)])
def test_loader_blob_is_the_documented_concatenation(args):
    parse = sub("upscaler").parse_swinir_state_dict
    sd = R.make_state_dict(*args)
    blob, cfg = parse(sd)
    assert cfg == R.config_of(sd) and cfg["depths"] == tuple(args[1]) and cfg["resi_3conv"] == int(args[3] == "3conv")
    assert np.array_equal(blob, blob_of(sd, cfg))
    n = sum(v.numel() for k, v in sd.items() if not k.endswith(("relative_position_index", "attn_mask")))
    assert blob.size == n                                                                    # the two buffers are ignored, nothing else is


@pytest.mark.parametrize("wrapper", ["params_ema", "params"])
def test_loader_unwraps_the_training_wrappers(wrapper):
    parse = sub("upscaler").parse_swinir_state_dict
    sd = R.make_state_dict(60, (2,), 2, "1conv", 2)
    blob = parse(sd)[0]
    assert np.array_equal(parse({wrapper: sd})[0], blob)
    assert np.array_equal(parse({"params": zeros_state_dict(60, (2,), 2, scale=2), "params_ema": sd})[0], blob)      # the EMA weights win


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_swinir_state_dict
    with pytest.raises(ValueError, match="upsampler 'pixelshuffle'.*nearest\\+conv"):
        parse(zeros_state_dict(upsampler="pixelshuffle"))
    with pytest.raises(ValueError, match="upsampler 'none'"):
        parse(zeros_state_dict(upsampler="none"))
    with pytest.raises(ValueError, match="window_size 7 \\(a 169-row bias table\\)"):
        parse(zeros_state_dict(table_rows=169))
    with pytest.raises(ValueError, match="head_dim = 240/6 = 40"):
        parse(zeros_state_dict(240, (2,), 6))
    with pytest.raises(ValueError, match="takes 1 input channels"):
        parse(zeros_state_dict(in_ch=1))
    sd = zeros_state_dict()
    del sd["layers.0.residual_group.blocks.1.mlp.fc2.bias"]
    with pytest.raises(ValueError, match=r"lacks layers\.0\.residual_group\.blocks\.1\.mlp\.fc2\.bias"):
        parse(sd)
    sd = zeros_state_dict()
    sd["absolute_pos_embed"] = torch.zeros(1, 4096, 60)
    with pytest.raises(ValueError, match="ape"):
        parse(sd)
    with pytest.raises(ValueError, match="not a SwinIR checkpoint"):
        parse(RR.make_state_dict(1, 4))


# ---- the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_sends_the_three_key_layouts_to_their_loaders():
    up = sub("upscaler")
    swin = R.make_state_dict(60, (2,), 2, "1conv", 2)
    for sd in (swin, {"params_ema": swin}, {"params": swin}):
        assert up.upscaler_family(sd) == "swinir"
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "swinir" and parsed[-1] == 2 and parsed[1] == R.config_of(swin)
        assert np.array_equal(parsed[0], up.parse_swinir_state_dict(swin)[0])
    # what tests/test_cpu_compact.py and tests/test_cpu_esrgan.py assert of the dispatcher keeps its answer
    rrdb = RR.make_state_dict(2, 4)
    for sd in (rrdb, RR.to_old_arch(rrdb, 2), {"params_ema": rrdb}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "rrdb" and parsed[1:] == (2, 3, 4)
    compact = CR.make_state_dict(4, 2)
    for sd in (compact, {"params": compact}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "compact" and parsed[1:] == (4, 2)
    with pytest.raises(ValueError, match="not an RRDBNet checkpoint: neither conv_first.weight nor model.0.weight"):
        up.parse_upscaler_state_dict({"layers.0.weight": torch.zeros(4, 4)})
    with pytest.raises(ValueError, match="head_dim"):                                         # a SwinIR the engine refuses: that loader's message
        up.parse_upscaler_state_dict(zeros_state_dict(240, (2,), 6))


def test_make_upscaler_net_picks_the_class_by_the_keys(monkeypatch):
    up = sub("upscaler")
    made = []
    for cls, tag in ((up.EsrganNet, "rrdb"), (up.CompactNet, "compact"), (up.SwinIRNet, "swinir")):
        monkeypatch.setattr(cls, "__init__", lambda self, sd, device=0, engine=None, _t=tag: made.append(_t))
    assert isinstance(up.make_upscaler_net(RR.make_state_dict(1, 4)), up.EsrganNet)
    assert isinstance(up.make_upscaler_net({"params": CR.make_state_dict(2, 4)}), up.CompactNet)
    assert isinstance(up.make_upscaler_net({"params_ema": zeros_state_dict()}), up.SwinIRNet)
    assert made == ["rrdb", "compact", "swinir"]


def test_register_esrgan_takes_a_swinir_checkpoint(tmp_path, monkeypatch):
    up, shared = sub("upscaler"), sub("shared")
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save({"params_ema": zeros_state_dict(180, (2,), 6, scale=2)}, str(tmp_path / "swinir_m_x2.pth"))
    torch.save(RR.make_state_dict(1, 4), str(tmp_path / "rrdb_x4.pth"))
    added = up.register_esrgan([str(tmp_path / "swinir_m_x2.pth"), str(tmp_path / "rrdb_x4.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "swinir_m_x2", "rrdb_x4"]
    assert [d.scale for d in added] == [2, 4]


def test_too_large_or_too_small_an_input_is_refused(monkeypatch):
    up = sub("upscaler")
    net = up.SwinIRNet.__new__(up.SwinIRNet)
    net.scale, net.device, net.handle = 4, 0, None
    net.engine = types.SimpleNamespace(arena_bytes=lambda: 1000)
    monkeypatch.setattr(up.SwinIRNet, "scratch_bytes", lambda self, b, h, w: 5000)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 4000)
    net.check_fits(1, 512, 512)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 3999)
    with pytest.raises(up.EsrganInputTooLarge, match=r"512x512 \(batch 1\) is too large for the x4 upscaler"):
        net.check_fits(1, 512, 512)
    monkeypatch.setattr(up.SwinIRNet, "scratch_bytes", lambda self, b, h, w: 0)           # the engine's own refusal: a tensor of 2^31 elements
    with pytest.raises(up.EsrganInputTooLarge, match="2\\^31"):
        net.check_fits(1, 4096, 4096)
    with pytest.raises(ValueError, match="at least 8"):
        net.check_fits(1, 7, 64)


# ---- the webui hook ---------------------------------------------------------------------------------------------------------------
def test_install_swinir_hook_on_stub_scalers(tmp_path, monkeypatch):
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, jpeg = str(tmp_path / "SwinIR_4x.pth"), str(tmp_path / "jpeg_car.pth")
    torch.save({"params_ema": zeros_state_dict(180, (2,), 6)}, good)
    torch.save({"params": zeros_state_dict(180, (2,), 6, table_rows=169)}, jpeg)

    class UpscalerSwinIR:                                      # the shape of the extension's scaler object
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, model_file):
            self.stock_calls.append(model_file)
            return img

    class UpscalerESRGAN(UpscalerSwinIR):
        pass
    scaler, other = UpscalerSwinIR(), UpscalerESRGAN()
    url = "https://example.invalid/003_realSR_BSRGAN_DFOWMFC_s64w8_SwinIR-L_x4_GAN.pth"
    data = [types.SimpleNamespace(name="SwinIR 4x", data_path=good, local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="SwinIR jpeg", data_path=jpeg, local_data_path=jpeg, scaler=scaler),
            types.SimpleNamespace(name="SwinIR L", data_path=url, local_data_path=None, scaler=scaler),
            types.SimpleNamespace(name="ESRGAN_4x", data_path=good, local_data_path=good, scaler=other)]
    scaler.scalers = data[:3]
    engine_calls = []
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", lambda self, path: up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(path)))
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    shared = types.SimpleNamespace(sd_upscalers=data)
    assert bridge.install_swinir_hook(shared) == ["SwinIR 4x", "SwinIR jpeg", "SwinIR L"]          # the ESRGAN scaler is not this hook's
    assert bridge.install_swinir_hook(shared) == ["SwinIR 4x", "SwinIR jpeg", "SwinIR L"]          # idempotent
    assert not hasattr(other.do_upscale, "_mi355x_stock")
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, good)
    assert engine_calls == [good] and scaler.stock_calls == []
    scaler.do_upscale(img, jpeg)                               # window 7: the loader refuses, the stock path runs it
    assert engine_calls == [good] and scaler.stock_calls == [jpeg]
    scaler.do_upscale(img, url)                                # not on disk yet: the stock code downloads and runs it
    assert engine_calls == [good] and scaler.stock_calls == [jpeg, url]

    def too_large(self, img, path=None):
        raise up.EsrganInputTooLarge("too large")
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", too_large)
    scaler.do_upscale(img, good)
    assert scaler.stock_calls == [jpeg, url, good]


# ---- the reference, pinned --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_reference_block_equals_the_transformers_swin_layer(shift):
    """One SwinTransformerBlock of swinir_reference (C 60, 2 heads, mlp_ratio 2, 16 x 24) against transformers' SwinLayer with the same
    weights: an implementation written by other people from the same paper."""
    swin = pytest.importorskip("transformers.models.swin.modeling_swin")
    from transformers import SwinConfig
    sd = R.make_state_dict(60, (2,), 2, "1conv", 2, seed=3)
    pre = "layers.0.residual_group.blocks.1."
    layer = swin.SwinLayer(SwinConfig(window_size=8, mlp_ratio=2.0, hidden_act="gelu", layer_norm_eps=1e-5), 60, (16, 24), 2, 0.0, shift).eval()
    qkv_w, qkv_b = sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]
    mine = {"attention.relative_position_bias.relative_position_bias_table": sd[pre + "attn.relative_position_bias_table"],
            "attention.o_proj.weight": sd[pre + "attn.proj.weight"], "attention.o_proj.bias": sd[pre + "attn.proj.bias"],
            "layernorm_before.weight": sd[pre + "norm1.weight"], "layernorm_before.bias": sd[pre + "norm1.bias"],
            "layernorm_after.weight": sd[pre + "norm2.weight"], "layernorm_after.bias": sd[pre + "norm2.bias"],
            "mlp.fc1.weight": sd[pre + "mlp.fc1.weight"], "mlp.fc1.bias": sd[pre + "mlp.fc1.bias"],
            "mlp.fc2.weight": sd[pre + "mlp.fc2.weight"], "mlp.fc2.bias": sd[pre + "mlp.fc2.bias"]}
    for i, n in enumerate("qkv"):
        mine[f"attention.{n}_proj.weight"], mine[f"attention.{n}_proj.bias"] = qkv_w[60 * i:60 * (i + 1)], qkv_b[60 * i:60 * (i + 1)]
    missing, unexpected = layer.load_state_dict(mine, strict=False)
    assert not unexpected and all("relative_position_index" in k for k in missing), (missing, unexpected)
    x = torch.randn((2, 16, 24, 60), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        theirs = layer(x.reshape(2, 16 * 24, 60), (16, 24))
    theirs = theirs[0] if isinstance(theirs, (tuple, list)) else theirs
    ours = R.block(sd, pre, x, 2, shift).reshape(2, 16 * 24, 60)
    assert torch.allclose(ours, theirs, rtol=1e-5, atol=1e-5), float((ours - theirs).abs().max())


def test_relative_position_index_at_three_pairs_by_hand():
    """index[a][b] = (ya - yb + 7) * 15 + (xa - xb + 7), tokens row-major in the window."""
    idx = R.relative_position_index()
    assert idx.shape == (64, 64)
    assert int(idx[0, 0]) == 7 * 15 + 7 == 112                           # a token and itself: the table's centre
    assert int(idx[0, 63]) == 0 and int(idx[63, 0]) == 224               # (0,0) vs (7,7): (-7, -7) -> 0; the other way (7, 7) -> 14 * 15 + 14
    assert int(idx[10, 3]) == (1 - 0 + 7) * 15 + (2 - 3 + 7) == 126      # (1,2) vs (0,3)


def test_region_ids_and_mask_of_a_shifted_16x16_grid_by_hand():
    ids = R.region_ids(16, 16)
    # rows / columns 0..7 -> 0, 8..11 -> 1, 12..15 -> 2; id = 3 * row class + column class
    assert int(ids[0, 0]) == 0 and int(ids[7, 7]) == 0 and int(ids[7, 8]) == 1 and int(ids[7, 12]) == 2
    assert int(ids[8, 0]) == 3 and int(ids[11, 11]) == 4 and int(ids[12, 12]) == 8 and int(ids[15, 3]) == 6 and int(ids[9, 15]) == 5
    mask = R.shift_mask(16, 16)
    assert mask.shape == (4, 64, 64) and set(mask.unique().tolist()) == {-100.0, 0.0}
    assert bool((mask[0] == 0).all())                                    # window (0, 0): one region
    # window (0, 1) = columns 8..15: local columns 0..3 are region 1, 4..7 region 2
    assert float(mask[1, 0, 3]) == 0 and float(mask[1, 0, 4]) == -100 and float(mask[1, 4, 12]) == 0 and float(mask[1, 3, 12]) == -100
    # window (1, 1): four regions; token (3, 3) = 27 and (4, 4) = 36 differ, (0, 0) and (3, 3) agree
    assert float(mask[3, 27, 36]) == -100 and float(mask[3, 0, 27]) == 0 and float(mask[3, 36, 63]) == 0
    # an 8 x 8 grid: rows 0..3 -> class 1 (the slice (0, -8) is empty), 4..7 -> 2
    small = R.region_ids(8, 8)
    assert int(small[0, 0]) == 4 and int(small[3, 4]) == 5 and int(small[4, 3]) == 7 and int(small[7, 7]) == 8


def test_reference_one_block_network_by_hand():
    """C 2, one head, one block, 1conv, x2, an 8 x 8 image whose channel 0 is 0.75 in the left half and 0.25 in the right.
    conv_first: feature 0 = 10 (x0 - 0.4488), feature 1 = -feature 0 (centre taps) -> (3.012, -3.012) | (-1.988, 1.988).
    patch_embed.norm (gamma 1, beta 0): mean 0, so (s, -s) with s = +-1 (to eps / f^2 ~ 1e-6).  The block's linears are all zero: its
    two branches add nothing; the layer's conv is zero: t stays.  norm: (s, -s) again.  conv_after_body: 3 x token feature 0 (centre tap)
    into feature 0, plus the skip f: 6.012 | -4.988.  conv_before_upsample.0 copies feature 0, LeakyReLU(0.01): 6.012 | -0.04988.
    conv_up1 copies it after the nearest x2, LeakyReLU(0.2): 6.012 | -0.009976; conv_hr the same: 6.012 | -0.0019952.
    conv_last: 0.1 x feature 0 into output channel 1, plus the mean: 0.4371 + 0.6012 | 0.4371 - 0.00019952; channels 0 and 2 are the mean."""
    sd = zeros_state_dict(2, (1,), 1, scale=2)
    sd["conv_first.weight"][0, 0, 1, 1], sd["conv_first.weight"][1, 0, 1, 1] = 10.0, -10.0
    sd["patch_embed.norm.weight"].fill_(1.0)
    sd["norm.weight"].fill_(1.0)
    sd["layers.0.residual_group.blocks.0.norm1.weight"].fill_(1.0)
    sd["layers.0.residual_group.blocks.0.norm2.weight"].fill_(1.0)
    sd["conv_after_body.weight"][0, 0, 1, 1] = 3.0
    for n in ("conv_before_upsample.0", "conv_up1", "conv_hr"):
        sd[n + ".weight"][0, 0, 1, 1] = 1.0
    sd["conv_last.weight"][1, 0, 1, 1] = 0.1
    x = torch.zeros(1, 3, 8, 8)
    x[:, 0, :, :4], x[:, 0, :, 4:] = 0.75, 0.25
    y = R.forward(sd, x)
    assert y.shape == (1, 3, 16, 16)
    want = torch.tensor(R.MEAN).view(1, 3, 1, 1).expand(1, 3, 16, 16).clone()
    want[:, 1, :, :8] += 0.6012
    want[:, 1, :, 8:] -= 0.00019952
    assert torch.allclose(y, want, atol=2e-6), float((y - want).abs().max())
    assert R.config_of(sd) == dict(embed_dim=2, depths=(1,), num_heads=1, mlp_hidden=4, resi_3conv=0, scale=2)


def test_reference_pads_by_reflection_and_crops():
    """19 x 13: the padded run equals the run on the explicitly reflect-padded 24 x 16 image, cropped."""
    sd = R.make_state_dict(60, (2,), 2, "1conv", 2)
    x = R.image(1, 19, 13, 12)
    padded = torch.nn.functional.pad(x, (0, 3, 0, 5), "reflect")
    assert torch.equal(R.forward(sd, x), R.forward(sd, padded)[:, :, :38, :26])


# ---- the GPU tests' inputs are fit for their rule -----------------------------------------------------------------------------------
def test_gpu_test_inputs_are_fit_for_the_comparison_rule():
    """For every net and image of tests/test_gpu_swinir.py, on the reference alone: fewer than 5 % of the output bytes are 0 or 255, the
    twin's rel_l2 lies above 1e-4 and its worst slice within 2.5 x of it."""
    import test_gpu_swinir as G
    to_u8 = sub("upscaler").model_output_to_u8
    assert len(G.NET_CASES) == 5
    for name, (args, (b, h, w)) in G.NET_CASES.items():
        x, ref, twin = G.reference_for(name)
        assert x.shape == (b, 3, h, w) and torch.equal(torch.round(x * 255) / 255, x)
        assert ref.shape == (b, 3, h * args[4], w * args[4])
        u8 = to_u8(ref.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, name
        yard = rel_l2(twin, ref)
        assert yard > 1e-4, (name, yard)
        for keep in ((1,), (0, 2)):
            assert worst_slice_rel_l2(twin, ref, keep)[0] <= 2.5 * yard, (name, keep)


# ---- the kernels as compiled --------------------------------------------------------------------------------------------------------
# csrc/swinir.hip holds exactly these kernels (fragments of the mangled names; ILb0E / ILb1E: the template argument COSINE false / true)
SWIN_KERNELS = {"attn": "swin_window_attn_kernelILb0E", "cosine_attn": "swin_window_attn_kernelILb1E",
                "layernorm": "swin_layernorm_kernelE", "layernorm_add": "swin2_layernorm_add_kernelE",
                "input": "swin_input_kernelE", "lrelu": "swin_lrelu_kernelE", "output": "swin_output_kernelE",
                "pixel_shuffle": "swin2_pixel_shuffle_kernelE", "output_shuffle": "swin2_output_shuffle_kernelE"}


def swin_kernel_meta():
    """-> (the gfx950 assembly of csrc/swinir.hip, {key of SWIN_KERNELS: (mangled name, its metadata counts)}); the file must hold the
    nine kernels of SWIN_KERNELS and no other."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("swinir")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    assert len(meta) == 9, sorted(meta)
    found = {}
    for key, frag in SWIN_KERNELS.items():
        names = [n for n in meta if frag in n]
        assert len(names) == 1, (key, sorted(meta))
        found[key] = (names[0], meta[names[0]])
    assert len({n for n, _ in found.values()}) == 9, sorted(meta)
    return asm, found


def test_swinir_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of csrc/swinir.hip, from the metadata: no kernel has scratch or spills; swin_window_attn (the plain
    instantiation) stays within 256 VGPRs (two workgroups of 4 waves per CU) and its body holds the MFMAs."""
    asm, found = swin_kernel_meta()
    for name, m in found.values():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    attn = [found["attn"][0]]
    assert found["attn"][1]["vgpr_count"] <= 256, found
    body = asm[asm.index(attn[0] + ":"):]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body
    assert "v_mfma_f32_16x16x32_f16" in body or "v_mfma_f32_32x32x16_f16" in body
