"""CPU tier of the ScuNET path: the host-only parts (checkpoint loader and dispatcher, webui hook, the reference restatement itself,
pinned to an independent implementation and to answers worked out by hand), the fitness of the GPU tests' inputs for their comparison
rule, the compiled kernels' metadata, and one run of tests/test_gpu_scunet.py on the host-emulated library."""
import importlib
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import compact_reference as CR
import rrdb_reference as RR
import scunet_reference as R
import swinir_reference as SR
from helpers import rel_l2, worst_slice_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE_CASES = 7 + 1 + 2 + 1 + 2 + 4 + 1 + 1 + 1 + 1 + 1                     # the cases of tests/test_gpu_scunet.py


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_scunet_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_scunet.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= GPU_FILE_CASES, out[-2000:]


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def zeros_state_dict(depths=(1,) * 7, dim=64, in_nc=3, side=15):
    """The key layout of a SCUNet checkpoint, all zeros."""
    z = torch.zeros
    half = dim // 2
    sd = {"m_head.0.weight": z(dim, in_nc, 3, 3), "m_tail.0.weight": z(in_nc, dim, 3, 3)}
    for st, (stem, depth) in enumerate(zip(R.STAGES, depths)):
        c = half << (st if st < 4 else 6 - st)
        d, first = 2 * c, (1 if st > 3 else 0)
        if st > 3:
            sd[f"{stem}.0.weight"] = z(2 * d, d, 2, 2)
        for i in range(first, first + depth):
            t = f"{stem}.{i}.trans_block."
            for n in ("ln1", "ln2"):
                sd[t + n + ".weight"], sd[t + n + ".bias"] = z(c), z(c)
            sd[t + "msa.relative_position_params"] = z(c // 32, side, side)
            for n, (o, k) in (("msa.embedding_layer", (3 * c, c)), ("msa.linear", (c, c)), ("mlp.0", (4 * c, c)), ("mlp.2", (c, 4 * c))):
                sd[t + n + ".weight"], sd[t + n + ".bias"] = z(o, k), z(o)
            for n in ("conv1_1", "conv1_2"):
                sd[f"{stem}.{i}.{n}.weight"], sd[f"{stem}.{i}.{n}.bias"] = z(d, d, 1, 1), z(d)
            sd[f"{stem}.{i}.conv_block.0.weight"], sd[f"{stem}.{i}.conv_block.2.weight"] = z(c, c, 3, 3), z(c, c, 3, 3)
        if st < 3:
            sd[f"{stem}.{depth}.weight"] = z(2 * d, d, 2, 2)
    return sd


def blob_of(sd, depths):
    """The documented order (include/sdmi.h at sdmi_scunet_config), written out independently of the loader."""
    parts = [sd["m_head.0.weight"]]
    for st, (stem, depth) in enumerate(zip(R.STAGES, depths)):
        first = 1 if st > 3 else 0
        if st > 3:
            parts.append(sd[f"{stem}.0.weight"])
        for i in range(first, first + depth):
            t = f"{stem}.{i}.trans_block."
            names = [t + "ln1.weight", t + "ln1.bias", t + "msa.relative_position_params"]
            for n in ("msa.embedding_layer", "msa.linear"):
                names += [t + n + ".weight", t + n + ".bias"]
            names += [t + "ln2.weight", t + "ln2.bias", t + "mlp.0.weight", t + "mlp.0.bias", t + "mlp.2.weight", t + "mlp.2.bias"]
            names += [f"{stem}.{i}.conv1_1.weight", f"{stem}.{i}.conv1_1.bias", f"{stem}.{i}.conv1_2.weight", f"{stem}.{i}.conv1_2.bias",
                      f"{stem}.{i}.conv_block.0.weight", f"{stem}.{i}.conv_block.2.weight"]
            parts += [sd[n] for n in names]
        if st < 3:
            parts.append(sd[f"{stem}.{depth}.weight"])
    parts.append(sd["m_tail.0.weight"])
    return torch.cat([p.flatten() for p in parts]).float().numpy()


def test_loader_reads_the_config_of_the_shipped_shapes():
    parse = sub("upscaler").parse_scunet_state_dict
    blob, cfg = parse(zeros_state_dict((4,) * 7))                                  # ScuNET GAN / ScuNET PSNR
    assert cfg == dict(depths=(4,) * 7, dim=64, scale=1)
    assert blob.dtype == np.float32 and blob.ndim == 1 and blob.size == sum(v.numel() for v in zeros_state_dict((4,) * 7).values())


@pytest.mark.parametrize("depths", [(1,) * 7, (2, 1, 1, 1, 1, 1, 2), (1, 2, 3, 1, 2, 1, 3)])
def test_loader_blob_is_the_documented_concatenation(depths):
    parse = sub("upscaler").parse_scunet_state_dict
    sd = R.make_state_dict(depths)
    blob, cfg = parse(sd)
    assert cfg == R.config_of(sd) and cfg["depths"] == depths
    assert np.array_equal(blob, blob_of(sd, depths))
    assert blob.size == sum(v.numel() for v in sd.values())                        # every tensor of the checkpoint, once


@pytest.mark.parametrize("wrapper", ["params_ema", "params"])
def test_loader_unwraps_the_training_wrappers(wrapper):
    parse = sub("upscaler").parse_scunet_state_dict
    sd = R.make_state_dict((1,) * 7)
    blob = parse(sd)[0]
    assert np.array_equal(parse({wrapper: sd})[0], blob)
    assert np.array_equal(parse({"params": zeros_state_dict(), "params_ema": sd})[0], blob)      # the EMA weights win


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_scunet_state_dict
    with pytest.raises(ValueError, match="dim = 128: the engine's kernels are built for 64"):
        parse(zeros_state_dict(dim=128))
    with pytest.raises(ValueError, match=r"window_size 4 \(relative_position_params \(1, 7, 7\)\)"):
        parse(zeros_state_dict(side=7))
    with pytest.raises(ValueError, match="in_nc = 1"):
        parse(zeros_state_dict(in_nc=1))
    sd = zeros_state_dict()
    del sd["m_up2.1.trans_block.mlp.2.bias"]
    with pytest.raises(ValueError, match=r"lacks m_up2\.1\.trans_block\.mlp\.2\.bias"):
        parse(sd)
    sd = zeros_state_dict()
    del sd["m_down2.1.weight"]                                                    # the stride-2 conv behind the stage's one block
    with pytest.raises(ValueError, match=r"lacks m_down2\.1\.weight"):
        parse(sd)
    sd = zeros_state_dict((2,) * 7)
    for k in [k for k in sd if k.startswith("m_body.0.")]:
        del sd[k]
    with pytest.raises(ValueError, match=r"m_body: blocks are not 0\.\.n: \[1\]"):
        parse(sd)
    sd = zeros_state_dict()
    sd["m_down3.0.conv_block.2.weight"] = torch.zeros(128, 128, 1, 1)
    with pytest.raises(ValueError, match=r"m_down3\.0\.conv_block\.2\.weight: \(128, 128, 1, 1\), expected \(128, 128, 3, 3\)"):
        parse(sd)
    with pytest.raises(ValueError, match="not a ScuNET checkpoint: no m_head.0.weight"):
        parse(RR.make_state_dict(1, 4))


# ---- the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_keeps_its_answers_and_sends_scunet_to_its_loader():
    up = sub("upscaler")
    scu = R.make_state_dict((1,) * 7)
    for sd in (scu, {"params_ema": scu}, {"params": scu}):
        assert up.upscaler_family(sd) == "scunet"
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "scunet" and parsed[-1] == 1 and parsed[1] == R.config_of(scu)
        assert np.array_equal(parsed[0], up.parse_scunet_state_dict(scu)[0])
    swin = SR.make_state_dict(60, (2,), 2, "1conv", 2)
    family, parsed = up.parse_upscaler_state_dict({"params_ema": swin})
    assert family == "swinir" and parsed[-1] == 2 and parsed[1] == SR.config_of(swin)
    rrdb = RR.make_state_dict(2, 4)
    for sd in (rrdb, RR.to_old_arch(rrdb, 2), {"params_ema": rrdb}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "rrdb" and parsed[1:] == (2, 3, 4)
    compact = CR.make_state_dict(4, 2)
    for sd in (compact, {"params": compact}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "compact" and parsed[1:] == (4, 2)
    with pytest.raises(ValueError, match="not an RRDBNet checkpoint"):
        up.parse_upscaler_state_dict({"m_head.0.weight": torch.zeros(64, 3, 3, 3)})        # one of the two marks alone is not a ScuNET
    with pytest.raises(ValueError, match="dim = 96"):                                      # a ScuNET the engine refuses: that loader's message
        up.parse_upscaler_state_dict(zeros_state_dict(dim=96))


def test_make_upscaler_net_picks_the_class_by_the_keys(monkeypatch):
    up = sub("upscaler")
    made = []
    for cls, tag in ((up.EsrganNet, "rrdb"), (up.CompactNet, "compact"), (up.SwinIRNet, "swinir"), (up.ScuNETNet, "scunet")):
        monkeypatch.setattr(cls, "__init__", lambda self, sd, device=0, engine=None, _t=tag: made.append(_t))
    assert isinstance(up.make_upscaler_net(RR.make_state_dict(1, 4)), up.EsrganNet)
    assert isinstance(up.make_upscaler_net({"params_ema": zeros_state_dict()}), up.ScuNETNet)
    assert made == ["rrdb", "scunet"]


def test_register_esrgan_takes_a_scunet_checkpoint(tmp_path, monkeypatch):
    up, shared = sub("upscaler"), sub("shared")
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save(zeros_state_dict((1,) * 7), str(tmp_path / "scunet_color_real_gan.pth"))
    torch.save(RR.make_state_dict(1, 4), str(tmp_path / "rrdb_x4.pth"))
    added = up.register_esrgan([str(tmp_path / "scunet_color_real_gan.pth"), str(tmp_path / "rrdb_x4.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "scunet_color_real_gan", "rrdb_x4"]
    assert [d.scale for d in added] == [1, 4]


def test_too_large_an_input_is_refused(monkeypatch):
    up = sub("upscaler")
    net = up.ScuNETNet.__new__(up.ScuNETNet)
    net.scale, net.device, net.handle = 1, 0, None
    net.engine = types.SimpleNamespace(arena_bytes=lambda: 1000)
    monkeypatch.setattr(up.ScuNETNet, "scratch_bytes", lambda self, b, h, w: 5000)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 4000)
    net.check_fits(1, 512, 512)
    net.check_fits(1, 1, 1)                                                       # any side: the padding is the engine's
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 3999)
    with pytest.raises(up.EsrganInputTooLarge, match=r"512x512 \(batch 1\) is too large for ScuNET"):
        net.check_fits(1, 512, 512)
    monkeypatch.setattr(up.ScuNETNet, "scratch_bytes", lambda self, b, h, w: 0)  # the engine's own refusal: a tensor of 2^31 elements
    with pytest.raises(up.EsrganInputTooLarge, match="2\\^31"):
        net.check_fits(1, 8192, 4096)


# ---- the webui hook ---------------------------------------------------------------------------------------------------------------
def test_install_scunet_hook_on_stub_scalers(tmp_path, monkeypatch):
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, wide = str(tmp_path / "ScuNET.pth"), str(tmp_path / "scunet_dim96.pth")
    torch.save(zeros_state_dict((1,) * 7), good)
    torch.save(zeros_state_dict(dim=96), wide)

    class UpscalerScuNET:                                      # the shape of the extension's scaler object
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, selected_file):
            self.stock_calls.append(selected_file)
            return img

    class UpscalerSwinIR(UpscalerScuNET):
        pass
    scaler, other = UpscalerScuNET(), UpscalerSwinIR()
    url = "https://example.invalid/scunet_color_real_psnr.pth"
    data = [types.SimpleNamespace(name="ScuNET GAN", data_path=good, local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="ScuNET wide", data_path=wide, local_data_path=wide, scaler=scaler),
            types.SimpleNamespace(name="ScuNET PSNR", data_path=url, local_data_path=None, scaler=scaler),
            types.SimpleNamespace(name="SwinIR 4x", data_path=good, local_data_path=good, scaler=other)]
    scaler.scalers = data[:3]
    engine_calls = []
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", lambda self, path: up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(path)))
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    shared = types.SimpleNamespace(sd_upscalers=data)
    assert bridge.install_scunet_hook(shared) == ["ScuNET GAN", "ScuNET wide", "ScuNET PSNR"]           # the SwinIR scaler is not this hook's
    hooked = scaler.do_upscale
    assert bridge.install_scunet_hook(shared) == ["ScuNET GAN", "ScuNET wide", "ScuNET PSNR"]           # idempotent
    assert scaler.do_upscale is hooked and not hasattr(other.do_upscale, "_mi355x_stock")
    assert bridge.install_swinir_hook(shared) == ["SwinIR 4x"] and scaler.do_upscale is hooked         # each hook keeps to its own class
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, good)
    assert engine_calls == [good] and scaler.stock_calls == []
    scaler.do_upscale(img, wide)                               # dim 96: the loader refuses, the stock path runs it
    assert engine_calls == [good] and scaler.stock_calls == [wide]
    scaler.do_upscale(img, url)                                # not on disk yet: the stock code downloads and runs it
    assert engine_calls == [good] and scaler.stock_calls == [wide, url]

    def too_large(self, img, path=None):
        raise up.EsrganInputTooLarge("too large")
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", too_large)
    scaler.do_upscale(img, good)
    assert scaler.stock_calls == [wide, url, good]


# ---- the reference, pinned --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(16, 16), (8, 8), (16, 24)])
def test_wmsa_mask_forbids_the_pairs_of_the_swin_region_mask(grid):
    """WMSA.generate_mask (the last row / column of windows, halves of the window) against Swin's region-id mask at shift 4: the same
    forbidden pairs, window for window."""
    h, w = grid
    ours = R.wmsa_mask(h // 8, w // 8).reshape(-1, 64, 64)
    theirs = SR.shift_mask(h, w, 4) != 0
    assert ours.shape == theirs.shape and torch.equal(ours, theirs)
    assert bool(ours.any()) and not bool(ours[:, torch.arange(64), torch.arange(64)].any())          # a token always sees itself


def test_relative_bias_at_three_pairs_by_hand():
    """bias[h][a][b] = params[h][ya - yb + 7][xa - xb + 7], tokens row-major in the window."""
    params = torch.arange(2 * 225, dtype=torch.float32).view(2, 15, 15)
    bias = R.relative_bias(params)
    assert bias.shape == (2, 64, 64)
    assert float(bias[0, 0, 0]) == 7 * 15 + 7 == 112                      # a token and itself: the centre
    assert float(bias[0, 0, 63]) == 0 and float(bias[1, 63, 0]) == 225 + 224          # (0,0) vs (7,7): (-7, -7) -> [0][0]; the other way [14][14]
    assert float(bias[1, 10, 3]) == 225 + (1 - 0 + 7) * 15 + (2 - 3 + 7) == 225 + 126      # (1,2) vs (0,3)


@pytest.mark.parametrize("shift", [0, 4])
def test_reference_block_equals_the_transformers_swin_layer(shift):
    """One Block of scunet_reference (trans_dim 64, 2 heads, 16 x 24) against transformers' SwinLayer with the same weights: an
    implementation written by other people (it puts -100 where WMSA puts -inf: the same probabilities to fp32 resolution)."""
    swin = pytest.importorskip("transformers.models.swin.modeling_swin")
    from transformers import SwinConfig
    sd, pre, c = {}, "b.", 64
    R.make_block(sd, pre, c, torch.Generator().manual_seed(3))
    layer = swin.SwinLayer(SwinConfig(window_size=8, mlp_ratio=4.0, hidden_act="gelu", layer_norm_eps=1e-5), c, (16, 24), 2, 0.0, shift).eval()
    qkv_w, qkv_b = sd[pre + "msa.embedding_layer.weight"], sd[pre + "msa.embedding_layer.bias"]
    mine = {"attention.relative_position_bias.relative_position_bias_table": sd[pre + "msa.relative_position_params"].reshape(2, 225).t(),
            "attention.o_proj.weight": sd[pre + "msa.linear.weight"], "attention.o_proj.bias": sd[pre + "msa.linear.bias"],
            "layernorm_before.weight": sd[pre + "ln1.weight"], "layernorm_before.bias": sd[pre + "ln1.bias"],
            "layernorm_after.weight": sd[pre + "ln2.weight"], "layernorm_after.bias": sd[pre + "ln2.bias"],
            "mlp.fc1.weight": sd[pre + "mlp.0.weight"], "mlp.fc1.bias": sd[pre + "mlp.0.bias"],
            "mlp.fc2.weight": sd[pre + "mlp.2.weight"], "mlp.fc2.bias": sd[pre + "mlp.2.bias"]}
    for i, n in enumerate("qkv"):
        mine[f"attention.{n}_proj.weight"], mine[f"attention.{n}_proj.bias"] = qkv_w[c * i:c * (i + 1)], qkv_b[c * i:c * (i + 1)]
    missing, unexpected = layer.load_state_dict(mine, strict=False)
    assert not unexpected and all("relative_position_index" in k for k in missing), (missing, unexpected)
    x = torch.randn((2, 16, 24, c), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        theirs = layer(x.reshape(2, 16 * 24, c), (16, 24))
    theirs = theirs[0] if isinstance(theirs, (tuple, list)) else theirs
    ours = R.block(sd, pre, x, shift).reshape(2, 16 * 24, c)
    assert torch.allclose(ours, theirs, rtol=1e-5, atol=1e-5), float((ours - theirs).abs().max())


def test_reference_tiny_network_by_hand():
    """Depths 1 x 7, every tensor zero but five: a ConvTransBlock with zero weights adds nothing, so each stage is the identity.
    Image channel 0 = 0.5 (x odd) + 0.25 (y odd): the 2 x 2 cells hold (0, 0.5 / 0.25, 0.75).
    m_head: feature 0 = 2 x channel 0 (centre tap)                                   -> cells (0, 1 / 0.5, 1.5) = x1[0]
    m_down1's conv: output 0 = (0.1, 0.2 / 0.3, 0.4) . cell of feature 0            -> 0.2 + 0.15 + 0.6 = 0.95 everywhere = x2[0]
    m_down2's conv is zero: x3 = x4 = 0, and m_body, m_up3, m_up2 carry zeros.
    m_up1: ConvTranspose2d of (0 + x2): input 0 -> output 1 with taps (1, 2 / 3, 4)  -> cells (0.95, 1.9 / 2.85, 3.8) in feature 1
    m_tail of (that + x1): out 0 = 0.5 x feature 0, out 1 = 0.1 x feature 1          -> channel 0 again; cells (0.095, 0.19 / 0.285, 0.38); 0."""
    sd = zeros_state_dict()
    sd["m_head.0.weight"][0, 0, 1, 1] = 2.0
    sd["m_down1.1.weight"][0, 0] = torch.tensor([[0.1, 0.2], [0.3, 0.4]])
    sd["m_up1.0.weight"][0, 1] = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    sd["m_tail.0.weight"][0, 0, 1, 1], sd["m_tail.0.weight"][1, 1, 1, 1] = 0.5, 0.1
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(128), indexing="ij")
    x = torch.zeros(1, 3, 64, 128)
    x[0, 0] = 0.5 * (xx % 2) + 0.25 * (yy % 2)
    y = R.forward(sd, x)
    assert y.shape == (1, 3, 64, 128)
    want = torch.zeros_like(x)
    want[0, 0] = x[0, 0]
    want[0, 1] = 0.095 * (1 + (xx % 2) + 2 * (yy % 2))
    assert torch.allclose(y, want, atol=2e-6), float((y - want).abs().max())
    assert R.config_of(sd) == dict(depths=(1,) * 7, dim=64, scale=1)


def test_reference_pads_by_replication_and_crops():
    """70 x 100: the padded run equals the run on the explicitly replicate-padded 128 x 128 image, cropped."""
    sd = R.make_state_dict((1,) * 7)
    x = R.image(1, 70, 100, 12)
    padded = F.pad(x, (0, 28, 0, 58), "replicate")
    assert float(padded[0, 1, 127, 127]) == float(x[0, 1, 69, 99]) and float(padded[0, 2, 100, 5]) == float(x[0, 2, 69, 5])
    assert torch.equal(R.forward(sd, x), R.forward(sd, padded)[:, :, :70, :100])


# ---- the GPU tests' inputs are fit for their rule -----------------------------------------------------------------------------------
def test_gpu_test_inputs_are_fit_for_the_comparison_rule():
    """For every net and image of tests/test_gpu_scunet.py, on the reference alone: fewer than 5 % of the output bytes are 0 or 255, the
    twin's rel_l2 lies above 1e-4 and its worst slice within 2.5 x of it."""
    import test_gpu_scunet as G
    to_u8 = sub("upscaler").model_output_to_u8
    assert len(G.NET_CASES) == 4 and G.SMALL in G.NET_CASES
    for name, (depths, (b, h, w)) in G.NET_CASES.items():
        x, ref, twin = G.reference_for(name)
        assert x.shape == (b, 3, h, w) and torch.equal(torch.round(x * 255) / 255, x)
        assert ref.shape == (b, 3, h, w)
        u8 = to_u8(ref.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, name
        yard = rel_l2(twin, ref)
        assert yard > 1e-4, (name, yard)
        for keep in ((1,), (0, 2)):
            assert worst_slice_rel_l2(twin, ref, keep)[0] <= 2.5 * yard, (name, keep)


# ---- the kernels as compiled --------------------------------------------------------------------------------------------------------
def test_scunet_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of csrc/scunet.hip, from the metadata: no kernel has scratch or spills; both widths of scu_block stay
    within 256 VGPRs and their bodies hold the f16 MFMA."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("scunet")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    assert len(meta) >= 7 and all("scu_" in n for n in meta), sorted(meta)
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    blocks = [n for n in meta if "scu_block_kernel" in n]
    assert len(blocks) == 2, sorted(meta)
    for name in blocks:
        assert meta[name]["vgpr_count"] <= 256, (name, meta[name])
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body
        assert "v_mfma_f32_16x16x32_f16" in body or "v_mfma_f32_32x32x16_f16" in body
