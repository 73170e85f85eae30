"""CPU tier of the Swin2SR path: the reference restatement pinned end to end to the `transformers` port, the checkpoint loader and
dispatcher, the loader's host precompute (bias table, head scales, folded projections), the webui hook, the fitness of the GPU tests'
inputs for their comparison rule, the compiled kernels' metadata, and one run of tests/test_gpu_swin2sr.py on the host-emulated
library."""
import importlib
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import rrdb_reference as RR
import swin2sr_reference as R
import swinir_reference as SR
from helpers import rel_l2, worst_slice_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases of tests/test_gpu_swin2sr.py: attention 7 + zero rows + mask + wide rows + refusals | layernorm_add 6 + in place + refusals
# | networks 9 + arena size + uint8 3 + handles | do_upscale + registry
GPU_FILE_CASES = (7 + 1 + 1 + 1 + 1) + (6 + 1 + 1) + (9 + 1 + 3 + 1) + (1 + 1)


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_swin2sr_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_swin2sr.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == GPU_FILE_CASES, out[-2000:]


# ---- the reference, pinned to transformers ------------------------------------------------------------------------------------------
def to_transformers_keys(sd):
    """The original key layout (network_swin2sr.py) -> Swin2SRForImageSuperResolution's; the three buffers are dropped (the port
    recomputes them)."""
    out = {}
    c = sd["conv_first.weight"].shape[0]
    for k, v in sd.items():
        if k.endswith(("relative_coords_table", "relative_position_index", "attn_mask")):
            continue
        m = re.match(r"layers\.(\d+)\.residual_group\.blocks\.(\d+)\.(.+)$", k)
        if m:
            pre, rest = f"swin2sr.encoder.stages.{m.group(1)}.layers.{m.group(2)}.", m.group(3)
            if rest == "attn.qkv.weight":
                for i, n in enumerate(("query", "key", "value")):
                    out[pre + f"attention.self.{n}.weight"] = v[c * i:c * (i + 1)]
                continue
            rest = {"attn.q_bias": "attention.self.query.bias", "attn.v_bias": "attention.self.value.bias",
                    "attn.logit_scale": "attention.self.logit_scale"}.get(rest, rest)
            for a, b in (("attn.cpb_mlp.", "attention.self.continuous_position_bias_mlp."), ("attn.proj.", "attention.output.dense."),
                         ("norm1.", "layernorm_before."), ("norm2.", "layernorm_after."), ("mlp.fc1.", "intermediate.dense."),
                         ("mlp.fc2.", "output.dense.")):
                if rest.startswith(a):
                    rest = b + rest[len(a):]
            out[pre + rest] = v
            continue
        m = re.match(r"layers\.(\d+)\.(conv\..+|patch_embed\.proj\.(weight|bias))$", k)
        if m:
            out[f"swin2sr.encoder.stages.{m.group(1)}." + m.group(2).replace("patch_embed.proj", "patch_embed.projection")] = v
            continue
        for a, b in (("conv_first.", "swin2sr.first_convolution."), ("patch_embed.proj.", "swin2sr.embeddings.patch_embeddings.projection."),
                     ("patch_embed.norm.", "swin2sr.embeddings.patch_embeddings.layernorm."), ("norm.", "swin2sr.layernorm."),
                     ("conv_after_body.", "swin2sr.conv_after_body."), ("conv_before_upsample.0.", "upsample.conv_before_upsample."),
                     ("conv_up1.", "upsample.conv_up1."), ("conv_up2.", "upsample.conv_up2."), ("conv_hr.", "upsample.conv_hr."),
                     ("conv_last.", "upsample.final_convolution.")):
            if k.startswith(a):
                out[b + k[len(a):]] = v
                break
        else:
            assert k.startswith("upsample."), k
            cfg = R.config_of(sd)
            step, leaf = k.split(".")[1:]
            if cfg["upsampler"] == "pixelshuffledirect":
                out["upsample.conv." + leaf] = v
            elif cfg["scale"] == 3:
                out["upsample.upsample.convolution." + leaf] = v
            else:
                out[f"upsample.upsample.convolution_{int(step) // 2}.{leaf}"] = v
    return out


@pytest.mark.parametrize("upsampler,scale,resi,hw", [("nearest+conv", 4, "1conv", (16, 24)), ("pixelshuffle", 4, "1conv", (16, 24)),
                                                     ("pixelshuffle", 3, "1conv", (8, 16)), ("pixelshuffledirect", 2, "1conv", (24, 16))])
def test_reference_equals_transformers_swin2sr(upsampler, scale, resi, hw):
    """The whole model, float64, against Swin2SRForImageSuperResolution with the same weights (image_size 64: shifted blocks keep
    their shift).  Sides are multiples of 8: the port un-embeds with the unpadded size.  Every logit_scale is ln 10: the port's
    Swin2SRSelfAttention.forward adds the shift mask twice (-200 where the original has -100), and on such weights a masked key is below
    e^-60 of the row either way — the reference applies the mask once, as the original does.  1conv throughout: the port builds
    conv_after_body as one conv whatever resi_connection says."""
    transformers = pytest.importorskip("transformers")
    sd = R.make_state_dict(60, (2, 2), 6, resi, scale, upsampler, seed=5)
    for k in sd:
        if k.endswith("logit_scale"):
            sd[k] = torch.full_like(sd[k], math.log(10.0))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    cfg = transformers.Swin2SRConfig(image_size=64, patch_size=1, num_channels=3, num_channels_out=3, embed_dim=60, depths=[2, 2], num_heads=[6, 6],
                                     window_size=8, mlp_ratio=2.0, qkv_bias=True, hidden_act="gelu", upscale=scale, img_range=1.0,
                                     resi_connection=resi, upsampler=upsampler)
    model = transformers.Swin2SRForImageSuperResolution(cfg).eval().double()
    model.load_state_dict(to_transformers_keys(sd), strict=True)
    with torch.no_grad():                                      # the port keeps the mean as an fp32 buffer: .double() of it is 1e-8 off the decimal constants
        model.swin2sr.mean.copy_(torch.tensor(R.MEAN, dtype=torch.float64).view(1, 3, 1, 1))
    x = R.image(2, hw[0], hw[1], 31).double()
    with torch.no_grad():
        theirs = model(pixel_values=x).reconstruction
    ours = R.forward(sd, x)
    assert ours.shape == theirs.shape == (2, 3, hw[0] * scale, hw[1] * scale)
    assert rel_l2(ours, theirs) <= 1e-9, rel_l2(ours, theirs)
    x32 = x.float()
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    assert rel_l2(R.forward(sd32, x32).double(), theirs) <= 2e-5                # the fp32 form the GPU tests use


def test_reference_pads_by_reflection_and_crops():
    sd = R.make_state_dict(60, (2,), 6, "1conv", 2, "pixelshuffledirect")
    x = R.image(1, 19, 13, 12)
    padded = torch.nn.functional.pad(x, (0, 3, 0, 5), "reflect")
    assert torch.equal(R.forward(sd, x), R.forward(sd, padded)[:, :, :38, :26])


def test_folded_projection_is_the_same_function():
    sd = R.make_state_dict(60, (2, 2), 6, "3conv", 2, "pixelshuffle")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    folded = R.fold_projections(sd)
    assert "layers.0.patch_embed.proj.weight" in sd and not any("layers.0.patch_embed.proj" in k for k in folded) and "patch_embed.proj.weight" in folded
    x = R.image(1, 16, 16, 3).double()
    assert rel_l2(R.forward(folded, x), R.forward(sd, x)) < 1e-12


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def blob_of(sd, cfg):
    """The documented order (include/sdmi.h at sdmi_swin2sr_config), written out independently of the loader, from the reference's
    bias table / head scale and folded projections."""
    c = cfg["embed_dim"]
    f = R.fold_projections(sd)

    def wb(n):
        return [f[n + ".weight"].flatten(), f[n + ".bias"].flatten()]

    def resi(stem):
        return sum((wb(f"{stem}.{k}") for k in (0, 2, 4)), []) if cfg["resi_3conv"] else wb(stem)
    parts = wb("conv_first")
    parts += wb("patch_embed.proj") if "patch_embed.proj.weight" in sd else [torch.eye(c).flatten(), torch.zeros(c)]
    parts += wb("patch_embed.norm")
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            parts += [f[b + "attn.qkv.weight"].flatten(), R.qkv_bias(f, b, c), R.bias_table(f, b).flatten(), R.head_scale(f, b)]
            parts += wb(b + "attn.proj") + wb(b + "norm1") + wb(b + "mlp.fc1") + wb(b + "mlp.fc2") + wb(b + "norm2")
        parts += resi(f"layers.{i}.conv")
    parts += wb("norm") + resi("conv_after_body")
    if cfg["upsampler"] == "nearest+conv":
        parts += wb("conv_before_upsample.0") + wb("conv_up1") + wb("conv_up2") + wb("conv_hr") + wb("conv_last")
    elif cfg["upsampler"] == "pixelshuffle":
        parts += wb("conv_before_upsample.0") + wb("upsample.0") + (wb("upsample.2") if cfg["scale"] == 4 else []) + wb("conv_last")
    else:
        parts += wb("upsample.0")
    return torch.cat(parts).float().numpy()


LOADER_CASES = [((60, (2, 2), 6, "1conv", 4, "nearest+conv"), {}), ((60, (1, 3), 6, "3conv", 2, "pixelshuffle"), {}),
                ((60, (2,), 6, "1conv", 3, "pixelshuffle"), {}), ((60, (2,), 6, "1conv", 4, "pixelshuffle"), {}),
                ((60, (2,), 6, "1conv", 3, "pixelshuffledirect"), {"proj": False}), ((180, (2,), 6, "1conv", 4, "pixelshuffledirect"), {})]


@pytest.mark.parametrize("args,kw", LOADER_CASES)
def test_loader_blob_is_the_documented_concatenation(args, kw):
    up = sub("upscaler")
    sd = R.make_state_dict(*args, **kw)
    blob, cfg = up.parse_swin2sr_state_dict(sd)
    assert cfg == R.config_of(sd) and cfg["depths"] == tuple(args[1]) and cfg["upsampler"] == args[5] and cfg["scale"] == args[4]
    want = blob_of(sd, cfg)
    assert blob.dtype == np.float32 and blob.shape == want.shape
    assert np.allclose(blob, want, rtol=2e-6, atol=2e-6), float(np.abs(blob - want).max())      # two fp32 evaluations of the cpb MLP / the fold
    for wrapper in ("params_ema", "params"):
        assert np.array_equal(up.parse_swin2sr_state_dict({wrapper: sd})[0], blob)


def test_loader_precomputes_the_bias_table_and_the_head_scales():
    """The table against the reference's float64 evaluation and, at three offsets, against the formula by hand; head_scale clamped."""
    up = sub("upscaler")
    sd = R.make_state_dict(60, (2,), 6, "1conv", 2, "pixelshuffledirect")
    pre = "layers.0.residual_group.blocks.1."
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    table = up.swin2sr_bias_table(sd[pre + "attn.cpb_mlp.0.weight"].numpy(), sd[pre + "attn.cpb_mlp.0.bias"].numpy(), sd[pre + "attn.cpb_mlp.2.weight"].numpy())
    assert table.shape == (225, 6) and table.dtype == np.float32
    coords64 = R.coords_table(torch.float64)
    w0, b0, w2 = (sd64[pre + n] for n in ("attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias", "attn.cpb_mlp.2.weight"))
    want = 16 * torch.sigmoid(torch.relu(coords64 @ w0.T + b0) @ w2.T)
    assert np.abs(table - want.numpy()).max() < 2e-5
    assert 0 < table.min() < 4 and 12 < table.max() < 16                            # the test weights spread the bias across (0, 16)
    coords = up.swin2sr_coords_table()
    assert coords.shape == (225, 2) and np.allclose(coords, R.coords_table().numpy(), atol=1e-7)
    top = math.log2(9) / 3                                                       # offset 7 -> 8 -> log2(8 + 1) / log2(8)
    assert np.allclose(coords[112], (0, 0)) and np.allclose(coords[0], (-top, -top)) and np.allclose(coords[224], (top, top))
    assert np.allclose(coords[7 * 15 + 8], (0, math.log2(8 / 7 + 1) / 3))         # (dy, dx) = (0, 1)
    scale = up.swin2sr_head_scale(sd[pre + "attn.logit_scale"].numpy())
    raw = sd[pre + "attn.logit_scale"].flatten()
    assert np.allclose(scale, np.exp(np.minimum(raw.numpy(), math.log(100.0))), rtol=1e-6) and scale.max() <= 100.0 * (1 + 1e-6)
    assert np.allclose(up.swin2sr_head_scale(np.array([math.log(250.0), math.log(3.0)])), [100.0, 3.0], rtol=1e-6)
    # some head of the test weights sits above the clamp
    assert any(float(v.max()) > math.log(100.0) for k, v in R.make_state_dict(60, (2, 2), 6).items() if k.endswith("logit_scale"))
    # where they sit in the blob: after conv_first, the projection, the norm, and the block's qkv
    blob, _ = up.parse_swin2sr_state_dict(sd)
    c = 60
    off = (c * 27 + c) + (c * c + c) + 2 * c
    per_block = (3 * c * c + 3 * c) + 226 * 6 + (c * c + c) + 2 * c + (120 * c + 120) + (c * 120 + c) + 2 * c
    at = off + per_block + 3 * c * c + 3 * c
    assert np.array_equal(blob[at:at + 225 * 6].reshape(225, 6), table) and np.array_equal(blob[at + 1350:at + 1356], scale)
    q_bias = blob[at - 3 * c:at]
    assert np.array_equal(q_bias[:c], sd[pre + "attn.q_bias"].numpy()) and not q_bias[c:2 * c].any() and np.array_equal(q_bias[2 * c:], sd[pre + "attn.v_bias"].numpy())


def test_loader_reads_the_shipped_shapes_and_missing_biases():
    up = sub("upscaler")
    sd = R.make_state_dict(180, (1,) * 6, 6, "1conv", 4, "nearest+conv")                 # the webui's *.v2.pth geometry, one block per layer
    for k in [k for k in sd if k.endswith(("q_bias", "v_bias"))]:
        del sd[k]                                                                         # qkv_bias = False
    blob, cfg = up.parse_swin2sr_state_dict(sd)
    assert cfg == dict(embed_dim=180, depths=(1,) * 6, num_heads=6, mlp_hidden=360, resi_3conv=0, upsampler="nearest+conv", scale=4)
    c = 180
    at = (c * 27 + c) + (c * c + c) + 2 * c + 3 * c * c
    assert not blob[at:at + 3 * c].any()


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_swin2sr_state_dict
    base = R.make_state_dict(60, (2,), 6, "1conv", 2, "pixelshuffle")

    def variant(drop=(), **put):
        sd = {k: v for k, v in base.items() if not any(k.startswith(d) for d in drop)}
        sd.update(put)
        return sd
    z = torch.zeros
    with pytest.raises(ValueError, match="pixelshuffle_aux"):
        parse(variant(**{"conv_bicubic.weight": z(64, 3, 3, 3), "conv_aux.weight": z(3, 64, 3, 3)}))
    with pytest.raises(ValueError, match="without an upsampler"):
        parse(variant(drop=("upsample.", "conv_before_upsample.")))
    with pytest.raises(ValueError, match="window_size 7"):
        parse(variant(**{"layers.0.residual_group.blocks.0.attn.relative_position_index": z(49, 49, dtype=torch.long)}))
    with pytest.raises(ValueError, match="window_size 16"):
        parse(variant(**{"layers.0.residual_group.blocks.1.attn_mask": z(16, 256, 256)}))
    with pytest.raises(ValueError, match="window_size 7"):
        parse(variant(**{"layers.0.residual_group.blocks.0.attn.relative_coords_table": z(1, 13, 13, 2)}))
    with pytest.raises(ValueError, match="head_dim = 240/6 = 40"):
        parse(R.make_state_dict(240, (1,), 6, "1conv", 2, "pixelshuffledirect"))
    with pytest.raises(ValueError, match="takes 1 input channels"):
        parse(variant(**{"conv_first.weight": z(60, 1, 3, 3)}))
    with pytest.raises(ValueError, match="ape"):
        parse(variant(absolute_pos_embed=z(1, 4096, 60)))
    with pytest.raises(ValueError, match="num_feat = 32"):
        parse(variant(**{"conv_before_upsample.0.weight": z(32, 60, 3, 3)}))
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(**{"upsample.0.weight": z(1024, 64, 3, 3)}))                                  # a single x4 step
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(**{"upsample.2.weight": z(256, 64, 3, 3), "upsample.2.bias": z(256), "upsample.4.weight": z(256, 64, 3, 3)}))     # x8
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(drop=("conv_before_upsample.", "conv_last."), **{"upsample.0.weight": z(75, 60, 3, 3)}))     # pixelshuffledirect x5
    with pytest.raises(ValueError, match="scale 4 only"):
        parse(variant(drop=("upsample.",), **{"conv_up1.weight": z(64, 64, 3, 3), "conv_hr.weight": z(64, 64, 3, 3)}))
    sd = variant()
    del sd["layers.0.residual_group.blocks.1.mlp.fc2.bias"]
    with pytest.raises(ValueError, match=r"lacks layers\.0\.residual_group\.blocks\.1\.mlp\.fc2\.bias"):
        parse(sd)
    with pytest.raises(ValueError, match="not a Swin2SR checkpoint"):
        parse(SR.make_state_dict(60, (2,), 2, "1conv", 2))


# ---- the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_sends_swin2sr_to_its_own_loader_and_leaves_swinir_alone():
    up = sub("upscaler")
    v2 = R.make_state_dict(60, (2,), 6, "1conv", 3, "pixelshuffle")
    for sd in (v2, {"params_ema": v2}, {"params": v2}):
        assert up.upscaler_family(sd) == "swin2sr"
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "swin2sr" and parsed[-1] == 3 and parsed[1] == R.config_of(v2)
        assert np.array_equal(parsed[0], up.parse_swin2sr_state_dict(v2)[0])
    with pytest.raises(ValueError, match="SwinIR"):                                  # the SwinIR parser itself still refuses such a file
        up.parse_swinir_state_dict(v2)
    v1 = SR.make_state_dict(60, (2,), 2, "1conv", 2)
    assert up.upscaler_family(v1) == "swinir" and up.parse_upscaler_state_dict(v1)[0] == "swinir"
    import test_cpu_swinir as T1
    for kw in (dict(), dict(c=180, depths=(2,), heads=6, scale=2), dict(c=240, depths=(2,), heads=8, resi3=True)):
        zsd = T1.zeros_state_dict(**kw)                                             # the existing zero dicts: unchanged answers
        assert up.upscaler_family(zsd) == "swinir"
        blob, cfg = up.parse_swinir_state_dict(zsd)
        assert not blob.any() and np.array_equal(blob, T1.blob_of(zsd, cfg))
    with pytest.raises(ValueError, match="upsampler 'pixelshuffle'.*nearest\\+conv"):
        up.parse_swinir_state_dict(T1.zeros_state_dict(upsampler="pixelshuffle"))
    assert up.upscaler_family(RR.make_state_dict(1, 4)) == "rrdb"
    with pytest.raises(ValueError, match="head_dim"):                                 # a Swin2SR the engine refuses: that loader's message
        up.parse_upscaler_state_dict(R.make_state_dict(240, (1,), 6, "1conv", 2, "pixelshuffledirect"))


def test_make_upscaler_net_picks_swin2srnet(monkeypatch, tmp_path):
    up, shared = sub("upscaler"), sub("shared")
    made = []
    for cls, tag in ((up.SwinIRNet, "swinir"), (up.Swin2SRNet, "swin2sr")):
        monkeypatch.setattr(cls, "__init__", lambda self, sd, device=0, engine=None, _t=tag: made.append(_t))
    v2 = R.make_state_dict(60, (2,), 6, "1conv", 2, "pixelshuffledirect")
    assert type(up.make_upscaler_net({"params_ema": v2})) is up.Swin2SRNet
    assert type(up.make_upscaler_net(SR.make_state_dict(60, (2,), 2, "1conv", 2))) is up.SwinIRNet
    assert made == ["swin2sr", "swinir"] and issubclass(up.Swin2SRNet, up.SwinIRNet) and up.Swin2SRNet._abi == "sdmi_swin2sr"
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save({"params_ema": R.make_state_dict(60, (2,), 6, "1conv", 3, "pixelshuffle")}, str(tmp_path / "swin2sr_classical_x3.pth"))
    added = up.register_esrgan([str(tmp_path / "swin2sr_classical_x3.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "swin2sr_classical_x3"] and added[0].scale == 3


# ---- the webui hook ---------------------------------------------------------------------------------------------------------------
def test_install_swinir_hook_runs_a_swin2sr_file_on_the_engine(tmp_path, monkeypatch):
    """An UpscalerSwinIR entry that points at a Swin2SR file (what the extension builds from swinir_model_arch_v2.py) runs on the
    engine; a pixelshuffle_aux file stays on the stock path."""
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, aux = str(tmp_path / "Swin2SR_RealworldSR_X4_64_BSRGAN_PSNR.v2.pth"), str(tmp_path / "Swin2SR_CompressedSR_X4_48.pth")
    v2 = R.make_state_dict(60, (2,), 6, "1conv", 4, "nearest+conv")
    torch.save({"params_ema": v2}, good)
    torch.save({"params": dict(v2, **{"conv_bicubic.weight": torch.zeros(64, 3, 3, 3), "conv_aux.weight": torch.zeros(3, 64, 3, 3)})}, aux)

    class UpscalerSwinIR:                                      # the shape of the extension's scaler object
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, model_file):
            self.stock_calls.append(model_file)
            return img
    scaler = UpscalerSwinIR()
    data = [types.SimpleNamespace(name="Swin2SR 4x", data_path=good, local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="Swin2SR aux", data_path=aux, local_data_path=aux, scaler=scaler)]
    scaler.scalers = data
    engine_calls, families = [], []

    def load_model(self, path):
        family, parsed = up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(path))
        families.append(family)
        return parsed
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", load_model)
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    shared = types.SimpleNamespace(sd_upscalers=data)
    assert bridge.install_swinir_hook(shared) == ["Swin2SR 4x", "Swin2SR aux"]
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, good)
    assert engine_calls == [good] and scaler.stock_calls == [] and families == ["swin2sr"]
    scaler.do_upscale(img, aux)
    assert engine_calls == [good] and scaler.stock_calls == [aux]


# ---- the GPU tests' inputs are fit for their rule -----------------------------------------------------------------------------------
def test_gpu_test_inputs_are_fit_for_the_comparison_rule():
    """For every attention case, LayerNorm case and net of tests/test_gpu_swin2sr.py, on the reference alone: the twin's rel_l2 lies
    above 1e-4 and its worst slice within 2.5 x of it; the nets' outputs stay inside [0, 1] on all but a few per cent of the bytes and
    the twin flips few of them; the crafted mask case tells -100 from -inf."""
    import test_gpu_swin2sr as G
    to_u8 = sub("upscaler").model_output_to_u8

    def fit(twin, ref, channel_dim, row_dims, ctx):
        yard = rel_l2(twin.double(), ref.double())
        assert yard > 1e-4, (ctx, yard)
        for keep in ((channel_dim,), row_dims):
            assert worst_slice_rel_l2(twin.double(), ref.double(), keep)[0] <= 2.5 * yard, (ctx, keep)
        return yard
    assert len(G.ATTN_SHAPES) == 7
    for b, h, w, heads, d, shift in G.ATTN_SHAPES:
        case = G.attn_case(b, h, w, heads, d, G.attn_seed(b, h, w, heads, d))
        ref = G.graph(case, shift)
        yard = fit(G.graph(case, shift, G.r16d), ref, 3, (0, 1), (b, h, w, heads, d, shift))
        assert float(case["scale"].min()) >= 3 and float(case["scale"].max()) <= 100 and 0 < float(case["table"].min()) and float(case["table"].max()) < 16
        assert rel_l2(graph_no(G, case, shift, "bias"), ref) > 10 * yard and rel_l2(graph_no(G, case, shift, "scale"), ref) > 10 * yard
        if shift:
            assert rel_l2(graph_no(G, case, shift, "mask"), ref) > 10 * yard
            assert rel_l2(G.graph(case, shift, mask_value=-math.inf), ref) < 0.01 * yard      # random data cannot tell the two masks apart
    crafted = G.crafted_mask_case()
    ref = G.graph(crafted, 4)
    yard = fit(G.graph(crafted, 4, G.r16d), ref, 3, (0, 1), "crafted")
    assert rel_l2(G.graph(crafted, 4, mask_value=-math.inf), ref) > 10 * yard
    for c, ld in ((60, 64), (180, 192), (240, 256)):
        for rows in (130, 1):
            y, resid, g, b = G.lnadd_inputs(rows, c, ld, 140 + c)
            ref = G.lnadd_ref(y, resid, g, b, c)
            fit(G.r16d(ref), ref, 1, (0,), ("layernorm_add", c, ld, rows))
    assert len(G.NET_CASES) == 9 and {a[5] for a, _, _ in G.NET_CASES.values()} == set(R.UPSAMPLERS)
    for name, (args, kw, (b, h, w)) in G.NET_CASES.items():
        x, ref, twin = G.reference_for(name)
        assert x.shape == (b, 3, h, w) and torch.equal(torch.round(x * 255) / 255, x)
        assert ref.shape == (b, 3, h * args[4], w * args[4])
        u8 = to_u8(ref.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, name
        fit(twin, ref, 1, (0, 2), name)
        assert G.twin_flip_share(name) < 0.1, name


def graph_no(G, case, shift, what):
    return G.graph(case, shift, **{what: False})


# ---- the kernels as compiled --------------------------------------------------------------------------------------------------------
def test_swin2sr_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of csrc/swinir.hip (which holds Swin2SR's kernels too), from the metadata: no kernel has scratch or spills;
    swin2_layernorm_add stays within 128 VGPRs, the cosine instantiation of swin_window_attn within 256 (two workgroups
    of 4 waves per CU) with the MFMAs in its body."""
    from test_cpu_swinir import swin_kernel_meta
    asm, found = swin_kernel_meta()
    for name, m in found.values():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert found["layernorm_add"][1]["vgpr_count"] <= 128, found
    attn = [found["cosine_attn"][0]]
    assert found["cosine_attn"][1]["vgpr_count"] <= 256, found
    body = asm[asm.index(attn[0] + ":"):]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body and body.count("v_mfma_f32_16x16x32_f16") >= 32
