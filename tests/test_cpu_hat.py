"""CPU tier of the HAT path: the parts of the reference restatement pinned to torch (and the region mask to transformers' Swin), the
checkpoint loader (blob order, the two OCA index layouts, refusals) and dispatcher, the webui hook, the fitness of the GPU tests' inputs
for their comparison rule, the compiled kernels' metadata, and one run of tests/test_gpu_hat.py on the host-emulated library."""
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
import torch.nn.functional as F
from PIL import Image

import compact_reference as CR
import dat_reference as DR
import hat_reference as R
import rrdb_reference as RR
import scunet_reference as UR
import swin2sr_reference as S2
import swinir_reference as SR
from helpers import rel_l2, seeded, worst_slice_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases of tests/test_gpu_hat.py: self 4 + overlap 4 + mask + wide rows 2 + refusals | gate 4 + cab_add 3 + refusals
# | networks 4 + the other index layout + arena size + uint8 2 + handles | do_upscale + registry
GPU_FILE_CASES = (4 + 4 + 1 + 2 + 1) + (4 + 3 + 1) + (4 + 1 + 1 + 2 + 1) + (1 + 1)


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_hat_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_hat.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == GPU_FILE_CASES, out[-2000:]


# ---- the reference's parts, pinned to torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 8])
def test_reference_window_attention_equals_sdpa_on_unfolded_windows(shift):
    """float64 against F.scaled_dot_product_attention with the additive bias + mask, the windows taken by Tensor.unfold."""
    b, h, w, heads, d = 2, 48, 32, 3, 10
    qkv = seeded((b, h, w, 3 * heads * d), 11 + shift).double()
    table = seeded((961, heads), 12, 1.5).double()
    got = R.window_attention(qkv, table, heads, shift)
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    win = x.unfold(1, 16, 16).unfold(2, 16, 16)                                  # [b, nwy, nwx, 3C, 16, 16]
    nwy, nwx = win.shape[1], win.shape[2]
    q, k, v = win.reshape(b, nwy * nwx, 3, heads, d, 256).permute(2, 0, 1, 3, 5, 4)                   # [b, nW, heads, 256, d]
    add = table[R.sa_index().view(-1)].view(256, 256, heads).permute(2, 0, 1)[None, None]
    if shift:
        add = add + R.shift_mask(h, w).double()[None, :, None]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=add.expand(b, nwy * nwx, heads, 256, 256))
    o = o.view(b, nwy, nwx, heads, 16, 16, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(b, h, w, heads * d)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    assert rel_l2(got, o) < 1e-12


def test_reference_overlap_keys_equal_nn_unfold_and_the_attention_sdpa():
    """overlap_windows against nn.Unfold(24, stride=16, padding=4) of the k | v maps, rearranged as the architecture does; then the whole
    block's attention against scaled_dot_product_attention on those keys."""
    b, h, w, heads, d = 2, 32, 48, 3, 10
    c = heads * d
    qkv = seeded((b, h, w, 3 * c), 21).double()
    kv = qkv[..., c:].permute(0, 3, 1, 2)                                         # [b, 2c, h, w]
    unf = torch.nn.Unfold(kernel_size=(24, 24), stride=16, padding=4)(kv)         # [b, 2c * 576, nW]
    nw = unf.shape[-1]
    assert nw == (h // 16) * (w // 16)
    unf = unf.view(b, 2, c, 576, nw).permute(1, 0, 4, 3, 2).reshape(2, b * nw, 576, c)
    assert torch.equal(R.overlap_windows(qkv[..., c:2 * c]), unf[0]) and torch.equal(R.overlap_windows(qkv[..., 2 * c:]), unf[1])
    zeros = (unf[0].abs().sum(-1) == 0).view(b, nw, 576)
    assert int(zeros[0, 0].sum()) == 576 - 20 * 20                                # a corner window: 4 rows and 4 columns outside
    for layout in ("reference", "plain"):
        index = R.oca_index(layout)
        table = seeded((1521, heads), 22, 1.5).double()
        got = R.overlap_attention(qkv, table, heads, index=index)
        q = R.window_partition(qkv[..., :c]).view(-1, 256, heads, d).transpose(1, 2)
        k, v = (t.view(-1, 576, heads, d).transpose(1, 2) for t in unf)
        add = table[index.view(-1)].view(256, 576, heads).permute(2, 0, 1)[None]
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=add.expand(q.shape[0], heads, 256, 576))
        assert rel_l2(got, R.window_reverse(o.transpose(1, 2).reshape(-1, 256, c), b, h, w)) < 1e-12


def test_region_mask_equals_transformers_swin_mask_at_window_16():
    transformers = pytest.importorskip("transformers")
    from transformers.models.swin.modeling_swin import SwinLayer
    cfg = transformers.SwinConfig(image_size=64, patch_size=1, embed_dim=16, depths=[2], num_heads=[2], window_size=16)
    layer = SwinLayer(cfg, 16, (48, 32), 2, shift_size=8)
    want = layer.get_attn_mask(48, 32, torch.float32, torch.device("cpu"))
    assert torch.equal(R.shift_mask(48, 32), want)


def test_reference_channel_attention_equals_torch_modules():
    """cab.3 against AdaptiveAvgPool2d + Conv2d + ReLU + Conv2d + Sigmoid, and the branch against Conv2d + GELU + Conv2d."""
    nn = torch.nn
    sd = R.make_state_dict(60, (1,), 6, 3, 30, 2, 2)
    pre = "layers.0.residual_group.blocks.0.conv_block."
    att = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(60, 2, 1), nn.ReLU(), nn.Conv2d(2, 60, 1), nn.Sigmoid())
    att[1].load_state_dict({k: sd[pre + "cab.3.attention.1." + k] for k in ("weight", "bias")})
    att[3].load_state_dict({k: sd[pre + "cab.3.attention.3." + k] for k in ("weight", "bias")})
    body = nn.Sequential(nn.Conv2d(60, 20, 3, padding=1), nn.GELU(), nn.Conv2d(20, 60, 3, padding=1))
    body[0].load_state_dict({k: sd[pre + "cab.0." + k] for k in ("weight", "bias")})
    body[2].load_state_dict({k: sd[pre + "cab.2." + k] for k in ("weight", "bias")})
    n = seeded((2, 60, 16, 32), 31)
    with torch.no_grad():
        y = body(n)
        want = y * att(y)
    conv, gate = R.cab(sd, pre, n)
    assert gate.shape == (2, 60, 1, 1) and rel_l2(conv * gate, want) < 1e-6 and float(gate.std()) > 0.02


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_reference_tail_equals_torch_pixelshuffle_modules(scale):
    sd = R.make_state_dict(60, (1,), 6, 3, 30, 2, scale)
    nn = torch.nn
    mods = [nn.Conv2d(60, 64, 3, padding=1), nn.LeakyReLU(0.01)]
    names = ["conv_before_upsample.0", None]
    for k in ((0, 2) if scale == 4 else (0,)):
        mods += [nn.Conv2d(64, (9 if scale == 3 else 4) * 64, 3, padding=1), nn.PixelShuffle(3 if scale == 3 else 2)]
        names += [f"upsample.{k}", None]
    mods.append(nn.Conv2d(64, 3, 3, padding=1))
    names.append("conv_last")
    for m, n in zip(mods, names):
        if n:
            m.load_state_dict({"weight": sd[n + ".weight"], "bias": sd[n + ".bias"]})
    f = seeded((1, 60, 7, 9), 51)
    with torch.no_grad():
        want = nn.Sequential(*mods)(f)
    assert want.shape == (1, 3, 7 * scale, 9 * scale) and rel_l2(R.tail(sd, f, scale), want) < 1e-6


def test_reference_pads_by_reflection_and_crops():
    """17 x 33 is computed on the 32 x 48 reflect-padded image and cropped: the same as running the padded image and cropping."""
    sd = R.make_state_dict(48, (1,), 2, 24, 24, 2, 2)
    x = R.image(1, 17, 33, 3)
    padded = F.pad(x, (0, 15, 0, 15), mode="reflect")
    assert torch.equal(R.forward(sd, x), R.forward(sd, padded)[:, :, :34, :66])


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
def blob_by_hand(sd, cfg):
    """The documented order (include/sdmi.h at sdmi_hat_config), written out independently of the loader."""
    parts = []

    def wb(n):
        parts.extend([sd[n + ".weight"].flatten(), sd[n + ".bias"].flatten()])
    wb("conv_first")
    wb("patch_embed.norm")
    index = sd["relative_position_index_OCA"]
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            wb(b + "norm1")
            parts.append(sd[b + "attn.relative_position_bias_table"].flatten())
            for n in ("attn.qkv", "attn.proj", "conv_block.cab.0", "conv_block.cab.2", "conv_block.cab.3.attention.1", "conv_block.cab.3.attention.3",
                      "norm2", "mlp.fc1", "mlp.fc2"):
                wb(b + n)
        o = f"layers.{i}.residual_group.overlap_attn."
        wb(o + "norm1")
        wb(o + "qkv")
        table = sd[o + "relative_position_bias_table"]
        by_offset = torch.zeros((39, 39, table.shape[1]))
        for dy in range(-15, 24):                                # query (ya, xa), key (ya + dy, xa + dx): any pair with this offset
            for dx in range(-15, 24):
                ya, xa = max(0, -dy), max(0, -dx)
                by_offset[dy + 15, dx + 15] = table[int(index[ya * 16 + xa, (ya + dy) * 24 + xa + dx])]
        parts.append(by_offset.flatten())
        for n in ("proj", "norm2", "mlp.fc1", "mlp.fc2"):
            wb(o + n)
        wb(f"layers.{i}.conv")
    for n in ["norm", "conv_after_body", "conv_before_upsample.0", "upsample.0"] + (["upsample.2"] if cfg["scale"] == 4 else []) + ["conv_last"]:
        wb(n)
    return torch.cat(parts)


@pytest.mark.parametrize("kw", [dict(embed_dim=60, depths=(2, 1), heads=6, compress_ratio=3, squeeze_factor=30, mlp_ratio=2, scale=4),
                                dict(embed_dim=144, depths=(1,), heads=6, compress_ratio=24, squeeze_factor=24, mlp_ratio=2, scale=3,
                                     index_layout="plain")])
def test_loader_blob_is_the_documented_order(kw):
    up = sub("upscaler")
    sd = R.make_state_dict(**kw)
    for wrap in (sd, {"params_ema": sd}, {"params": sd}):
        blob, cfg = up.parse_hat_state_dict(wrap)
    c = kw["embed_dim"]
    assert cfg == dict(embed_dim=c, depths=kw["depths"], num_heads=kw["heads"], mlp_hidden=2 * c, cab_mid=c // kw["compress_ratio"],
                       cab_squeeze=c // kw["squeeze_factor"], conv_scale=0.01, scale=kw["scale"]) == R.config_of(sd)
    want = blob_by_hand(sd, cfg)
    assert blob.dtype == np.float32 and blob.shape == tuple(want.shape)
    assert torch.equal(torch.from_numpy(blob), want)
    assert up.parse_hat_state_dict(sd, conv_scale=0.5)[1]["conv_scale"] == 0.5
    no_masks = {k: v for k, v in sd.items() if not k.endswith("attn_mask") and k != "relative_position_index_SA"}
    assert np.array_equal(up.parse_hat_state_dict(no_masks)[0], blob)               # those buffers hold nothing the loader reads


def test_loader_reads_the_published_geometries():
    up = sub("upscaler")
    sd = R.make_state_dict(180, (1,) * 6, 6, 3, 30, 2, 4)
    assert up.parse_hat_state_dict(sd)[1] == dict(embed_dim=180, depths=(1,) * 6, num_heads=6, mlp_hidden=360, cab_mid=60, cab_squeeze=6,
                                                  conv_scale=0.01, scale=4)
    cfg = up.parse_hat_state_dict(R.make_state_dict(144, (1,), 6, 24, 24, 2, 2))[1]                   # HAT-S
    assert (cfg["cab_mid"], cfg["cab_squeeze"], cfg["scale"]) == (6, 6, 2)


def test_both_index_layouts_reduce_to_offset_tables_that_reproduce_table_of_index():
    """hat_oca_rows of either layout's buffer, and of no buffer at all (the formula): table[rows] read by offset IS table[index], entry
    for entry, negative rows counted from the end; the loader follows the buffer, not the formula."""
    up = sub("upscaler")
    dy, dx = R.oca_offsets()
    plain = ((dy + 15) * 39 + (dx + 15)).numpy()
    table = seeded((1521, 3), 61)
    for layout in ("reference", "plain"):
        index = R.oca_index(layout)
        rows = up.hat_oca_rows(index.numpy())
        assert rows.shape == (1521,) and rows.dtype == np.int64 and sorted(rows.tolist()) == list(range(1521))
        assert torch.equal(table[torch.from_numpy(rows)][torch.from_numpy(plain).view(-1)], table[index.view(-1)])
    assert int(R.oca_index("reference").min()) == -880 and int(R.oca_index("reference").max()) == 640
    assert np.array_equal(up.hat_oca_rows(None), up.hat_oca_rows(R.oca_index("reference").numpy()))
    assert not np.array_equal(up.hat_oca_rows(None), up.hat_oca_rows(R.oca_index("plain").numpy()))
    # the same function in two checkpoints: one blob
    a, b = (up.parse_hat_state_dict(R.make_state_dict(60, (1,), 6, 3, 30, 2, 2, index_layout=l))[0] for l in ("reference", "plain"))
    assert np.array_equal(a, b)
    # a plain-layout checkpoint without its buffer would be read by the formula: another blob — the buffer is what the loader follows
    sd = R.make_state_dict(60, (1,), 6, 3, 30, 2, 2, index_layout="plain")
    del sd["relative_position_index_OCA"]
    assert not np.array_equal(up.parse_hat_state_dict(sd)[0], a)
    assert np.array_equal(up.hat_sa_index(), R.sa_index().numpy()) and np.array_equal(up.hat_sa_index(), DR.relative_position_index(16, 16).numpy())


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_hat_state_dict
    base = R.make_state_dict(60, (2,), 6, 3, 30, 2, 2)
    b0, o0 = "layers.0.residual_group.blocks.0.", "layers.0.residual_group.overlap_attn."

    def variant(drop=(), **put):
        sd = {k: v for k, v in base.items() if not any(k.startswith(d) for d in drop)}
        sd.update(put)
        return sd
    z = torch.zeros
    with pytest.raises(ValueError, match="window_size 8"):
        parse(variant(**{b0 + "attn.relative_position_bias_table": z(225, 6)}))
    with pytest.raises(ValueError, match=r"overlap_ratio 0.25 \(a 1225-row"):
        parse(variant(**{o0 + "relative_position_bias_table": z(35 * 35, 6)}))
    with pytest.raises(ValueError, match=r"relative_position_index_OCA \(256, 400\)"):
        parse(variant(relative_position_index_OCA=z(256, 400, dtype=torch.long)))
    with pytest.raises(ValueError, match="head_dim = 240/6 = 40"):
        parse(R.make_state_dict(240, (1,), 6, 4, 30, 2, 2))
    with pytest.raises(ValueError, match="3conv"):
        parse(variant(drop=("layers.0.conv.",), **{"layers.0.conv.0.weight": z(15, 60, 3, 3)}))
    with pytest.raises(ValueError, match="identity"):
        parse(variant(drop=("layers.0.conv.",)))
    with pytest.raises(ValueError, match="pixelshuffledirect"):
        parse(variant(drop=("conv_before_upsample.", "conv_last."), **{"upsample.0.weight": z(12, 60, 3, 3)}))
    with pytest.raises(ValueError, match="without an upsampler"):
        parse(variant(drop=("conv_before_upsample.", "upsample.")))
    with pytest.raises(ValueError, match="num_feat = 32"):
        parse(variant(**{"conv_before_upsample.0.weight": z(32, 60, 3, 3)}))
    with pytest.raises(ValueError, match="takes 1 input channels"):
        parse(variant(**{"conv_first.weight": z(60, 1, 3, 3)}))
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(**{"upsample.0.weight": z(1024, 64, 3, 3)}))
    with pytest.raises(ValueError, match="absolute_pos_embed"):
        parse(variant(absolute_pos_embed=z(1, 256, 60)))
    with pytest.raises(ValueError, match="70 mid"):
        parse(variant(**{b0 + "conv_block.cab.0.weight": z(70, 60, 3, 3)}))
    bad = R.oca_index("reference").clone()
    bad[0, 0] += 1                                               # two pairs with the offset (0, 0) now name different rows
    with pytest.raises(ValueError, match="not a function of the key offset"):
        parse(variant(relative_position_index_OCA=bad))
    with pytest.raises(ValueError, match="outside the 1521-row table"):
        parse(variant(relative_position_index_OCA=R.oca_index("plain") + 1))
    with pytest.raises(ValueError, match="relative_position_index_SA is not the standard"):
        parse(variant(relative_position_index_SA=R.sa_index().t().contiguous()))
    for key in ("layers.0.residual_group.blocks.1.mlp.fc2.bias", o0 + "proj.weight", b0 + "conv_block.cab.3.attention.3.bias", "patch_embed.norm.bias",
                "layers.0.residual_group.blocks.1.attn.relative_position_bias_table", "upsample.0.bias", "conv_last.weight"):
        sd = variant()
        del sd[key]
        with pytest.raises(ValueError, match=re.escape(key.rsplit(".", 1)[0] if key.endswith(("weight", "bias")) else key)):
            parse(sd)
    with pytest.raises(ValueError, match="not a HAT checkpoint"):
        parse(SR.make_state_dict(60, (2,), 2, "1conv", 2))


# ---- the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_answers_hat_and_the_six_other_families_as_before():
    up = sub("upscaler")
    hat = R.make_state_dict(60, (2,), 6, 3, 30, 2, 3)
    assert up.SWINIR_MARK in hat                                 # what sent a HAT checkpoint to the SwinIR loader
    for sd in (hat, {"params_ema": hat}, {"params": hat}):
        assert up.upscaler_family(sd) == "hat"
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "hat" and parsed[-1] == 3 and parsed[1] == R.config_of(hat)
        assert np.array_equal(parsed[0], up.parse_hat_state_dict(hat)[0])
    others = {"dat": DR.make_state_dict(60, (2,), 6, (8, 32), 2, 3), "swin2sr": S2.make_state_dict(60, (2,), 6, "1conv", 3, "pixelshuffle"),
              "swinir": SR.make_state_dict(60, (2,), 2, "1conv", 2), "rrdb": RR.make_state_dict(1, 4), "compact": CR.make_state_dict(),
              "scunet": UR.make_state_dict()}
    for family, sd in others.items():
        assert up.HAT_MARK not in sd, family                     # no other family has the key
        assert up.upscaler_family(sd) == family and up.parse_upscaler_state_dict(sd)[0] == family
    with pytest.raises(ValueError, match="head_dim"):            # a HAT the engine refuses: that loader's message
        up.parse_upscaler_state_dict(R.make_state_dict(240, (1,), 6, 4, 30, 2, 2))


def test_make_upscaler_net_picks_hatnet(monkeypatch, tmp_path):
    up, shared = sub("upscaler"), sub("shared")
    made = []
    for cls, tag in ((up.SwinIRNet, "swinir"), (up.DATNet, "dat"), (up.HATNet, "hat")):
        monkeypatch.setattr(cls, "__init__", lambda self, sd, device=0, engine=None, _t=tag: made.append(_t))
    hat = R.make_state_dict(60, (2,), 6, 3, 30, 2, 2)
    assert type(up.make_upscaler_net({"params_ema": hat})) is up.HATNet
    assert type(up.make_upscaler_net(SR.make_state_dict(60, (2,), 2, "1conv", 2))) is up.SwinIRNet
    assert made == ["hat", "swinir"] and issubclass(up.HATNet, up._EngineNet) and up.HATNet._abi == "sdmi_hat"
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save({"params_ema": R.make_state_dict(60, (1,), 6, 3, 30, 2, 3)}, str(tmp_path / "HAT_x3.pth"))
    added = up.register_esrgan([str(tmp_path / "HAT_x3.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "HAT_x3"] and added[0].scale == 3


# ---- the webui hook ---------------------------------------------------------------------------------------------------------------
def test_install_hat_hook_runs_a_hat_file_on_the_engine(tmp_path, monkeypatch):
    """An UpscalerHAT entry runs on the engine; a file the loader refuses (3conv) and a URL stay on the stock path; a second install
    changes nothing."""
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, refused = str(tmp_path / "HAT_x2.pth"), str(tmp_path / "HAT_3conv_x2.pth")
    hat = R.make_state_dict(60, (1,), 6, 3, 30, 2, 2)
    torch.save({"params_ema": hat}, good)
    torch.save({"params_ema": dict({k: v for k, v in hat.items() if not k.startswith("layers.0.conv.")},
                                   **{"layers.0.conv.0.weight": torch.zeros(15, 60, 3, 3)})}, refused)

    class UpscalerHAT:                                          # the shape of modules/hat_model.py's scaler object
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, path):
            self.stock_calls.append(path)
            return img
    scaler, other = UpscalerHAT(), types.SimpleNamespace(do_upscale=lambda img, path: img)
    data = [types.SimpleNamespace(name="HAT x2", data_path=good, local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="HAT 3conv", data_path=refused, local_data_path=refused, scaler=scaler),
            types.SimpleNamespace(name="HAT x4", data_path="https://example.invalid/HAT_x4.pth", local_data_path=None, scaler=scaler),
            types.SimpleNamespace(name="Other", data_path=good, local_data_path=good, scaler=other)]
    scaler.scalers = data[:3]
    engine_calls, families = [], []

    def load_model(self, path):
        family, parsed = up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(path))
        families.append(family)
        return parsed
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", load_model)
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    shared = types.SimpleNamespace(sd_upscalers=data)
    assert bridge.install_hat_hook(shared) == ["HAT x2", "HAT 3conv", "HAT x4"]
    hooked = scaler.do_upscale
    assert bridge.install_hat_hook(shared) == ["HAT x2", "HAT 3conv", "HAT x4"] and scaler.do_upscale is hooked
    img = Image.new("RGB", (16, 16))
    scaler.do_upscale(img, good)
    assert engine_calls == [good] and scaler.stock_calls == [] and families == ["hat"]
    scaler.do_upscale(img, refused)
    assert engine_calls == [good] and scaler.stock_calls == [refused]
    scaler.do_upscale(img, "HAT x4")
    assert engine_calls == [good] and scaler.stock_calls == [refused, "HAT x4"]
    assert "UpscalerHAT" in bridge.install_hat_hook.__doc__ and "stock path" in bridge.install_hat_hook.__doc__


# ---- the GPU tests' inputs are fit for their rule -----------------------------------------------------------------------------------
def test_gpu_test_inputs_are_fit_for_the_comparison_rule():
    """For every case of tests/test_gpu_hat.py, on the reference alone: the twin's rel_l2 lies above 1e-4 and its worst slice within
    2.5 x of it; removing the bias or the mask, masking the padded keys and transposing the offset table each move the result by more
    than 10 x the yardstick; the independent graphs and the reference's roll / partition / unfold forms are the same functions; the
    crafted case tells -100 from -inf; the nets' outputs are 0 or 255 on fewer than 5 % of the bytes."""
    import test_gpu_hat as G
    to_u8 = sub("upscaler").model_output_to_u8

    def fit(twin, ref, channel_dim, row_dims, ctx):
        yard = rel_l2(twin.double(), ref.double())
        assert yard > 1e-4, (ctx, yard)
        for keep in ((channel_dim,), row_dims):
            assert worst_slice_rel_l2(twin.double(), ref.double(), keep)[0] <= 2.5 * yard, (ctx, keep)
        return yard
    assert [c[1:] for c in G.SELF_CASES] == [(16, 16, 6, 30, 0), (32, 32, 6, 30, 8), (48, 32, 2, 32, 8), (32, 48, 5, 24, 0)]
    for b, h, w, heads, d, shift in G.SELF_CASES:
        case = G.win_case(0, b, h, w, heads, d)
        ref = G.win_graph(case, shift)
        yard = fit(G.win_graph(case, shift, G.r16d), ref, 3, (0, 1), ("self", b, h, w, heads, d, shift))
        assert rel_l2(G.win_graph(case, shift, bias=False), ref) > 10 * yard
        assert rel_l2(G.win_graph(case, shift, transpose_table=True), ref) > 10 * yard
        if shift:
            assert rel_l2(G.win_graph(case, shift, mask=False), ref) > 10 * yard
            assert rel_l2(G.win_graph(case, shift, mask_value=-math.inf), ref) < 0.01 * yard         # random data cannot tell the two masks apart
        qkv = torch.cat([case[n].flatten(3) for n in "qkv"], dim=-1).double()
        assert rel_l2(R.window_attention(qkv, case["table"].double(), heads, shift), ref) < 1e-12
    regions = G.region(torch.arange(32), 32)
    assert sorted(set((3 * regions[:, None] + regions[None, :]).flatten().tolist())) == list(range(9))    # the 32 x 32 case has all nine
    assert [c[1:] for c in G.OVERLAP_CASES] == [(16, 16, 6, 30), (32, 48, 6, 30), (48, 48, 2, 32), (32, 32, 5, 24)]
    plain = R.oca_index("plain")
    for b, h, w, heads, d in G.OVERLAP_CASES:
        case = G.win_case(1, b, h, w, heads, d)
        ref = G.win_graph(case)
        yard = fit(G.win_graph(case, 0, G.r16d), ref, 3, (0, 1), ("overlap", b, h, w, heads, d))
        assert rel_l2(G.win_graph(case, bias=False), ref) > 10 * yard
        assert rel_l2(G.win_graph(case, transpose_table=True), ref) > 10 * yard
        assert rel_l2(G.win_graph(case, mask_padded_keys=True), ref) > 10 * yard
        qkv = torch.cat([case[n].flatten(3) for n in "qkv"], dim=-1).double()
        assert rel_l2(R.overlap_attention(qkv, case["table"].double(), heads, index=plain), ref) < 1e-12
        assert rel_l2(R.overlap_attention(qkv, case["table"].double(), heads, index=plain, mask_padded_keys=True),
                      G.win_graph(case, mask_padded_keys=True)) < 1e-12
    ones = R.overlap_windows(torch.ones((1, 16, 16, 1)))[0, :, 0]
    assert int((ones == 0).sum()) == 320                         # 16 x 16: 320 of the 576 keys are padding
    assert bool((R.overlap_windows(torch.ones((1, 48, 48, 1)))[4, :, 0] == 1).all())                 # 48 x 48: the centre window has none
    crafted = G.crafted_mask_case()
    ref = G.win_graph(crafted, 8)
    yard = fit(G.win_graph(crafted, 8, G.r16d), ref, 3, (0, 1), "crafted")
    assert rel_l2(G.win_graph(crafted, 8, mask_value=-math.inf), ref) > 10 * yard
    assert {(n, c, cs) for n, c, cs in G.CAB_CASES} >= {(256, 64, 2), (48 * 32, 192, 6), (300, 192, 6)}
    for n, c, cs in G.CAB_CASES:
        case = G.cab_case(n, c, cs)
        gate = G.gate_ref(case)
        assert float(gate.std()) > 0.05 and bool(torch.isfinite(gate).all())
        ref = case["t"].double() + 0.5 * gate[:, None] * case["conv"].double()
        yard = fit(G.r16d(ref), ref, 2, (0, 1), ("cab_add", n, c))
        assert rel_l2(case["t"].double() + 0.5 * 0.5 * case["conv"].double(), ref) > 10 * yard      # a constant gate is not the gate
    assert len(G.NET_CASES) == 4 and {kw["scale"] for kw, _ in G.NET_CASES.values()} == {2, 3, 4}
    for name, (kw, (b, h, w)) in G.NET_CASES.items():
        x, ref, twin = G.reference_for(name)
        assert x.shape == (b, 3, h, w) and torch.equal(torch.round(x * 255) / 255, x)
        assert ref.shape == (b, 3, h * kw["scale"], w * kw["scale"])
        u8 = to_u8(ref.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, name
        fit(twin, ref, 1, (0, 2), name)


# ---- the kernels as compiled --------------------------------------------------------------------------------------------------------
def test_hat_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of csrc/hat.hip, from the metadata counts: five kernels, none with scratch or spills; the file states
    its launch configuration with the LDS bytes the two window attention forms take."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("hat")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block)}
    assert len(meta) == 5, sorted(meta)
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    attn = {n: m for n, m in meta.items() if "hat_window_attn" in n}
    assert len(attn) == 2 and all(m["vgpr_count"] <= 512 for m in attn.values()), attn
    assert sorted(m["group_segment_fixed_size"] for m in attn.values()) == [41232, 89284]
    src = open(os.path.join(ROOT, "stable-diffusion-webui_amd", "csrc", "hat.hip")).read()
    assert "Launch configuration" in src
    for m in attn.values():                                     # the LDS bytes the comment states are the code object's
        assert str(m["group_segment_fixed_size"]) in src, m
        assert m["group_segment_fixed_size"] <= 160 * 1024
