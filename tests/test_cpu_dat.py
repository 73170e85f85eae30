"""CPU tier of the DAT path: the parts of the reference restatement pinned to torch (and the region mask to transformers' Swin), the
checkpoint loader and dispatcher, the loader's host precompute (bias tables, BatchNorm folds), the webui hook, the fitness of the GPU
tests' inputs for their comparison rule, the compiled kernels' metadata, and one run of tests/test_gpu_dat.py on the host-emulated
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
import torch.nn.functional as F
from PIL import Image

import compact_reference as CR
import dat_reference as R
import rrdb_reference as RR
import scunet_reference as UR
import swin2sr_reference as S2
import swinir_reference as SR
from helpers import rel_l2, seeded, worst_slice_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases of tests/test_gpu_dat.py: window attention 5 + mask + wide rows + refusals | channel attention 5 + refusals | dwconv 6 + refusals
# | pool gate 2 + aim_combine 2 | networks 5 + arena size + uint8 2 + handles | do_upscale + registry
GPU_FILE_CASES = (5 + 1 + 1 + 1) + (5 + 1) + (6 + 1) + (2 + 2) + (5 + 1 + 2 + 1) + (1 + 1)


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_dat_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_dat.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == GPU_FILE_CASES, out[-2000:]


# ---- the reference's parts, pinned to torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,ws,shifted", [(8, 16, False), (8, 32, True), (32, 8, True), (16, 8, True)])
def test_reference_window_attention_equals_sdpa_on_unfolded_windows(hs, ws, shifted):
    """One branch in float64 against F.scaled_dot_product_attention with the additive bias + mask, the windows taken by Tensor.unfold."""
    b, hp, wp, heads, d = 2, 64, 64, 3, 10
    qkv = seeded((3, b, hp, wp, heads * d), 11 + hs + ws).double()
    table = seeded(((2 * hs - 1) * (2 * ws - 1), heads), 12 + hs, 1.5).double()
    got = R.branch_attention(qkv, table, heads, hs, ws, shifted)
    x = torch.roll(qkv, (-(hs // 2), -(ws // 2)), (2, 3)) if shifted else qkv
    win = x.unfold(2, hs, hs).unfold(3, ws, ws)                                  # [3, b, nwy, nwx, C, hs, ws]
    nwy, nwx = win.shape[2], win.shape[3]
    q, k, v = win.reshape(3, b, nwy * nwx, heads, d, hs * ws).transpose(-1, -2)   # [b, nW, heads, N, d]
    add = table[R.relative_position_index(hs, ws).view(-1)].view(hs * ws, hs * ws, heads).permute(2, 0, 1)[None, None]
    if shifted:
        add = add + R.shift_mask(hp, wp, hs, ws).double()[None, :, None]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=add.expand(b, nwy * nwx, heads, hs * ws, hs * ws))
    o = o.view(b, nwy, nwx, heads, hs, ws, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(b, hp, wp, heads * d)
    if shifted:
        o = torch.roll(o, (hs // 2, ws // 2), (1, 2))
    assert rel_l2(got, o) < 1e-12


def test_reference_spatial_attention_pads_after_the_linear_and_crops():
    """The two branches on the halves of the channels; the padded tokens are zero rows that take part as keys."""
    b, h, w, heads, d, split = 1, 20, 37, 4, 6, (8, 16)
    c = heads * d
    qkv = seeded((b, h, w, 3 * c), 21).double()
    tables = tuple(seeded((15 * 31, heads // 2), 22 + i, 1.5).double() for i in range(2))
    got = R.spatial_attention(qkv, tables, heads, split, True)
    assert got.shape == (b, h, w, c)
    pad = F.pad(qkv, (0, 0, 0, 48 - w, 0, 32 - h)).view(b, 32, 48, 3, c).permute(3, 0, 1, 2, 4)
    want = torch.cat([R.branch_attention(pad[..., :c // 2], tables[0], 2, 8, 16, True), R.branch_attention(pad[..., c // 2:], tables[1], 2, 16, 8, True)], -1)
    assert torch.equal(got, want[:, :h, :w])


def test_reference_channel_attention_equals_the_einsum_form():
    b, n, heads, d = 2, 77, 3, 10
    qkv = seeded((b, n, 3 * heads * d), 31).double()
    temp = torch.tensor([0.5, 2.0, 9.0], dtype=torch.float64)
    q, k, v = qkv.view(b, n, 3, heads, d).unbind(2)
    qn, kn = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12), k / k.norm(dim=1, keepdim=True).clamp_min(1e-12)
    a = torch.softmax(torch.einsum("bnhi,bnhj->bhij", qn, kn) * temp.view(1, -1, 1, 1), dim=-1)
    want = torch.einsum("bhij,bnhj->bnhi", a, v).reshape(b, n, heads * d)
    assert rel_l2(R.channel_attention(qkv, temp, heads), want) < 1e-12


def test_batchnorm_and_its_fold_equal_torch_batchnorm2d_eval():
    up = sub("upscaler")
    sd = R.make_state_dict(60, (2,), 6, (8, 16), 2, 2)
    pre = "layers.0.blocks.0."
    x = seeded((2, 60, 9, 7), 41)
    for conv, bn, groups in ((pre + "attn.dwconv.0", pre + "attn.dwconv.1", 60), (pre + "attn.spatial_interaction.0", pre + "attn.spatial_interaction.1", 1)):
        w, bias = sd[conv + ".weight"], sd[conv + ".bias"]
        m = torch.nn.BatchNorm2d(w.shape[0]).eval()
        m.load_state_dict({k: sd[bn + "." + k] for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")})
        pad = w.shape[-1] // 2
        with torch.no_grad():
            want = m(F.conv2d(x, w, bias, padding=pad, groups=groups))
        assert rel_l2(R.batchnorm(sd, bn, F.conv2d(x, w, bias, padding=pad, groups=groups)), want) < 1e-6
        fw, fb = up.dat_bn_fold(w.numpy(), bias.numpy(), *(sd[bn + "." + k].numpy() for k in ("weight", "bias", "running_mean", "running_var")))
        assert fw.dtype == np.float32 and fb.dtype == np.float32
        assert rel_l2(F.conv2d(x, torch.from_numpy(fw), torch.from_numpy(fb), padding=pad, groups=groups), want) < 1e-6


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_reference_tail_equals_torch_pixelshuffle_modules(scale):
    sd = R.make_state_dict(60, (1,), 6, (8, 16), 2, scale)
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


def test_roll_and_mask_equal_transformers_swin_region_mask_in_the_square_case():
    """shift_mask with a square window is Swin's region mask: transformers' SwinLayer.get_attn_mask at window 8, shift 4."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.swin.modeling_swin import SwinLayer
    cfg = transformers.SwinConfig(image_size=32, patch_size=1, embed_dim=16, depths=[2], num_heads=[2], window_size=8)
    layer = SwinLayer(cfg, 16, (32, 24), 2, shift_size=4)
    want = layer.get_attn_mask(32, 24, torch.float32, torch.device("cpu"))
    assert torch.equal(R.shift_mask(32, 24, 8, 8), want)
    ids = R.region_ids(32, 48, 8, 32)                            # the rectangular case by hand: rows 0..23 | 24..27 | 28..31, columns 0..15 | 16..31 | 32..47
    assert ids[23, 15] == 0 and ids[24, 15] == 3 and ids[28, 15] == 6 and ids[0, 16] == 1 and ids[0, 32] == 2 and ids[31, 47] == 8
    assert [R.is_shifted(i, j) for i in (0, 1) for j in range(8)] == [False, False, True, False, False, False, True, False,
                                                                      True, False, False, False, True, False, False, False]


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
def by_hand_table(sd, pre, hs, ws, dy, dx):
    """One row of the bias table in float64, scalar by scalar."""
    g = {k[len(pre):]: v.double() for k, v in sd.items() if k.startswith(pre)}
    x = g["pos_proj.weight"] @ torch.tensor([float(dy), float(dx)], dtype=torch.float64) + g["pos_proj.bias"]
    for k in ("pos1", "pos2", "pos3"):
        mu = x.mean()
        x = (x - mu) / torch.sqrt(((x - mu) ** 2).mean() + 1e-5) * g[k + ".0.weight"] + g[k + ".0.bias"]
        x = g[k + ".2.weight"] @ torch.clamp(x, min=0) + g[k + ".2.bias"]
    return x


def test_bias_table_against_float64_and_three_offsets_by_hand():
    up = sub("upscaler")
    sd = R.make_state_dict(180, (1,), 6, (8, 32), 4, 2)          # pos_dim 5
    for k, (hs, ws) in enumerate(((8, 32), (32, 8))):
        pre = f"layers.0.blocks.0.attn.attns.{k}.pos."
        pos = {n[len(pre):]: v.numpy() for n, v in sd.items() if n.startswith(pre)}
        table = up.dat_position_bias(pos, hs, ws)
        assert table.shape == ((2 * hs - 1) * (2 * ws - 1), 3) and table.dtype == np.float32
        want = R.position_bias({n: v.double() for n, v in sd.items()}, pre, hs, ws)
        assert rel_l2(table, want) < 1e-5 and float(want.std()) > 0.1
        for dy, dx in ((1 - hs, 1 - ws), (0, 0), (hs - 1, 3)):
            row = (dy + hs - 1) * (2 * ws - 1) + dx + ws - 1
            assert float((torch.from_numpy(table[row]).double() - by_hand_table(sd, pre, hs, ws, dy, dx)).abs().max()) < 1e-4


def blob_by_hand(sd, cfg):
    """The documented order (include/sdmi.h at sdmi_dat_config), written out independently of the loader; folds and tables in float64."""
    c, heads, (s0, s1), hidden = cfg["embed_dim"], cfg["num_heads"], cfg["split"], cfg["ffn_hidden"]
    d = {k: v.double() for k, v in sd.items()}
    parts = []

    def wb(n):
        parts.extend([d[n + ".weight"].flatten(), d[n + ".bias"].flatten()])

    def folded(conv, bn):
        s = d[bn + ".weight"] / torch.sqrt(d[bn + ".running_var"] + 1e-5)
        parts.extend([(d[conv + ".weight"] * s.view(-1, 1, 1, 1)).flatten(), (d[conv + ".bias"] - d[bn + ".running_mean"]) * s + d[bn + ".bias"]])
    wb("conv_first")
    wb("before_RG.1")
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            b = f"layers.{i}.blocks.{j}."
            wb(b + "norm1")
            wb(b + "attn.qkv")
            if j % 2 == 0:
                parts.append(R.position_bias(d, b + "attn.attns.0.pos.", s0, s1).flatten())
                parts.append(R.position_bias(d, b + "attn.attns.1.pos.", s1, s0).flatten())
            else:
                parts.append(d[b + "attn.temperature"].flatten())
            folded(b + "attn.dwconv.0", b + "attn.dwconv.1")
            folded(b + "attn.channel_interaction.1", b + "attn.channel_interaction.2")
            wb(b + "attn.channel_interaction.4")
            folded(b + "attn.spatial_interaction.0", b + "attn.spatial_interaction.1")
            wb(b + "attn.spatial_interaction.3")
            for n in ("attn.proj", "norm2", "ffn.fc1", "ffn.sg.norm", "ffn.sg.conv", "ffn.fc2"):
                wb(b + n)
        wb(f"layers.{i}.conv")
    for n in ["norm", "conv_after_body", "conv_before_upsample.0", "upsample.0"] + (["upsample.2"] if cfg["scale"] == 4 else []) + ["conv_last"]:
        wb(n)
    return torch.cat(parts)


@pytest.mark.parametrize("kw", [dict(embed_dim=60, depths=(4, 2), heads=6, split=(8, 16), expansion=2, scale=4),
                                dict(embed_dim=180, depths=(2, 1), heads=6, split=(8, 32), expansion=4, scale=3)])
def test_loader_blob_is_the_documented_order(kw):
    up = sub("upscaler")
    sd = R.make_state_dict(**kw)
    for wrap in (sd, {"params_ema": sd}, {"params": sd}):
        blob, cfg = up.parse_dat_state_dict(wrap)
    assert cfg == dict(embed_dim=kw["embed_dim"], depths=kw["depths"], num_heads=kw["heads"], split=kw["split"],
                       ffn_hidden=kw["expansion"] * kw["embed_dim"], scale=kw["scale"]) == R.config_of(sd)
    want = blob_by_hand(sd, cfg)
    assert blob.dtype == np.float32 and blob.shape == tuple(want.shape)
    assert float((torch.from_numpy(blob).double() - want).abs().max()) < 1e-5
    raw = torch.from_numpy(blob)
    c = kw["embed_dim"]
    assert torch.equal(raw[:c * 27], sd["conv_first.weight"].flatten()) and torch.equal(raw[-3:], sd["conv_last.bias"])
    no_buffers = {k: v for k, v in sd.items() if not k.endswith(("relative_position_index", "attn_mask_0", "attn_mask_1"))}
    assert np.array_equal(up.parse_dat_state_dict(no_buffers)[0], blob)              # the buffers hold nothing the loader reads
    no_rpe = {k: v for k, v in sd.items() if not k.endswith("rpe_biases")}
    assert np.array_equal(up.parse_dat_state_dict(no_rpe)[0], blob)                  # the split from relative_position_index


def test_loader_reads_the_webui_geometry():
    up = sub("upscaler")
    sd = R.make_state_dict(180, (2,) * 6, 6, (8, 32), 4, 4)                         # "DAT x4" with two blocks per group
    blob, cfg = up.parse_dat_state_dict(sd)
    assert cfg == dict(embed_dim=180, depths=(2,) * 6, num_heads=6, split=(8, 32), ffn_hidden=720, scale=4)
    assert up.parse_dat_state_dict(R.make_state_dict(180, (1,), 6, (8, 16), 2, 2))[1]["ffn_hidden"] == 360      # DAT-S


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_dat_state_dict
    base = R.make_state_dict(60, (2,), 6, (8, 16), 2, 2)

    def variant(drop=(), **put):
        sd = {k: v for k, v in base.items() if not any(k.startswith(d) for d in drop)}
        sd.update(put)
        return sd
    z = torch.zeros
    with pytest.raises(ValueError, match="pixelshuffledirect"):
        parse(variant(drop=("conv_before_upsample.", "conv_last."), **{"upsample.0.weight": z(12, 60, 3, 3)}))
    with pytest.raises(ValueError, match="3conv"):
        parse(variant(drop=("layers.0.conv.",), **{"layers.0.conv.0.weight": z(15, 60, 3, 3)}))
    with pytest.raises(ValueError, match="head_dim = 240/6 = 40"):
        parse(R.make_state_dict(240, (1,), 6, (8, 16), 2, 2))
    with pytest.raises(ValueError, match="num_heads = 3 is odd"):
        parse(variant(**{"layers.0.blocks.1.attn.temperature": z(3, 1, 1)}))
    with pytest.raises(ValueError, match=r"split_size with 961 rows.*\(8, 16\) and \(8, 32\)"):
        parse(variant(**{"layers.0.blocks.0.attn.attns.0.rpe_biases": z(31 * 31, 2)}))
    with pytest.raises(ValueError, match="split_size with 64 tokens"):
        parse(variant(drop=("layers.0.blocks.0.attn.attns.0.rpe_biases",), **{"layers.0.blocks.0.attn.attns.0.relative_position_index": z(64, 64)}))
    with pytest.raises(ValueError, match="takes 1 input channels"):
        parse(variant(**{"conv_first.weight": z(60, 1, 3, 3)}))
    with pytest.raises(ValueError, match="num_feat = 32"):
        parse(variant(**{"conv_before_upsample.0.weight": z(32, 60, 3, 3)}))
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(**{"upsample.0.weight": z(1024, 64, 3, 3)}))                                  # a single x4 step
    with pytest.raises(ValueError, match="scales 2, 3 and 4"):
        parse(variant(**{"upsample.2.weight": z(256, 64, 3, 3), "upsample.2.bias": z(256), "upsample.4.weight": z(256, 64, 3, 3)}))     # x8
    for key in ("layers.0.blocks.1.ffn.fc2.bias", "layers.0.blocks.0.attn.attns.1.pos.pos2.2.weight", "layers.0.blocks.0.attn.dwconv.1.running_var",
                "layers.0.blocks.1.attn.temperature", "before_RG.1.bias", "upsample.0.weight"):
        sd = variant()
        del sd[key]
        if key.endswith("temperature"):                         # the head count then comes from the position MLP
            pass
        with pytest.raises(ValueError, match="lacks " + re.escape(key)):
            parse(sd)
    sd = variant(drop=("layers.0.blocks.0.attn.attns.0.rpe_biases", "layers.0.blocks.0.attn.attns.0.relative_position_index"))
    with pytest.raises(ValueError, match="lacks layers.0.blocks.0.attn.attns.0.rpe_biases"):
        parse(sd)
    with pytest.raises(ValueError, match="not a DAT checkpoint"):
        parse(S2.make_state_dict(60, (2,), 6, "1conv", 2, "pixelshuffle"))


# ---- the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_answers_for_all_six_families():
    up = sub("upscaler")
    dat = R.make_state_dict(60, (2,), 6, (8, 32), 2, 3)
    for sd in (dat, {"params_ema": dat}, {"params": dat}):
        assert up.upscaler_family(sd) == "dat"
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "dat" and parsed[-1] == 3 and parsed[1] == R.config_of(dat)
        assert np.array_equal(parsed[0], up.parse_dat_state_dict(dat)[0])
    others = {"swin2sr": S2.make_state_dict(60, (2,), 6, "1conv", 3, "pixelshuffle"), "swinir": SR.make_state_dict(60, (2,), 2, "1conv", 2),
              "rrdb": RR.make_state_dict(1, 4), "compact": CR.make_state_dict(), "scunet": UR.make_state_dict()}
    for family, sd in others.items():
        assert not any(k in sd for k in up.DAT_MARKS), family       # no existing family has either key
        assert up.upscaler_family(sd) == family and up.parse_upscaler_state_dict(sd)[0] == family
    with pytest.raises(ValueError, match="head_dim"):            # a DAT the engine refuses: that loader's message
        up.parse_upscaler_state_dict(R.make_state_dict(240, (1,), 6, (8, 16), 2, 2))


def test_make_upscaler_net_picks_datnet(monkeypatch, tmp_path):
    up, shared = sub("upscaler"), sub("shared")
    made = []
    for cls, tag in ((up.SwinIRNet, "swinir"), (up.Swin2SRNet, "swin2sr"), (up.DATNet, "dat")):
        monkeypatch.setattr(cls, "__init__", lambda self, sd, device=0, engine=None, _t=tag: made.append(_t))
    dat = R.make_state_dict(60, (2,), 6, (8, 16), 2, 2)
    assert type(up.make_upscaler_net({"params": dat})) is up.DATNet
    assert type(up.make_upscaler_net(SR.make_state_dict(60, (2,), 2, "1conv", 2))) is up.SwinIRNet
    assert made == ["dat", "swinir"] and issubclass(up.DATNet, up._EngineNet) and up.DATNet._abi == "sdmi_dat"
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save({"params": R.make_state_dict(60, (2,), 6, (8, 32), 2, 3)}, str(tmp_path / "DAT_x3.pth"))
    added = up.register_esrgan([str(tmp_path / "DAT_x3.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "DAT_x3"] and added[0].scale == 3


# ---- the webui hook ---------------------------------------------------------------------------------------------------------------
def test_install_dat_hook_runs_a_dat_file_on_the_engine(tmp_path, monkeypatch):
    """An UpscalerDAT entry runs on the engine; a DAT-light file (pixelshuffledirect) and a URL stay on the stock path; a second install
    changes nothing."""
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, light = str(tmp_path / "DAT_x2.pth"), str(tmp_path / "DAT_light_x2.pth")
    dat = R.make_state_dict(60, (2,), 6, (8, 16), 2, 2)
    torch.save({"params": dat}, good)
    torch.save({"params": {k: v for k, v in dat.items() if not k.startswith("conv_before_upsample.")}}, light)

    class UpscalerDAT:                                          # the shape of modules/dat_model.py's scaler object
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, path):
            self.stock_calls.append(path)
            return img
    scaler, other = UpscalerDAT(), types.SimpleNamespace(do_upscale=lambda img, path: img)
    data = [types.SimpleNamespace(name="DAT x2", data_path=good, local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="DAT light", data_path=light, local_data_path=light, scaler=scaler),
            types.SimpleNamespace(name="DAT x3", data_path="https://example.invalid/DAT_x3.pth", local_data_path=None, scaler=scaler),
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
    assert bridge.install_dat_hook(shared) == ["DAT x2", "DAT light", "DAT x3"]
    hooked = scaler.do_upscale
    assert bridge.install_dat_hook(shared) == ["DAT x2", "DAT light", "DAT x3"] and scaler.do_upscale is hooked
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, good)
    assert engine_calls == [good] and scaler.stock_calls == [] and families == ["dat"]
    scaler.do_upscale(img, light)
    assert engine_calls == [good] and scaler.stock_calls == [light]
    scaler.do_upscale(img, "DAT x3")
    assert engine_calls == [good] and scaler.stock_calls == [light, "DAT x3"]


# ---- the GPU tests' inputs are fit for their rule -----------------------------------------------------------------------------------
def test_gpu_test_inputs_are_fit_for_the_comparison_rule():
    """For every case of tests/test_gpu_dat.py, on the reference alone: the twin's rel_l2 lies above 1e-4 and its worst slice within
    2.5 x of it; the with / without-bias, with / without-mask and padded-key distances exceed 10 x the yardstick; the crafted mask case
    tells -100 from -inf; the nets' outputs stay inside [0, 1] on at least 95 % of the bytes."""
    import test_gpu_dat as G
    to_u8 = sub("upscaler").model_output_to_u8

    def fit(twin, ref, channel_dim, row_dims, ctx):
        yard = rel_l2(twin.double(), ref.double())
        assert yard > 1e-4, (ctx, yard)
        for keep in ((channel_dim,), row_dims):
            assert worst_slice_rel_l2(twin.double(), ref.double(), keep)[0] <= 2.5 * yard, (ctx, keep)
        return yard
    assert len(G.WIN_CASES) == 5
    padded = 0
    for b, h, w, heads, d, split, shifted in G.WIN_CASES:
        case = G.win_case(b, h, w, heads, d, split)
        ref = G.win_graph(case, shifted)
        yard = fit(G.win_graph(case, shifted, G.r16d), ref, 3, (0, 1), (b, h, w, heads, d, split, shifted))
        assert rel_l2(G.win_graph(case, shifted, bias=False), ref) > 10 * yard
        if shifted:
            assert rel_l2(G.win_graph(case, shifted, mask=False), ref) > 10 * yard
            assert rel_l2(G.win_graph(case, shifted, mask_value=-math.inf), ref) < 0.01 * yard       # random data cannot tell the two masks apart
        if h % split[1] or w % split[1]:
            padded += 1
            assert rel_l2(G.win_graph(case, shifted, mask_padded_keys=True), ref) > 10 * yard
        # the independent graph and the reference's roll / partition form are the same function
        qkv = torch.cat([case[n].flatten(3) for n in "qkv"], dim=-1).double()
        assert rel_l2(R.spatial_attention(qkv, tuple(t.double() for t in case["tables"]), heads, split, shifted), ref) < 1e-12
    assert padded >= 3
    crafted = G.crafted_mask_case()
    ref = G.win_graph(crafted, True)
    yard = fit(G.win_graph(crafted, True, G.r16d), ref, 3, (0, 1), "crafted")
    assert rel_l2(G.win_graph(crafted, True, mask_value=-math.inf), ref) > 10 * yard
    assert {n for _, n, _, _, _ in G.CH_CASES} == {1, 64, 9 * 13, 40 * 72} and any(z for *_, z in G.CH_CASES)
    for b, n, heads, d, zero in G.CH_CASES:
        q, k, temp = G.channel_case(b, n, heads, d, zero)
        ref = G.channel_graph(q, k, temp)
        fit(G.r16d(ref), ref, 1, (0, 2), ("channel", b, n, heads, d))
        assert float(temp.max()) <= 10 and bool(torch.isfinite(ref).all())
    assert max(float(G.channel_case(*c)[2].max()) for c in G.CH_CASES) > 8
    assert len(G.NET_CASES) == 5 and {kw["scale"] for kw, _ in G.NET_CASES.values()} == {2, 3, 4}
    assert {kw["split"] for kw, _ in G.NET_CASES.values()} == {(8, 16), (8, 32)}
    for name, (kw, (b, h, w)) in G.NET_CASES.items():
        x, ref, twin = G.reference_for(name)
        assert x.shape == (b, 3, h, w) and torch.equal(torch.round(x * 255) / 255, x)
        assert ref.shape == (b, 3, h * kw["scale"], w * kw["scale"])
        u8 = to_u8(ref.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, name
        fit(twin, ref, 1, (0, 2), name)


# ---- the kernels as compiled --------------------------------------------------------------------------------------------------------
def test_dat_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of csrc/dat.hip, from the metadata counts: eight kernels, none with scratch or spills, both window
    attention instantiations within 256 VGPRs; the file states its launch configuration with the LDS bytes it takes."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("dat")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block)}
    assert len(meta) == 8, sorted(meta)
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    attn = {n: m for n, m in meta.items() if "dat_window_attn" in n}
    assert len(attn) == 2 and all(m["vgpr_count"] <= 256 for m in attn.values()), attn
    src = open(os.path.join(ROOT, "stable-diffusion-webui_amd", "csrc", "dat.hip")).read()
    assert "Launch configuration" in src
    for m in attn.values():                                     # the LDS bytes the comment states are the code object's
        assert str(m["group_segment_fixed_size"]) in src, m
