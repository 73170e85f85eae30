"""CPU tier of the compact Real-ESRGAN path (SRVGGNetCompact): the host-only parts (checkpoint loader and dispatcher, registry, webui
hook, the reference restatement itself), the compiled kernel's metadata, and one run of tests/test_gpu_compact.py on the host-emulated
library."""
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

import compact_reference as R
import rrdb_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE_CASES = 2 + 1 + 3 + 3 + 2 + 4 + 1 + 6 + 1 + 1 + 1 + 1         # the cases of tests/test_gpu_compact.py


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_compact_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_compact.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= GPU_FILE_CASES, out[-2000:]


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def zeros_state_dict(num_conv, scale=4, num_feat=64, in_ch=3, prelu=True):
    sd = {}
    for i in range(num_conv + 2):
        o = 3 * scale * scale if i == num_conv + 1 else num_feat
        sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"] = torch.zeros(o, in_ch if i == 0 else num_feat, 3, 3), torch.zeros(o)
        if prelu and i <= num_conv:
            sd[f"body.{2 * i + 1}.weight"] = torch.zeros(num_feat)
    return sd


def blob_of(sd, num_conv):
    parts = []
    for i in range(num_conv + 2):
        parts += [sd[f"body.{2 * i}.weight"].flatten(), sd[f"body.{2 * i}.bias"].flatten()]
        if i <= num_conv:
            parts.append(sd[f"body.{2 * i + 1}.weight"].flatten())
    return torch.cat(parts).numpy()


@pytest.mark.parametrize("num_conv,scale", [(16, 4), (32, 4), (4, 2), (4, 3), (2, 1)])
def test_loader_reads_num_conv_and_scale_from_the_keys(num_conv, scale):
    up = sub("upscaler")
    sd = R.make_state_dict(num_conv, scale)
    blob, nc, s = up.parse_compact_state_dict(sd)
    assert (nc, s) == (num_conv, scale) and blob.dtype == np.float32
    assert np.array_equal(blob, blob_of(sd, num_conv))
    assert blob.size == (64 * 27 + 128) + num_conv * (64 * 576 + 128) + 3 * scale * scale * 577


@pytest.mark.parametrize("wrapper", ["params_ema", "params"])
def test_loader_unwraps_the_training_wrappers(wrapper):
    up = sub("upscaler")
    sd = R.make_state_dict(4, 4)
    blob = up.parse_compact_state_dict(sd)[0]
    assert np.array_equal(up.parse_compact_state_dict({wrapper: sd})[0], blob)
    both = {"params": zeros_state_dict(4), "params_ema": sd}                    # the EMA weights win, as for RRDBNets
    assert np.array_equal(up.parse_compact_state_dict(both)[0], blob)


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_compact_state_dict
    with pytest.raises(ValueError, match="num_feat = 48"):
        parse(zeros_state_dict(4, num_feat=48))
    sd = zeros_state_dict(4)
    sd["body.10.weight"], sd["body.10.bias"] = torch.zeros(75, 64, 3, 3), torch.zeros(75)          # r = 5
    with pytest.raises(ValueError, match="75 channels"):
        parse(sd)
    sd["body.10.weight"], sd["body.10.bias"] = torch.zeros(24, 64, 3, 3), torch.zeros(24)          # not 3 r^2
    with pytest.raises(ValueError, match="24 channels"):
        parse(sd)
    with pytest.raises(ValueError, match="takes 1 input channels"):
        parse(zeros_state_dict(4, in_ch=1))
    with pytest.raises(ValueError, match="no PReLU weight"):
        parse(zeros_state_dict(4, prelu=False) | {"body.1.weight": torch.zeros(64)})                # a relu build keeps no slopes
    sd = zeros_state_dict(4)
    sd["body.3.weight"] = torch.zeros(1)                                                           # PReLU(num_parameters=1)
    with pytest.raises(ValueError, match=r"body\.3: no PReLU weight of shape \(64,\)"):
        parse(sd)
    sd = zeros_state_dict(4)
    del sd["body.4.weight"], sd["body.4.bias"], sd["body.5.weight"]
    with pytest.raises(ValueError, match="without gaps"):
        parse(sd)
    sd = zeros_state_dict(4)
    sd["body.6.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(ValueError, match=r"body\.6: weight \(64, 64, 1, 1\)"):
        parse(sd)
    sd = zeros_state_dict(4)
    del sd["body.2.bias"]
    with pytest.raises(ValueError, match=r"body\.2: bias"):
        parse(sd)
    with pytest.raises(ValueError, match="not a compact"):
        parse({"layers.0.weight": torch.zeros(4, 4)})


def test_dispatcher_sends_each_key_layout_to_its_loader():
    up = sub("upscaler")
    rrdb = RR.make_state_dict(2, 4)
    for sd in (rrdb, RR.to_old_arch(rrdb, 2), {"params_ema": rrdb}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        want = up.parse_esrgan_state_dict(sd)
        assert family == "rrdb" and parsed[1:] == want[1:] == (2, 3, 4) and np.array_equal(parsed[0], want[0])
    compact = R.make_state_dict(4, 2)
    for sd in (compact, {"params": compact}):
        family, parsed = up.parse_upscaler_state_dict(sd)
        assert family == "compact" and parsed[1:] == (4, 2) and np.array_equal(parsed[0], blob_of(compact, 4))
    with pytest.raises(ValueError, match="not an RRDBNet checkpoint: neither conv_first.weight nor model.0.weight"):
        up.parse_upscaler_state_dict({"layers.0.weight": torch.zeros(4, 4)})              # what it said before there was a dispatcher
    with pytest.raises(ValueError, match="num_feat = 32"):
        up.parse_upscaler_state_dict(zeros_state_dict(4, num_feat=32))


def test_loader_reads_pth_and_safetensors_files(tmp_path):
    up = sub("upscaler")
    sd = R.make_state_dict(4, 4)
    blob = up.parse_compact_state_dict(sd)[0]
    torch.save({"params": sd}, str(tmp_path / "a.pth"))
    family, parsed = up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(str(tmp_path / "a.pth")))
    assert family == "compact" and np.array_equal(parsed[0], blob)
    st = pytest.importorskip("safetensors.torch")
    st.save_file(sd, str(tmp_path / "a.safetensors"))
    family, parsed = up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(str(tmp_path / "a.safetensors")))
    assert family == "compact" and parsed[1:] == (4, 4) and np.array_equal(parsed[0], blob)


# ---- registry, hook ------------------------------------------------------------------------------------------------------------------
def test_register_esrgan_takes_a_mixed_list(tmp_path, monkeypatch):
    up, shared = sub("upscaler"), sub("shared")
    monkeypatch.setattr(shared, "sd_upscalers", [])
    torch.save(RR.make_state_dict(2, 4), str(tmp_path / "rrdb_x4.pth"))
    torch.save({"params": zeros_state_dict(16, 4)}, str(tmp_path / "animevideo.pth"))
    torch.save(zeros_state_dict(4, 2), str(tmp_path / "compact_x2.pth"))
    added = up.register_esrgan({"R-ESRGAN 4x+": str(tmp_path / "rrdb_x4.pth"), "R-ESRGAN AnimeVideo": str(tmp_path / "animevideo.pth")})
    added += up.register_esrgan([str(tmp_path / "compact_x2.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "R-ESRGAN 4x+", "R-ESRGAN AnimeVideo", "compact_x2"]
    assert [d.scale for d in added] == [4, 4, 2] and added[0].scaler is added[1].scaler
    assert all(isinstance(d.scaler, up.UpscalerESRGAN) for d in added)
    torch.save(zeros_state_dict(4, num_feat=32), str(tmp_path / "narrow.pth"))
    with pytest.raises(ValueError, match="num_feat = 32"):
        up.register_esrgan([str(tmp_path / "narrow.pth")])


def test_install_esrgan_hook_runs_a_compact_checkpoint_on_the_engine(tmp_path, monkeypatch):
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, relu = str(tmp_path / "general_x4v3.pth"), str(tmp_path / "relu_build.pth")
    torch.save({"params": zeros_state_dict(32)}, good)
    torch.save({"params": zeros_state_dict(32, prelu=False)}, relu)

    class UpscalerRealESRGAN:                                  # the shape of the webui's scaler objects
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, path):
            self.stock_calls.append(path)
            return img
    scaler = UpscalerRealESRGAN()
    data = [types.SimpleNamespace(name="R-ESRGAN General 4xV3", data_path="https://example.invalid/realesr-general-x4v3.pth",
                                  local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="relu", data_path=relu, local_data_path=relu, scaler=scaler)]
    scaler.scalers = data
    engine_calls = []
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", lambda self, path: up.parse_upscaler_state_dict(up.load_esrgan_checkpoint(path)))
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    assert bridge.install_esrgan_hook(types.SimpleNamespace(sd_upscalers=data)) == ["R-ESRGAN General 4xV3", "relu"]
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, data[0].data_path)                  # resolved to the local file; a compact checkpoint loads: the engine
    assert engine_calls == [good] and scaler.stock_calls == []
    scaler.do_upscale(img, relu)                               # no PReLU slopes: the loader refuses, the stock path runs it
    assert engine_calls == [good] and scaler.stock_calls == [relu]


def test_make_upscaler_net_picks_the_class_by_the_keys(monkeypatch):
    up = sub("upscaler")
    made = []
    monkeypatch.setattr(up.EsrganNet, "__init__", lambda self, sd, device=0, engine=None: made.append("rrdb"))
    monkeypatch.setattr(up.CompactNet, "__init__", lambda self, sd, device=0, engine=None: made.append("compact"))
    assert isinstance(up.make_upscaler_net(RR.make_state_dict(1, 4)), up.EsrganNet)
    assert isinstance(up.make_upscaler_net({"params_ema": zeros_state_dict(2)}), up.CompactNet)
    assert made == ["rrdb", "compact"]


def test_too_large_an_input_is_refused(monkeypatch):
    up = sub("upscaler")
    net = up.CompactNet.__new__(up.CompactNet)
    net.scale, net.device, net.handle = 4, 0, None
    net.engine = types.SimpleNamespace(arena_bytes=lambda: 1000)
    monkeypatch.setattr(up.CompactNet, "scratch_bytes", lambda self, b, h, w: 5000)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 4000)
    net.check_fits(1, 512, 512)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 3999)
    with pytest.raises(up.EsrganInputTooLarge, match=r"512x512 \(batch 1\) is too large for the x4 upscaler"):
        net.check_fits(1, 512, 512)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 1 << 62)
    with pytest.raises(up.EsrganInputTooLarge, match="too large"):
        net.check_fits(1, 11600, 11600)                                       # 16 H W reaches 2^31 output pixels


# ---- the kernel as compiled ------------------------------------------------------------------------------------------------------------
def test_compact_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of both instantiations, from the metadata: no scratch, no spills, at most 512 VGPRs (one workgroup per
    CU: LDS decides the occupancy, not registers); from the body: MFMAs in whole K steps of 16, ds_read_b128 operand reads, LDS-DMA
    staging and ONE barrier (per tile; none in the K loop)."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("compact")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    for cin, name in ((32, "_ZN4sdmi19compact_conv_kernelILi32EEEvNS_8CompactPE"), (64, "_ZN4sdmi19compact_conv_kernelILi64EEEvNS_8CompactPE")):
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (cin, m)
        assert m["vgpr_count"] <= 512, (cin, m)
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body
        assert body.count("v_mfma_f32_16x16x32_f16") == (cin // 32) * 9 * 16, cin
        assert "ds_read_b128" in body and "global_load_lds_dwordx4" in body
        assert body.count("s_barrier") == 1, cin


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_two_pixels_by_hand():
    """A 1 x 2 image, num_conv 1, x2.  conv 0 copies input channel 0 to feature 0 with weight 2 (centre tap) and bias -1; its PReLU has
    slope 0.5 on feature 0; conv 1 (the body conv) copies feature 0 from the LEFT neighbour (tap (1, 0)), PReLU slope 0.25; the last conv
    sends feature 0 (centre tap) to output channel 1's sub-pixel (dy, dx) = (1, 0), i.e. channel 1 * 4 + 2 = 6, with weight 3.
    Pixels p0 = 0.75, p1 = 0.25 (all three colour channels):
      conv 0:  2 * 0.75 - 1 = 0.5 -> 0.5;  2 * 0.25 - 1 = -0.5 -> PReLU -0.25
      conv 1:  pixel 0 reads the zero padding -> 0;  pixel 1 reads pixel 0 -> 0.5;  PReLU leaves both
      last:    channel 6: 0 and 1.5
      out:     base everywhere, plus 1.5 at channel 1, row 1, column 2 (= pixel 1's (dy 1, dx 0))."""
    sd = zeros_state_dict(1, scale=2)
    sd["body.0.weight"][0, 0, 1, 1], sd["body.0.bias"][0] = 2.0, -1.0
    sd["body.1.weight"][0] = 0.5
    sd["body.2.weight"][0, 0, 1, 0] = 1.0
    sd["body.3.weight"][0] = 0.25
    sd["body.4.weight"][6, 0, 1, 1] = 3.0
    x = torch.tensor([0.75, 0.25]).view(1, 1, 1, 2).expand(1, 3, 1, 2).contiguous()
    want = torch.tensor([[0.75, 0.75, 0.25, 0.25]] * 2).expand(1, 3, 2, 4).clone()
    want[0, 1, 1, 2] += 1.5
    assert torch.allclose(R.forward(sd, x), want, atol=1e-6)
    sd["body.2.weight"].zero_()
    sd["body.2.weight"][0, 0, 1, 2] = 1.0                      # the RIGHT neighbour: pixel 0 reads pixel 1's -0.25 -> PReLU -0.0625
    want = torch.tensor([[0.75, 0.75, 0.25, 0.25]] * 2).expand(1, 3, 2, 4).clone()
    want[0, 1, 1, 0] += 3.0 * -0.0625
    assert torch.allclose(R.forward(sd, x), want, atol=1e-6)
    assert (R.num_conv_of(sd), R.scale_of(sd)) == (1, 2)


def test_reference_output_is_an_image_with_a_visible_residual():
    """The nets and inputs of the GPU tests: fewer than 5 % of the fp32 reference's output bytes are 0 or 255, and for num_conv <= 16 the
    residual (out - nearest base) has a spread of at least 0.1; the fp16-storage twin is close to, but not equal to, the reference."""
    to_u8 = sub("upscaler").model_output_to_u8
    for num_conv, scale, b, h, w in ((4, 4, 2, 12, 20), (16, 4, 1, 17, 13), (4, 2, 1, 12, 20), (4, 3, 1, 9, 11), (4, 1, 1, 16, 24),
                                     (32, 4, 1, 33, 35), (2, 4, 1, 8, 8)):
        sd = R.make_state_dict(num_conv, scale)
        x = R.image(b, h, w, 10 + scale)
        assert torch.equal(torch.round(x * 255) / 255, x) and 0.34 < float(x.min()) and float(x.max()) < 0.66
        y = R.forward(sd, x)
        assert y.shape == (b, 3, h * scale, w * scale)
        u8 = to_u8(y.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, (num_conv, scale)
        res = y - R.base(sd, x)
        if num_conv <= 16:
            assert float(res.std()) >= 0.1, (num_conv, scale, float(res.std()))
        rel = float(((R.fp16_twin(sd, x) - R.base(sd, x)) - res).norm() / res.norm())
        assert 1e-4 < rel < 1e-2, (num_conv, scale, rel)
