"""CPU tier of the RRDBNet (ESRGAN / Real-ESRGAN) path: the host-only parts (checkpoint loader, uint8 hand-off, size refusal, registry,
webui hook, the reference restatement itself) and one run of tests/test_gpu_esrgan.py on the host-emulated library."""
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

import rrdb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_LEVEL_CASES = 5 + 2 + 2 + 1 + 1 + 2 + 1          # the op-level cases of tests/test_gpu_esrgan.py


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


# ---- the emulated run -------------------------------------------------------------------------------------------------------------
def test_gpu_esrgan_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_esrgan.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= OP_LEVEL_CASES, out[-2000:]


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def zeros_state_dict(num_block, in_ch=3, num_feat=64, growth=32):
    sd = {}
    for n in R.conv_names(num_block):
        o, i = R.conv_shape(n, in_ch)
        o = {64: num_feat, 32: growth}.get(o, o)
        if ".conv" in n:
            i = num_feat + growth * (int(n[-1]) - 1)
        elif n != "conv_first":
            i = num_feat
        sd[n + ".weight"], sd[n + ".bias"] = torch.zeros(o, i, 3, 3), torch.zeros(o)
    return sd


@pytest.mark.parametrize("num_block", [2, 6, 23])
@pytest.mark.parametrize("old_arch", [False, True])
def test_loader_reads_both_key_layouts_and_the_block_count(num_block, old_arch):
    up = sub("upscaler")
    sd = R.make_state_dict(num_block, 4)
    blob, nb, in_ch, scale = up.parse_esrgan_state_dict(R.to_old_arch(sd, num_block) if old_arch else sd)
    assert (nb, in_ch, scale) == (num_block, 3, 4) and blob.dtype == np.float32
    want = torch.cat([sd[n + leaf].flatten() for n in R.conv_names(num_block) for leaf in (".weight", ".bias")]).numpy()
    assert np.array_equal(blob, want)
    convs = 64 * 3 * 9 + 64 + num_block * 3 * sum((32 if k < 4 else 64) * (64 + 32 * k) * 9 + (32 if k < 4 else 64) for k in range(5))
    assert blob.size == convs + 4 * (64 * 64 * 9 + 64) + 3 * 64 * 9 + 3


@pytest.mark.parametrize("wrapper", ["params_ema", "params"])
def test_loader_unwraps_the_training_wrappers(wrapper):
    up = sub("upscaler")
    sd = R.make_state_dict(2, 4)
    blob, nb, _, _ = up.parse_esrgan_state_dict({wrapper: sd})
    assert nb == 2 and np.array_equal(blob, up.parse_esrgan_state_dict(sd)[0])
    both = {"params": zeros_state_dict(2), "params_ema": sd}                 # the EMA weights win, as in the reference's loaders
    assert np.array_equal(up.parse_esrgan_state_dict(both)[0], blob)


@pytest.mark.parametrize("in_ch,scale", [(3, 4), (12, 2), (48, 1)])
def test_loader_reads_the_scale_from_conv_first(in_ch, scale):
    assert sub("upscaler").parse_esrgan_state_dict(zeros_state_dict(2, in_ch))[1:] == (2, in_ch, scale)


def test_loader_refuses_what_the_engine_is_not_built_for():
    parse = sub("upscaler").parse_esrgan_state_dict
    with pytest.raises(ValueError, match="num_feat = 32"):
        parse(zeros_state_dict(2, num_feat=32))
    with pytest.raises(ValueError, match="num_grow_ch = 16"):
        parse(zeros_state_dict(2, growth=16))
    with pytest.raises(ValueError, match="takes 4 channels"):
        parse(zeros_state_dict(2, in_ch=4))
    with pytest.raises(ValueError, match="not an RRDBNet"):
        parse({"layers.0.weight": torch.zeros(4, 4)})
    sd = zeros_state_dict(2)
    del sd["body.1.rdb2.conv3.bias"]
    with pytest.raises(ValueError, match="lacks"):
        parse(sd)
    sd = zeros_state_dict(3)
    for k in [k for k in sd if k.startswith("body.1.")]:
        del sd[k]
    with pytest.raises(ValueError, match="not 0..n-1"):
        parse(sd)
    # old-arch x2: conv_up1 at model.3, then HR conv / last conv at model.5 / model.7
    old = R.to_old_arch(zeros_state_dict(2), 2)
    x2 = {k.replace("model.6.", "model.5.").replace("model.8.", "model.7."): v for k, v in old.items() if not k.startswith("model.10.")}
    with pytest.raises(ValueError, match="not a x4 model"):
        parse(x2)
    sd = zeros_state_dict(2)
    sd["conv_hr.weight"] = torch.zeros(64, 32, 3, 3)
    with pytest.raises(ValueError, match="conv_hr"):
        parse(sd)


def test_loader_reads_pth_files(tmp_path):
    up = sub("upscaler")
    sd = R.make_state_dict(2, 4)
    torch.save({"params_ema": sd}, str(tmp_path / "a.pth"))
    blob = up.parse_esrgan_state_dict(sd)[0]
    assert np.array_equal(up.parse_esrgan_state_dict(up.load_esrgan_checkpoint(str(tmp_path / "a.pth")))[0], blob)


def test_loader_reads_safetensors_files(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    up = sub("upscaler")
    sd = R.make_state_dict(2, 4)
    st.save_file(sd, str(tmp_path / "a.safetensors"))
    assert np.array_equal(up.parse_esrgan_state_dict(up.load_esrgan_checkpoint(str(tmp_path / "a.safetensors")))[0],
                          up.parse_esrgan_state_dict(sd)[0])


# ---- uint8 hand-off, size refusal ----------------------------------------------------------------------------------------------------
def test_uint8_hand_off_rounds_half_to_even():
    """A ramp through the 255 half-levels k + 0.5: the members that are still exactly k + 0.5 after the fp32 /255 and x255 go to the
    EVEN neighbour (np.round), where adding 0.5 and truncating would send every one of them up; values outside [0, 1] are clamped."""
    to_u8 = sub("upscaler").model_output_to_u8
    levels = np.arange(0, 255, dtype=np.float32) + np.float32(0.5)
    ramp = levels / np.float32(255.0)
    exact = (ramp * np.float32(255.0)) == levels
    assert exact.sum() > 100
    got = to_u8(ramp[exact])
    k = np.floor(levels[exact]).astype(np.int64)
    assert np.array_equal(got, np.where(k % 2 == 0, k, k + 1).astype(np.uint8))
    assert bool((got % 2 == 0).all()) and not np.array_equal(got, (k + 1).astype(np.uint8))
    assert list(to_u8(np.array([-0.3, 1.7, 0.0, 1.0, 0.2], dtype=np.float32))) == [0, 255, 0, 255, 51]


def test_too_large_an_input_is_refused_with_a_clear_error(monkeypatch):
    """The need is the engine's own figure (sdmi_esrgan_scratch_bytes, mocked here); what is available is the free device memory plus
    the arena the engine already holds, which a larger run replaces."""
    up = sub("upscaler")
    net = up.EsrganNet.__new__(up.EsrganNet)
    net.scale, net.device, net.handle = 4, 0, None
    net.engine = types.SimpleNamespace(arena_bytes=lambda: 1000)
    monkeypatch.setattr(up.EsrganNet, "scratch_bytes", lambda self, b, h, w: 5000)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 4000)
    net.check_fits(1, 512, 512)                                               # 4000 free + 1000 held = 5000
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 3999)
    with pytest.raises(up.EsrganInputTooLarge, match=r"512x512 \(batch 1\) is too large for the x4 upscaler"):
        net.check_fits(1, 512, 512)
    assert issubclass(up.EsrganInputTooLarge, ValueError)
    net.engine = types.SimpleNamespace(arena_bytes=lambda: 5000)            # a second run of the same image: the arena is already there
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 0)
    net.check_fits(1, 512, 512)
    monkeypatch.setattr(up, "arena_limit_bytes", lambda device=0: 1 << 62)
    with pytest.raises(up.EsrganInputTooLarge, match="too large"):
        net.check_fits(1, 11600, 11600)                                       # 16 B H W reaches 2^31 output pixels


# ---- registry, hook ------------------------------------------------------------------------------------------------------------------
def test_register_esrgan_and_name_resolution(tmp_path, monkeypatch):
    up, shared = sub("upscaler"), sub("shared")
    monkeypatch.setattr(shared, "sd_upscalers", [])
    for name, scale in (("a_x4", 4), ("b_x2", 2)):
        torch.save(zeros_state_dict(2, {4: 3, 2: 12}[scale]), str(tmp_path / f"{name}.pth"))
    added = up.register_esrgan({"R-ESRGAN 4x+": str(tmp_path / "a_x4.pth")})
    added += up.register_esrgan([str(tmp_path / "b_x2.pth")])
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "R-ESRGAN 4x+", "b_x2"]
    assert [d.scale for d in added] == [4, 2] and all(isinstance(d.scaler, up.UpscalerESRGAN) for d in added)
    assert [d.name for d in up.builtin_upscalers()] == ["None", "Lanczos", "Nearest"]
    calls = []

    def fake(img, selected_model=None):
        calls.append(selected_model)
        return img.resize((img.width * 4, img.height * 4))
    monkeypatch.setattr(added[0].scaler, "do_upscale", fake)
    out = up._resize_to(Image.new("RGB", (16, 16)), 40, 40, "R-ESRGAN 4x+")
    assert out.size == (40, 40) and calls == [str(tmp_path / "a_x4.pth")]
    monkeypatch.setattr(shared.opts, "upscaler_for_img2img", "R-ESRGAN 4x+")
    assert up.resize_image(0, Image.new("RGB", (16, 16)), 32, 32).size == (32, 32) and len(calls) == 2


def test_install_esrgan_hook_wraps_the_webui_scalers(tmp_path, monkeypatch):
    up, bridge = sub("upscaler"), sub("webui_bridge")
    good, bad = str(tmp_path / "good.pth"), str(tmp_path / "bad.pth")
    torch.save(zeros_state_dict(2), good)
    torch.save(zeros_state_dict(2, num_feat=32), bad)

    class UpscalerRealESRGAN:                                  # the shape of the webui's scaler objects
        def __init__(self):
            self.scalers, self.stock_calls = [], []

        def do_upscale(self, img, path):
            self.stock_calls.append(path)
            return img

    class UpscalerLanczos(UpscalerRealESRGAN):
        pass
    scaler, other = UpscalerRealESRGAN(), UpscalerLanczos()
    data = [types.SimpleNamespace(name="R-ESRGAN 4x+", data_path="https://example.invalid/x4.pth", local_data_path=good, scaler=scaler),
            types.SimpleNamespace(name="odd", data_path=bad, local_data_path=bad, scaler=scaler),
            types.SimpleNamespace(name="Lanczos", data_path=None, local_data_path=None, scaler=other)]
    scaler.scalers = data[:2]
    engine_calls = []
    monkeypatch.setattr(up.UpscalerESRGAN, "load_model", lambda self, path: up.parse_esrgan_state_dict(up.load_esrgan_checkpoint(path)))
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", lambda self, img, path=None: engine_calls.append(path) or img)
    webui_shared = types.SimpleNamespace(sd_upscalers=data)
    assert bridge.install_esrgan_hook(webui_shared) == ["R-ESRGAN 4x+", "odd"]
    assert not hasattr(other.do_upscale, "_mi355x_stock")
    img = Image.new("RGB", (8, 8))
    scaler.do_upscale(img, data[0].data_path)                  # resolved to the local file, run on the engine
    assert engine_calls == [good] and scaler.stock_calls == []
    scaler.do_upscale(img, bad)                                # not a 64 / 32 RRDBNet: the stock path
    assert engine_calls == [good] and scaler.stock_calls == [bad]
    assert bridge.install_esrgan_hook(webui_shared) == ["R-ESRGAN 4x+", "odd"]          # idempotent
    scaler.do_upscale(img, good)
    assert engine_calls == [good, good] and scaler.stock_calls == [bad]
    broken = str(tmp_path / "broken.pth")                      # a file the loader cannot read at all: the stock path, as before the hook
    open(broken, "wb").write(b"not a checkpoint")
    scaler.do_upscale(img, broken)
    assert engine_calls == [good, good] and scaler.stock_calls == [bad, broken]

    def too_large(self, img, path=None):
        raise up.EsrganInputTooLarge("image too large")
    monkeypatch.setattr(up.UpscalerESRGAN, "do_upscale", too_large)
    scaler.do_upscale(img, good)                               # the stock path tiles what the arena cannot hold whole
    assert scaler.stock_calls == [bad, broken, good]


# ---- the kernel as compiled ------------------------------------------------------------------------------------------------------------
def test_rrdb_kernels_compile_lean_for_gfx950():
    """The gfx950 code objects of both instantiations: no scratch, no spills, at most 256 VGPRs (two workgroups per CU) and the LDS of the
    two weight stage slots; the pixel gathers are awaited by COUNT (a step's MFMAs run under the next step's loads), and a K step is
    4 gathers, NOUT / 16 LDS reads and 4 NOUT / 16 MFMAs."""
    from test_cpu_host import _gfx950_assembly
    asm = _gfx950_assembly("rrdb")
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block)}
    kernels = {32: "_ZN4sdmi16rrdb_conv_kernelILi32ELi9EEEvNS_5RrdbPE", 64: "_ZN4sdmi16rrdb_conv_kernelILi64ELi3EEEvNS_5RrdbPE"}
    for nout, name in kernels.items():
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (nout, m)
        assert m["vgpr_count"] <= 256, (nout, m)
        assert m["group_segment_fixed_size"] == {32: 2 * 20 * 1024, 64: 2 * 12 * 1024}[nout], (nout, m)
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body
        assert body.count("v_mfma_f32_16x16x32_f16") % (4 * nout // 16) == 0 and body.count("v_mfma_f32_16x16x32_f16") >= 2 * 4 * nout // 16
        counted = [int(n) for n in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)]
        assert any(n >= 4 for n in counted), (nout, sorted(set(counted)))      # some wait leaves the 4 gathers of the next step in flight
        assert "global_load_lds_dwordx4" in body and "ds_read_b128" in body


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_rdb_by_hand():
    """One RDB whose convs copy: conv_k's only non-zero weights are centre taps of 1 from input channel 0 to its output channel 0, all
    biases 0.  For x > 0 in channel 0:  x1 = x2 = x3 = x4 = x (channel 0), x5 = x, so the block returns 0.2 x + x = 1.2 x in channel
    0 and x unchanged elsewhere; for x < 0 the LeakyReLU gives x1 = 0.2 x, x2 = x3 = x4 = 0.2 x (each reads channel 0 of x, not of the
    previous feature), conv5 reads channel 0 of x as well -> again 1.2 x.  With conv5 reading x4 instead (input channel 64 + 96): for
    x < 0, x5 = 0.2 x and the block returns 0.04 x + x = 1.04 x."""
    sd = {}
    for k in (1, 2, 3, 4, 5):
        o, i = R.conv_shape(f"body.0.rdb1.conv{k}")
        w = torch.zeros(o, i, 3, 3)
        w[0, 0, 1, 1] = 1.0
        sd[f"p.conv{k}.weight"], sd[f"p.conv{k}.bias"] = w, torch.zeros(o)
    x = torch.randn(1, 64, 5, 4, generator=torch.Generator().manual_seed(1))
    want = x.clone()
    want[:, 0] = 1.2 * x[:, 0]
    assert torch.allclose(R.rdb(sd, "p", x, lambda t: t), want, atol=1e-6)
    sd["p.conv5.weight"].zero_()
    sd["p.conv5.weight"][0, 64 + 96, 1, 1] = 1.0               # channel 0 of x4 in cat(x, x1, x2, x3, x4)
    want[:, 0] = torch.where(x[:, 0] > 0, 1.2 * x[:, 0], 1.04 * x[:, 0])
    assert torch.allclose(R.rdb(sd, "p", x, lambda t: t), want, atol=1e-6)


def test_reference_output_is_an_image_not_a_saturated_one():
    """With the test weights the fp32 reference's output bytes are not pinned at 0 / 255 (fewer than 5 %), for every scale the GPU tests
    use; and the fp16-storage twin is close to, but not equal to, the reference."""
    to_u8 = sub("upscaler").model_output_to_u8
    for scale, (h, w) in ((4, (12, 20)), (2, (12, 20)), (1, (16, 24))):
        sd = R.make_state_dict(2, scale)
        x = torch.rand((1, 3, h, w), generator=torch.Generator().manual_seed(3))
        y = R.forward(sd, x)
        assert y.shape == (1, 3, h * scale, w * scale)
        u8 = to_u8(y.numpy())
        assert ((u8 == 0) | (u8 == 255)).mean() < 0.05, scale
        assert u8.std() > 8                                     # and it is not flat either
        twin = R.fp16_twin(sd, x)
        rel = float((twin - y).norm() / y.norm())
        assert 1e-4 < rel < 5e-3, (scale, rel)
