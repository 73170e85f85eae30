"""GPU parity tests of the ScuNET path: the fused window-block kernel through sdmi_scu_block against the float64 graph on the same fp16
operands, the ReLU epilogue of sdmi_rrdb_conv against float64, whole networks through sdmi_scunet_run against tests/scunet_reference.py
(fp32, CPU), UpscalerESRGAN.do_upscale on a ScuNET checkpoint and one resize through the registry.

Comparison rule: that of tests/test_gpu_swinir.py (`assert_parity`, copied unchanged): the yardstick is the distance of the fp16-storage
twin from the reference; the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per channel, per
image row) within 2.5 x the yardstick, the yardstick itself is asserted above 1e-4 and the twin's own worst slice within 2.5 x of it
(inputs on which the rule could not decide fail the test instead of passing it).  The cases also run on the host-emulated library
(tests/test_cpu_scunet.py)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scunet_reference as R
from fp16_emu import r16
from helpers import rel_l2, seeded, worst_slice_rel_l2

pytestmark = pytest.mark.gpu


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


def assert_parity(got, ref, twin, channel_dim, row_dims, ctx=None):
    got, ref, twin = got.double().cpu(), ref.double(), twin.double()
    yard = rel_l2(twin, ref)
    err = rel_l2(got, ref)
    print(f"[scunet parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
    assert yard > 1e-4, (ctx, yard)
    for keep in ((channel_dim,), row_dims):
        worst, idx = worst_slice_rel_l2(twin, ref, keep)
        assert worst <= 2.5 * yard, (ctx, "the twin's own slices over dims", keep, "worst at", idx, worst, yard)
    assert err <= 1.25 * yard, (ctx, err, yard)
    for keep in ((channel_dim,), row_dims):
        worst, idx = worst_slice_rel_l2(got, ref, keep)
        assert worst <= 2.5 * yard, (ctx, "slices over dims", keep, "worst at", idx, worst, yard)
    return err, yard


def r16d(t):
    return t.half().double()


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


# ---- the window block -------------------------------------------------------------------------------------------------------------
BLOCKS = {}
PRE = "blk."


def block_case(b, h, w, c):
    """Seeded weights of one Block (matrices as fp16 values) and token rows [b, h, w, c] (fp16 values, a per-token offset on top of the
    spread); the float64 graphs are computed once per case and shared."""
    key = (b, h, w, c)
    if key not in BLOCKS:
        sd = {}
        R.make_block(sd, PRE, c, torch.Generator().manual_seed(900 + 3 * c + h + w))
        sd = R.round_weights(sd)
        x = r16(seeded((b, h, w, c), 901 + c + h, 1.0) + seeded((b, h, w, 1), 902 + c + h, 0.5))
        BLOCKS[key] = dict(sd=sd, sd64={k: v.double() for k, v in sd.items()}, x=x, c=c, graphs={}, dev={})
    return BLOCKS[key]


def graph(case, shift, rnd=R.ident, **drop):
    key = (shift, rnd is R.ident, tuple(sorted(drop.items())))
    if key not in case["graphs"]:
        case["graphs"][key] = R.block(case["sd64"], PRE, case["x"].double(), shift, rnd, **drop)
    return case["graphs"][key]


def on_device(dev, case):
    """(packs, expanded bias) of a case on the GPU, made once."""
    if not case["dev"]:
        ops, sd = sub("ops"), case["sd"]
        t = [sd[PRE + n].to(dev) for n in ("ln1.weight", "ln1.bias", "msa.embedding_layer.weight", "msa.embedding_layer.bias", "msa.linear.weight",
                                           "msa.linear.bias", "ln2.weight", "ln2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias")]
        case["dev"]["packs"] = ops.scu_block_pack(*t)
        case["dev"]["bias"] = R.relative_bias(sd[PRE + "msa.relative_position_params"]).contiguous().to(dev)
    return case["dev"]["packs"], case["dev"]["bias"]


def run_block(dev, case, shift, x=None, **kw):
    packs, bias = on_device(dev, case)
    x = case["x"].half().to(dev) if x is None else x
    return sub("ops").scu_block(x, packs, bias, case["c"], shift=shift, **kw)


@pytest.mark.parametrize("b,h,w,c,shift", [
    (2, 16, 24, 32, 0), (2, 16, 24, 32, 4),      # 2 x 3 windows: no window is interior when shifted
    (1, 24, 40, 32, 4),                          # interior windows
    (1, 8, 8, 32, 4), (1, 8, 8, 64, 4),          # one window wrapped onto itself
    (2, 16, 24, 64, 4), (1, 16, 16, 64, 0)])
def test_scu_block_vs_float64_graph(dev, b, h, w, c, shift):
    case = block_case(b, h, w, c)
    out = run_block(dev, case, shift)
    assert out.shape == (b, h, w, c) and out.dtype == torch.float16
    ref, twin = graph(case, shift), graph(case, shift, r16d)
    _, yard = assert_parity(out, ref, twin, 3, (0, 1), f"scu_block B{b} {h}x{w} C {c} shift {shift}")
    got = out.cpu()
    if shift:                                    # every term is really applied
        assert rel_l2(got, graph(case, shift, mask=False)) > 10 * yard
    assert rel_l2(got, graph(case, shift, bias=False)) > 10 * yard
    assert rel_l2(got, graph(case, shift, mlp=False)) > 10 * yard


def test_scu_block_in_rows_wider_than_the_block(dev):
    """The ConvTransBlock's own use: the input is columns 32..63 of 64-wide rows whose other columns hold 1e4, the output goes into
    columns 32..63 of a pre-filled 72-wide buffer.  The excess keeps its bits, the result is bit-equal to the dense call."""
    case = block_case(2, 16, 24, 32)
    dense = run_block(dev, case, 4)
    wide = torch.full((2, 16, 24, 64), 1e4, dtype=torch.float16)
    wide[..., 32:] = case["x"].half()
    out = torch.full((2, 16, 24, 72), 3.0, dtype=torch.float16).to(dev)
    got = run_block(dev, case, 4, x=wide.to(dev), col=32, out=out, out_col=32)
    assert got is out
    assert bool((out.cpu()[..., :32] == 3).all()) and bool((out.cpu()[..., 64:] == 3).all())
    assert same_bits(out[..., 32:64], dense)


@pytest.mark.parametrize("c,shift", [(32, 4), (64, 0)])
def test_scu_block_in_place_equals_out_of_place(dev, c, shift):
    case = block_case(2, 16, 24, c)
    dense = run_block(dev, case, shift)
    x = case["x"].half().to(dev)
    got = run_block(dev, case, shift, x=x, out=x)
    assert got is x and same_bits(x, dense)


def test_scu_block_refuses_what_it_is_not_built_for(dev):
    """Every refusal returns non-zero with a message and writes nothing."""
    _lib = sub("_lib")
    L = _lib.lib
    case = block_case(1, 16, 16, 64)
    packs, bias = on_device(dev, case)
    x = torch.zeros((1, 16, 16, 72), dtype=torch.float16).to(dev)
    out = torch.full((1, 16, 16, 72), 7.0, dtype=torch.float16).to(dev)

    def desc(**kw):
        d = _lib.ScuBlockDesc()
        d.x, d.out, d.packs, d.bias = x.data_ptr(), out.data_ptr(), packs.data_ptr(), bias.data_ptr()
        d.B, d.H, d.W, d.C, d.ldx, d.ldo, d.shift = 1, 16, 16, 64, 72, 72, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert L.sdmi_scu_block(ctypes.byref(desc()), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = [(dict(x=None), "null"), (dict(out=None), "null"), (dict(packs=None), "null"), (dict(bias=None), "null"),
           (dict(C=48), "trans_dim C = 32"), (dict(C=128), "trans_dim C = 32"), (dict(shift=2), "shift must be 0"), (dict(shift=-4), "shift must be 0"),
           (dict(H=12), "multiples of the window size 8"), (dict(W=0), "multiples of the window size 8"), (dict(B=0), "multiples of the window size 8"),
           (dict(ldx=56), "row strides too small"), (dict(ldo=32), "row strides too small"),
           (dict(x=x.data_ptr() + 2), "misaligned"), (dict(out=out.data_ptr() + 8), "misaligned"), (dict(bias=bias.data_ptr() + 4), "misaligned"),
           (dict(packs=packs.data_ptr() + 8), "misaligned"), (dict(ldx=68), "misaligned"), (dict(ldo=76), "misaligned")]
    for kw, msg in bad:
        assert L.sdmi_scu_block(ctypes.byref(desc(**kw)), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert L.sdmi_scu_block(None, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())
    # the pack: its size per width, and what it refuses
    assert L.sdmi_scu_block_pack_bytes(64) == packs.numel() and 0 < L.sdmi_scu_block_pack_bytes(32) < packs.numel()
    assert L.sdmi_scu_block_pack_bytes(48) == 0
    before = packs.clone()
    p = [_lib.ptr(bias)] * 12
    assert L.sdmi_scu_block_pack(*p, _lib.ptr(packs), 48, _lib.stream_ptr()) != 0 and "trans_dim 32 and 64" in _lib.last_error()
    assert L.sdmi_scu_block_pack(None, *p[1:], _lib.ptr(packs), 64, _lib.stream_ptr()) != 0 and "null" in _lib.last_error()
    assert L.sdmi_scu_block_pack(*p, packs.data_ptr() + 8, 64, _lib.stream_ptr()) != 0 and "16-byte aligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(packs.cpu(), before.cpu())


# ---- the ReLU epilogue of rrdb_conv -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,nout", [(32, 32), (64, 64)])
def test_rrdb_conv_relu_epilogue_vs_float64(dev, cin, nout):
    """conv_block.0 + ReLU of a ConvTransBlock at the two widths rrdb_conv serves, 2 x 9 x 11 (198 pixels: one ragged tile across two
    images), no bias, the input a channel prefix of wider rows."""
    ops = sub("ops")
    x = r16(seeded((2, 9, 11, 2 * cin), 70 + cin))
    w = r16(seeded((nout, cin, 3, 3), 71 + cin, (9 * cin) ** -0.5))
    got = ops.rrdb_conv(x.half().to(dev), ops.pack_rrdb_weight(w.to(dev), nout), None, cin=cin, ep="relu")
    assert got.shape == (2, 9, 11, nout)
    conv = F.conv2d(x[..., :cin].permute(0, 3, 1, 2).double(), w.double(), None, padding=1).permute(0, 2, 3, 1)
    ref = F.relu(conv)
    assert_parity(got, ref, r16d(ref), 3, (0, 1), f"rrdb_conv relu cin {cin} nout {nout}")
    assert bool((got.cpu() >= 0).all()) and 0.3 < float((got.cpu() == 0).float().mean()) < 0.7
    assert rel_l2(got.cpu(), conv) > 0.5                   # not the epilogue without the activation


# ---- network level ----------------------------------------------------------------------------------------------------------------
NET_CASES = {                                       # name: (depths, (b, h, w)); between them every kernel route sees 'W' and 'SW'
    "d2": ((2,) * 7, (2, 64, 64)),
    "d2111112-ragged": ((2, 1, 1, 1, 1, 1, 2), (1, 70, 100)),                   # replicate pad to 128 x 128, crop
    "d1222221": ((1, 2, 2, 2, 2, 2, 1), (1, 64, 128)),
    "d1-small": ((1,) * 7, (1, 24, 40)),                                        # one 64 x 64 grid: the host-path tests' network
}
NETS, REFS, ENGINE = {}, {}, []


def shared_engine():
    if not ENGINE:
        ENGINE.append(sub("engine").Engine(0))
    return ENGINE[0]


def net_for(depths):
    if depths not in NETS:
        sd = R.make_state_dict(depths)
        NETS[depths] = (sd, sub("upscaler").ScuNETNet(sd, device=0, engine=shared_engine()))
    return NETS[depths]


def reference_for(name):
    """(x, fp32 reference, fp16-storage twin) of a case: computed once, shared, never modified."""
    if name not in REFS:
        depths, (b, h, w) = NET_CASES[name]
        sd = R.make_state_dict(depths)
        x = R.image(b, h, w, 11)
        REFS[name] = (x, R.forward(sd, x), R.fp16_twin(sd, x))
    return REFS[name]


@pytest.mark.parametrize("name", list(NET_CASES))
def test_scunet_network_vs_reference(dev, name):
    depths, (b, h, w) = NET_CASES[name]
    sd, net = net_for(depths)
    assert net.scale == 1 and net.config == R.config_of(sd)
    x, ref, twin = reference_for(name)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h, w) and got.dtype == torch.float32
    assert 0 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    assert_parity(got, ref, twin, 1, (0, 2), f"network {name} {b}x{h}x{w}")


def test_scunet_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_scunet_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB).  24 x 40 pads
    to one 64 x 64 grid."""
    name = "d1-small"
    depths, (b, h, w) = NET_CASES[name]
    engine = sub("engine").Engine(0)
    net = sub("upscaler").ScuNETNet(R.make_state_dict(depths), device=0, engine=engine)
    assert engine.arena_bytes() == 0
    got = net.run(R.image(b, h, w, 11).to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, h, w) and 0 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


SMALL = "d1-small"


def test_scunet_uint8_in_and_out(dev):
    """uint8 in is the same image: the same output; uint8 out is model_output_to_u8 of the same run's fp32 output, byte for byte."""
    up = sub("upscaler")
    depths, (b, h, w) = NET_CASES[SMALL]
    sd, net = net_for(depths)
    x = reference_for(SMALL)[0]
    x8 = torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    f32 = net.run(x8)
    assert float((f32.cpu() - net.run(x.to(dev)).cpu()).abs().max()) < 1e-6
    u8 = net.run(x8, out_u8=True)
    assert u8.shape == (b, h, w, 3) and u8.dtype == torch.uint8
    assert np.array_equal(u8.cpu().numpy(), up.model_output_to_u8(f32.cpu().permute(0, 2, 3, 1).numpy()))


def test_scunet_handle_entries_directly(dev):
    """The C entries by name: blob_floats, create (and what it refuses), scratch_bytes, run (and what it refuses), destroy."""
    _lib, up = sub("_lib"), sub("upscaler")
    L = _lib.lib
    depths, (b, h, w) = NET_CASES[SMALL]
    sd = R.make_state_dict(depths)
    blob, config = up.parse_scunet_state_dict(sd)

    def cfg_c(d=depths):
        c = _lib.ScuNETConfigC()
        for i, v in enumerate(d):
            c.depths[i] = v
        return c
    eng = shared_engine()
    assert L.sdmi_scunet_blob_floats(ctypes.byref(cfg_c())) == blob.size
    assert L.sdmi_scunet_blob_floats(ctypes.byref(cfg_c((1, 1, 1, 0, 1, 1, 1)))) == 0
    assert L.sdmi_scunet_blob_floats(None) == 0
    assert not L.sdmi_scunet_create(eng.handle, blob.ctypes.data, blob.size - 1, ctypes.byref(cfg_c()))
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_scunet_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c((1, 1, 1, 0, 1, 1, 1))))
    assert "depths[i] in 1..64" in _lib.last_error()
    assert not L.sdmi_scunet_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c((1, 1, 1, 1, 1, 2, 1))))      # a 128-wide net: another blob
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_scunet_create(eng.handle, None, blob.size, ctypes.byref(cfg_c())) and "null" in _lib.last_error()
    hd = L.sdmi_scunet_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c()))
    assert hd, _lib.last_error()
    try:
        assert L.sdmi_scunet_scratch_bytes(hd, 1, 70, 100) == L.sdmi_scunet_scratch_bytes(hd, 1, 128, 128) > 0
        assert L.sdmi_scunet_scratch_bytes(hd, 1, 24, 40) == L.sdmi_scunet_scratch_bytes(hd, 1, 64, 64) < L.sdmi_scunet_scratch_bytes(hd, 1, 65, 64)
        assert L.sdmi_scunet_scratch_bytes(hd, 1, 1, 1) == L.sdmi_scunet_scratch_bytes(hd, 1, 64, 64) > 0
        assert L.sdmi_scunet_scratch_bytes(hd, 1, 0, 13) == 0
        assert L.sdmi_scunet_scratch_bytes(hd, 1, 8192, 4096) == 0               # 2^25 pixels x 64 channels = 2^31 elements
        x, ref, twin = reference_for(SMALL)
        xd = x.to(dev)
        out = torch.full((1, 3, 24, 40), 7.0, dtype=torch.float32).to(dev)
        assert L.sdmi_scunet_run(hd, _lib.ptr(xd), 0, 1, 0, 40, _lib.ptr(out), 0, _lib.stream_ptr()) != 0 and "empty image" in _lib.last_error()
        assert L.sdmi_scunet_run(hd, _lib.ptr(xd), 0, 1, 8192, 4096, _lib.ptr(out), 0, _lib.stream_ptr()) != 0 and "2^31" in _lib.last_error()
        assert L.sdmi_scunet_run(hd, None, 0, 1, 24, 40, _lib.ptr(out), 0, _lib.stream_ptr()) != 0 and "null" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((out.cpu() == 7).all())
        _lib.check(L.sdmi_scunet_run(hd, _lib.ptr(xd), 0, 1, 24, 40, _lib.ptr(out), 0, _lib.stream_ptr()), "sdmi_scunet_run")
        assert_parity(out, ref, twin, 1, (0, 2), "direct handle, 24x40")
    finally:
        L.sdmi_scunet_destroy(hd)


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_scunet_checkpoint(dev, tmp_path):
    from PIL import Image
    up = sub("upscaler")
    sd, net = net_for(NET_CASES[SMALL][0])
    path = str(tmp_path / "tiny_scunet.pth")
    torch.save(sd, path)
    src = np.random.RandomState(5).randint(90, 166, size=(19, 13, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0, engine=shared_engine())
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (13, 19) and img.mode == "RGB"           # scale 1: the same size out
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.ScuNETNet)
    direct = net.run(torch.from_numpy(src[None]).to(dev))[0].cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(img), up.model_output_to_u8(direct))


def test_resize_image_through_a_registered_scunet_upscaler(dev, tmp_path, monkeypatch):
    """24 x 16 -> 48 x 32: the driver loop stops after ONE network pass (the scaler returned its input's size) and Lanczos fits the rest."""
    from PIL import Image
    up, shared = sub("upscaler"), sub("shared")
    sd = net_for(NET_CASES[SMALL][0])[0]
    path = str(tmp_path / "tiny_scunet.pth")
    torch.save({"params": sd}, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    added = up.register_esrgan({"Tiny-ScuNET": path}, engine=shared_engine())
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-ScuNET"] and added[0].scale == 1
    passes = []
    run = up.ScuNETNet.run
    monkeypatch.setattr(up.ScuNETNet, "run", lambda self, x, out_u8=False: passes.append(tuple(x.shape)) or run(self, x, out_u8))
    im = Image.fromarray(np.random.RandomState(6).randint(90, 166, size=(16, 24, 3), dtype=np.uint8))
    got = up.resize_image(0, im, 48, 32, "Tiny-ScuNET")
    assert got.size == (48, 32) and passes == [(1, 16, 24, 3)] and isinstance(added[0].scaler._nets[path], up.ScuNETNet)
    once = added[0].scaler.do_upscale(im, path)
    assert once.size == (24, 16)
    assert np.array_equal(np.asarray(got), np.asarray(once.resize((48, 32), resample=Image.LANCZOS)))
