"""GPU parity tests of the SwinIR path: the shifted-window attention kernel through sdmi_swin_attention against the float64 graph on
the same fp16 operands, swin_layernorm against float64, whole networks through sdmi_swinir_run against tests/swinir_reference.py (fp32,
CPU), UpscalerESRGAN.do_upscale on a SwinIR checkpoint and one resize through the registry.

Comparison rule: that of tests/test_gpu_esrgan.py / test_gpu_compact.py (`assert_parity`): the yardstick is the distance of the
fp16-storage twin from the reference; the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per
channel, per image row) within 2.5 x the yardstick, the yardstick itself is asserted above 1e-4 and the twin's own worst slice within
2.5 x of it (inputs on which the rule could not decide fail the test instead of passing it).  Every case also runs on the
host-emulated library (tests/test_cpu_swinir.py)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import swinir_reference as R
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
    print(f"[swinir parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
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


# ---- window attention -------------------------------------------------------------------------------------------------------------
ATTN = {}


def attn_case(b, h, w, heads, d, seed):
    """Seeded q, k, v [b, h, w, heads, d] (fp16 values) and a bias table [225, heads] of spread ~ 1; the float64 graph for shift 0 and 4
    is computed once per case and shared."""
    key = (b, h, w, heads, d, seed)
    if key not in ATTN:
        q, k, v = (r16(seeded((b, h, w, heads, d), seed + i)) for i in range(3))
        table = seeded((225, heads), seed + 3, 0.5)
        ATTN[key] = dict(q=q, k=k, v=v, table=table, graphs={})
    return ATTN[key]


def graph(case, shift, rnd=R.ident, mask=True, bias=True):
    """The float64 graph: roll, partition, softmax(q k^T d^-1/2 + bias + mask) v, merge, roll back -> [b, h, w, heads * d]."""
    key = (shift, rnd is R.ident, mask, bias)
    if key not in case["graphs"]:
        q, k, v = case["q"], case["k"], case["v"]
        b, h, w, heads, d = q.shape
        x = torch.cat([q.flatten(3), k.flatten(3), v.flatten(3)], dim=-1).double()
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        m = R.shift_mask(h, w, shift).double() if shift and mask else None
        a = R.window_attention(R.window_partition(x), case["table"].double(), heads, m, rnd, use_bias=bias)
        a = R.window_reverse(a, b, h, w)
        if shift:
            a = torch.roll(a, (shift, shift), (1, 2))
        case["graphs"][key] = a
    return case["graphs"][key]


def packed_qkv(case, ldq=None, poison=1e4):
    """[b, h, w, ldq] fp16: the 32-wide head slots (tails zero), `poison` past 96 heads."""
    q = case["q"]
    b, h, w, heads, d = q.shape
    ldq = ldq or 96 * heads
    out = torch.full((b, h, w, ldq), poison, dtype=torch.float32)
    out[..., :96 * heads] = 0
    for t, src in enumerate((case["q"], case["k"], case["v"])):
        for hd in range(heads):
            out[..., (t * heads + hd) * 32:(t * heads + hd) * 32 + d] = src[..., hd, :]
    return out.half()


def expanded_bias(case):
    heads = case["table"].shape[1]
    return case["table"][R.relative_position_index().view(-1)].view(64, 64, heads).permute(2, 0, 1).contiguous()


def unslot(out, heads, d):
    """[b, h, w, >= 32 heads] -> [b, h, w, heads * d], and the slot tails."""
    o = out[..., :32 * heads].reshape(*out.shape[:3], heads, 32)
    return o[..., :d].reshape(*out.shape[:3], heads * d), o[..., d:]


def run_attn(dev, case, shift, **kw):
    ops = sub("ops")
    b, h, w, heads, d = case["q"].shape
    return ops.swin_attention(packed_qkv(case, kw.pop("ldq", None)).to(dev), expanded_bias(case).to(dev), heads, d, shift=shift, **kw)


@pytest.mark.parametrize("b,h,w,heads,d,shift", [
    (2, 16, 24, 2, 30, 0), (2, 16, 24, 2, 30, 4),      # 2 x 3 windows: every region id occurs, no window is interior when shifted
    (1, 24, 40, 2, 30, 4),                             # interior windows with an all-zero mask
    (1, 8, 8, 2, 30, 4),                               # one window wrapped onto itself
    (1, 16, 16, 4, 32, 4),                             # no slot tail
    (1, 16, 16, 8, 30, 4), (1, 16, 16, 8, 30, 0),      # two heads per wave
    (1, 16, 16, 6, 30, 4)])                            # a wave without a head in the second pass
def test_window_attention_vs_float64_graph(dev, b, h, w, heads, d, shift):
    case = attn_case(b, h, w, heads, d, 1000 + 7 * heads + d + h)
    out = run_attn(dev, case, shift)
    assert out.shape == (b, h, w, 32 * heads) and out.dtype == torch.float16
    got, tails = unslot(out.cpu(), heads, d)
    assert bool((tails == 0).all())
    ref, twin = graph(case, shift), graph(case, shift, r16d)
    _, yard = assert_parity(got, ref, twin, 3, (0, 1), f"attention B{b} {h}x{w} heads {heads} D {d} shift {shift}")
    if shift:                                          # both additive terms are really applied
        assert rel_l2(got, graph(case, shift, mask=False)) > 10 * yard
        assert rel_l2(got, graph(case, shift, bias=False)) > 10 * yard
    else:
        assert rel_l2(got, graph(case, 0, bias=False)) > 10 * yard


def test_window_attention_in_rows_wider_than_the_slots(dev):
    """ldq = 96 heads + 8, ldo = 32 heads + 8, the out buffer pre-filled: the excess keeps its bits, the slot tails read zero, the result
    is bit-equal to the dense call."""
    case = attn_case(2, 16, 24, 2, 30, 1000 + 14 + 30 + 16)
    dense = run_attn(dev, case, 4)
    out = torch.full((2, 16, 24, 72), 3.0, dtype=torch.float16).to(dev)
    got = run_attn(dev, case, 4, ldq=200, out=out)
    assert got is out and bool((out.cpu()[..., 64:] == 3).all())
    assert same_bits(out[..., :64], dense)
    assert bool((unslot(out.cpu(), 2, 30)[1] == 0).all())


def test_window_attention_refuses_what_it_is_not_built_for(dev):
    """Every refusal returns non-zero with a message and writes nothing."""
    _lib = sub("_lib")
    qkv = torch.zeros((1, 16, 16, 200), dtype=torch.float16).to(dev)
    bias = torch.zeros((2, 64, 64), dtype=torch.float32).to(dev)
    out = torch.full((1, 16, 16, 72), 7.0, dtype=torch.float16).to(dev)

    def desc(**kw):
        d = _lib.SwinAttnDesc()
        d.qkv, d.bias, d.out = qkv.data_ptr(), bias.data_ptr(), out.data_ptr()
        d.B, d.H, d.W, d.heads, d.D, d.ldq, d.ldo, d.shift, d.scale = 1, 16, 16, 2, 30, 200, 72, 4, 30 ** -0.5
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert _lib.lib.sdmi_swin_attention(ctypes.byref(desc()), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = [(dict(qkv=None), "null"), (dict(bias=None), "null"), (dict(out=None), "null"),
           (dict(H=12), "multiples of the window size 8"), (dict(W=0), "multiples of the window size 8"), (dict(W=20), "multiples of the window size 8"),
           (dict(D=0), "1..32"), (dict(D=33), "1..32"), (dict(shift=2), "shift must be 0 or 4"), (dict(shift=-4), "shift must be 0 or 4"),
           (dict(ldq=184), "ldq >= 96 heads"), (dict(ldo=56), "ldo >= 32 heads"),
           (dict(qkv=qkv.data_ptr() + 2), "misaligned"), (dict(out=out.data_ptr() + 8), "misaligned"), (dict(bias=bias.data_ptr() + 4), "misaligned"),
           (dict(ldq=196), "misaligned"), (dict(ldo=68), "misaligned")]
    for kw, msg in bad:
        assert _lib.lib.sdmi_swin_attention(ctypes.byref(desc(**kw)), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.lib.sdmi_swin_attention(None, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def ln_ref(x, g, b, c):
    x = x[..., :c].double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g.double() + b.double()


@pytest.mark.parametrize("rows", [130, 1])
@pytest.mark.parametrize("c,ld", [(60, 64), (180, 192), (240, 256)])
def test_swin_layernorm_vs_float64(dev, c, ld, rows):
    ops = sub("ops")
    x = torch.full((rows, ld), 1e4, dtype=torch.float32)                 # the pad columns of the input are never read
    x[:, :c] = seeded((rows, c), 40 + c, 1.5) + seeded((rows, 1), 41 + c, 0.5)
    x = r16(x)
    g, b = 1.0 + seeded((c,), 42 + c, 0.2), seeded((c,), 43 + c, 0.2)
    out = torch.full((rows, ld), 3.0, dtype=torch.float16).to(dev)
    got = ops.swin_layernorm(x.half().to(dev), g.to(dev), b.to(dev), out=out)
    assert got is out
    assert bool((out.cpu()[:, c:] == 0).all())                           # C .. Cp - 1 (here = ld) are zeros in a pre-filled output
    ref = ln_ref(x, g, b, c)
    assert_parity(out.cpu()[:, :c], ref, r16d(ref), 1, (0,), f"layernorm C {c} ld {ld} rows {rows}")


def test_swin_layernorm_on_offset_heavy_rows(dev):
    """Row mean 50, spread 0.5: a variance taken as E[x^2] - mean^2 in fp32 would lose the spread; the centred form does not."""
    ops = sub("ops")
    c, ld, rows = 180, 192, 130
    x = torch.zeros((rows, ld))
    x[:, :c] = 50.0 + seeded((rows, c), 77, 0.5)
    x = r16(x)
    g, b = 1.0 + seeded((c,), 78, 0.2), seeded((c,), 79, 0.2)
    got = ops.swin_layernorm(x.half().to(dev), g.to(dev), b.to(dev))
    ref = ln_ref(x, g, b, c)
    assert_parity(got.cpu()[:, :c], ref, r16d(ref), 1, (0,), "layernorm, mean 50 spread 0.5")
    assert bool((got.cpu()[:, c:] == 0).all())


@pytest.mark.parametrize("c,ld,rows", [(500, 512, 37), (600, 640, 9)])
def test_swin_layernorm_on_wider_rows(dev, c, ld, rows):
    """Rows wider than the networks use: 500 of 512 columns (four passes of the 128-column stride, the last one ragged; 37 rows = nine
    workgroups and a ragged one) and 600 of 640."""
    ops = sub("ops")
    x = torch.full((rows, ld), 1e4, dtype=torch.float32)
    x[:, :c] = seeded((rows, c), 50 + c, 1.5) + seeded((rows, 1), 51 + c, 0.5)
    x = r16(x)
    g, b = 1.0 + seeded((c,), 52 + c, 0.2), seeded((c,), 53 + c, 0.2)
    out = torch.full((rows, ld), 3.0, dtype=torch.float16).to(dev)
    ops.swin_layernorm(x.half().to(dev), g.to(dev), b.to(dev), out=out)
    assert bool((out.cpu()[:, c:] == 0).all())
    ref = ln_ref(x, g, b, c)
    assert_parity(out.cpu()[:, :c], ref, r16d(ref), 1, (0,), f"layernorm C {c} ld {ld} rows {rows}")


def test_swin_layernorm_refuses_narrow_rows(dev):
    _lib = sub("_lib")
    x = torch.zeros((4, 64), dtype=torch.float16).to(dev)
    g = torch.ones(70, dtype=torch.float32).to(dev)
    out = torch.full((4, 64), 7.0, dtype=torch.float16).to(dev)
    L = _lib.lib
    assert L.sdmi_swin_layernorm(_lib.ptr(x), _lib.ptr(g), _lib.ptr(g), _lib.ptr(out), 4, 70, 64, 1e-5, _lib.stream_ptr()) != 0
    assert "rounded up to 64" in _lib.last_error()
    assert L.sdmi_swin_layernorm(None, _lib.ptr(g), _lib.ptr(g), _lib.ptr(out), 4, 60, 64, 1e-5, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- network level ----------------------------------------------------------------------------------------------------------------
NET_CASES = {                                       # name: (make_state_dict arguments, (b, h, w))
    "c60-3conv-x4": ((60, (2, 2), 2, "3conv", 4), (2, 16, 24)),
    "c60-1conv-x2-ragged": ((60, (2,), 2, "1conv", 2), (1, 19, 13)),          # reflect pad 5 / 3, crop
    "c60-1conv-x2-one-window": ((60, (2,), 2, "1conv", 2), (1, 8, 8)),
    "c240-3conv-x4": ((240, (2,), 8, "3conv", 4), (1, 16, 16)),               # 240 -> 256, 480 -> 512, 60 -> 64
    "c180-1conv-x4": ((180, (2,), 6, "1conv", 4), (1, 16, 16)),               # 180 -> 192, 360 -> 384
}
NETS, REFS, ENGINE = {}, {}, []


def shared_engine():
    if not ENGINE:
        ENGINE.append(sub("engine").Engine(0))
    return ENGINE[0]


def net_for(args):
    if args not in NETS:
        sd = R.make_state_dict(*args)
        NETS[args] = (sd, sub("upscaler").SwinIRNet(sd, device=0, engine=shared_engine()))
    return NETS[args]


def reference_for(name):
    """(x, fp32 reference, fp16-storage twin) of a case: computed once, shared, never modified."""
    if name not in REFS:
        args, (b, h, w) = NET_CASES[name]
        sd = R.make_state_dict(*args)
        x = R.image(b, h, w, 10 + args[4])
        REFS[name] = (x, R.forward(sd, x), R.fp16_twin(sd, x))
    return REFS[name]


@pytest.mark.parametrize("name", list(NET_CASES))
def test_swinir_network_vs_reference(dev, name):
    args, (b, h, w) = NET_CASES[name]
    sd, net = net_for(args)
    s = args[4]
    assert net.scale == s and net.config == R.config_of(sd)
    x, ref, twin = reference_for(name)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * s, w * s) and got.dtype == torch.float32
    assert 0 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    assert_parity(got, ref, twin, 1, (0, 2), f"network {name} {b}x{h}x{w}")


def test_swinir_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_swinir_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB)."""
    name = "c60-1conv-x2-one-window"
    args, (b, h, w) = NET_CASES[name]
    engine = sub("engine").Engine(0)
    net = sub("upscaler").SwinIRNet(R.make_state_dict(*args), device=0, engine=engine)
    assert engine.arena_bytes() == 0
    got = net.run(R.image(b, h, w, 10 + args[4]).to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, h * args[4], w * args[4]) and 0 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


def test_swinir_uint8_in_and_out(dev):
    """uint8 in is the same image: the same output; uint8 out is model_output_to_u8 of the same run's fp32 output, byte for byte."""
    up = sub("upscaler")
    args, (b, h, w) = NET_CASES["c60-1conv-x2-ragged"]
    sd, net = net_for(args)
    x = reference_for("c60-1conv-x2-ragged")[0]
    x8 = torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    f32 = net.run(x8)
    assert float((f32.cpu() - net.run(x.to(dev)).cpu()).abs().max()) < 1e-6
    u8 = net.run(x8, out_u8=True)
    assert u8.shape == (b, h * 2, w * 2, 3) and u8.dtype == torch.uint8
    assert np.array_equal(u8.cpu().numpy(), up.model_output_to_u8(f32.cpu().permute(0, 2, 3, 1).numpy()))


def test_swinir_handle_entries_directly(dev):
    """The C entries by name: blob_floats, create (and what it refuses), scratch_bytes, run (and a side of 7), destroy."""
    _lib, up = sub("_lib"), sub("upscaler")
    L = _lib.lib
    sd = R.make_state_dict(60, (2,), 2, "1conv", 2)
    blob, config = up.parse_swinir_state_dict(sd)

    def cfg_c(**kw):
        c = _lib.SwinIRConfigC()
        c.embed_dim, c.num_layers, c.num_heads, c.mlp_hidden, c.resi_3conv, c.scale = 60, 1, 2, 120, 0, 2
        c.depths[0] = 2
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    eng = shared_engine()
    assert L.sdmi_swinir_blob_floats(ctypes.byref(cfg_c())) == blob.size
    assert L.sdmi_swinir_blob_floats(ctypes.byref(cfg_c(num_heads=1))) == 0
    assert not L.sdmi_swinir_create(eng.handle, blob.ctypes.data, blob.size - 1, ctypes.byref(cfg_c()))
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_swinir_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c(num_heads=1)))
    assert "num_heads * 32 >= embed_dim" in _lib.last_error()
    assert not L.sdmi_swinir_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c(scale=3)))
    h = L.sdmi_swinir_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c()))
    assert h, _lib.last_error()
    try:
        assert L.sdmi_swinir_scratch_bytes(h, 1, 19, 13) > 0
        assert L.sdmi_swinir_scratch_bytes(h, 1, 7, 13) == 0
        x, ref, twin = reference_for("c60-1conv-x2-ragged")
        xd = x.to(dev)
        out = torch.full((1, 3, 38, 26), 7.0, dtype=torch.float32).to(dev)
        small = torch.zeros((1, 3, 7, 13), dtype=torch.float32).to(dev)
        assert L.sdmi_swinir_run(h, _lib.ptr(small), 0, 1, 7, 13, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        assert "at least 8" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((out.cpu() == 7).all())
        _lib.check(L.sdmi_swinir_run(h, _lib.ptr(xd), 0, 1, 19, 13, _lib.ptr(out), 0, _lib.stream_ptr()), "sdmi_swinir_run")
        assert_parity(out, ref, twin, 1, (0, 2), "direct handle, 19x13")
    finally:
        L.sdmi_swinir_destroy(h)


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_swinir_checkpoint(dev, tmp_path):
    from PIL import Image
    up = sub("upscaler")
    args = NET_CASES["c60-1conv-x2-ragged"][0]
    sd, net = net_for(args)
    path = str(tmp_path / "tiny_swinir_x2.pth")
    torch.save({"params_ema": sd}, path)
    src = np.random.RandomState(5).randint(90, 166, size=(19, 13, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0, engine=shared_engine())
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (26, 38) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.SwinIRNet)
    direct = net.run(torch.from_numpy(src[None]).to(dev))[0].cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(img), up.model_output_to_u8(direct))


def test_resize_image_through_a_registered_swinir_upscaler(dev, tmp_path, monkeypatch):
    from PIL import Image
    up, shared = sub("upscaler"), sub("shared")
    sd = net_for(NET_CASES["c60-1conv-x2-ragged"][0])[0]
    path = str(tmp_path / "tiny_swinir_x2.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    added = up.register_esrgan({"Tiny-SwinIR 2x": path}, engine=shared_engine())
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-SwinIR 2x"] and added[0].scale == 2
    im = Image.fromarray(np.random.RandomState(6).randint(90, 166, size=(16, 24, 3), dtype=np.uint8))
    got = up.resize_image(0, im, 48, 32, "Tiny-SwinIR 2x")
    assert got.size == (48, 32) and isinstance(added[0].scaler._nets[path], up.SwinIRNet)
    assert np.array_equal(np.asarray(got), np.asarray(added[0].scaler.do_upscale(im, path)))
