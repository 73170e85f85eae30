"""GPU parity tests of the Swin2SR path: the cosine window attention kernel through sdmi_swin2_attention against the float64 graph on the
same fp16 operands, swin_layernorm_add against float64, whole networks (every upsampler) through sdmi_swin2sr_run against
tests/swin2sr_reference.py (fp32, CPU), UpscalerESRGAN.do_upscale on a Swin2SR checkpoint and one resize through the registry.

Comparison rule: `assert_parity` of tests/test_gpu_swinir.py — the yardstick is the distance of the fp16-storage twin from the reference;
the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per channel, per image row) within 2.5 x the
yardstick, the yardstick itself is asserted above 1e-4 and the twin's own worst slice within 2.5 x of it.  Every case also runs on the
host-emulated library (tests/test_cpu_swin2sr.py)."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import swin2sr_reference as R
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
    print(f"[swin2sr parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
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


# ---- cosine window attention --------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [
    (2, 16, 24, 2, 30, 0), (2, 16, 24, 2, 30, 4),      # 2 x 3 windows: every region id occurs
    (1, 8, 8, 2, 30, 4),                               # one window wrapped onto itself
    (1, 16, 16, 4, 32, 4),                             # no slot tail
    (1, 16, 16, 6, 30, 4),                             # a wave without a head in the second pass
    (1, 16, 16, 8, 10, 4),                             # two heads per wave, the lightweight models' head dim
    (1, 16, 16, 5, 12, 0)]
ATTN = {}


def attn_seed(b, h, w, heads, d):
    return 2000 + 7 * heads + d + h


def attn_case(b, h, w, heads, d, seed):
    """Seeded q, k, v [b, h, w, heads, d] (fp16 values), a bias table 16 sigmoid(N(0, 1.5^2)) [225, heads] and head scales
    exp(U(ln 3, ln 100)) (the clamp is the loader's); the float64 graphs are computed once per case and shared."""
    key = (b, h, w, heads, d, seed)
    if key not in ATTN:
        q, k, v = (r16(seeded((b, h, w, heads, d), seed + i)) for i in range(3))
        table = 16 * torch.sigmoid(seeded((225, heads), seed + 3, 1.5))
        u = torch.rand((heads,), generator=torch.Generator().manual_seed(seed + 4))
        scale = torch.exp(math.log(3.0) + (math.log(100.0) - math.log(3.0)) * u)
        ATTN[key] = dict(q=q, k=k, v=v, table=table, scale=scale, graphs={})
    return ATTN[key]


def graph(case, shift, rnd=R.ident, mask=True, bias=True, scale=True, mask_value=-100.0):
    """The float64 graph: roll, partition, softmax(cos(q, k) tau + bias + mask) v, merge, roll back -> [b, h, w, heads * d]."""
    key = (shift, rnd is R.ident, mask, bias, scale, mask_value)
    if key not in case["graphs"]:
        q, k, v = case["q"], case["k"], case["v"]
        b, h, w, heads, d = q.shape
        x = torch.cat([q.flatten(3), k.flatten(3), v.flatten(3)], dim=-1).double()
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        m = None
        if shift and mask:
            m = R.shift_mask(h, w, shift).double()
            m = torch.where(m != 0, torch.tensor(mask_value, dtype=torch.float64), m)
        a = R.cosine_window_attention(R.window_partition(x), case["table"].double(), case["scale"].double(), heads, m, rnd, use_bias=bias,
                                      use_scale=scale)
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
    return ops.swin2_attention(packed_qkv(case, kw.pop("ldq", None)).to(dev), expanded_bias(case).to(dev), case["scale"].to(dev), heads, d,
                               shift=shift, **kw)


@pytest.mark.parametrize("b,h,w,heads,d,shift", ATTN_SHAPES)
def test_cosine_attention_vs_float64_graph(dev, b, h, w, heads, d, shift):
    case = attn_case(b, h, w, heads, d, attn_seed(b, h, w, heads, d))
    out = run_attn(dev, case, shift)
    assert out.shape == (b, h, w, 32 * heads) and out.dtype == torch.float16
    got, tails = unslot(out.cpu(), heads, d)
    assert bool((tails == 0).all())
    ref, twin = graph(case, shift), graph(case, shift, r16d)
    _, yard = assert_parity(got, ref, twin, 3, (0, 1), f"attention B{b} {h}x{w} heads {heads} D {d} shift {shift}")
    # bias, mask and head_scale are really applied
    assert rel_l2(got, graph(case, shift, bias=False)) > 10 * yard
    assert rel_l2(got, graph(case, shift, scale=False)) > 10 * yard
    if shift:
        assert rel_l2(got, graph(case, shift, mask=False)) > 10 * yard


def test_cosine_attention_with_zero_q_and_zero_k_tokens(dev):
    """A token whose q slot is all zero and one whose k slot is all zero (every head): their scores are bias + mask alone, as
    F.normalize's eps gives them in the graph; nothing is NaN."""
    base = attn_case(2, 16, 24, 2, 30, attn_seed(2, 16, 24, 2, 30))
    case = dict(base, q=base["q"].clone(), k=base["k"].clone(), graphs={})
    case["q"][0, 3, 5] = 0
    case["q"][1, 12, 20] = 0
    case["k"][0, 9, 2] = 0
    case["k"][1, 12, 20] = 0                                      # both at one token
    out = run_attn(dev, case, 4).cpu()
    assert bool(torch.isfinite(out.float()).all())
    got, _ = unslot(out, 2, 30)
    assert_parity(got, graph(case, 4), graph(case, 4, r16d), 3, (0, 1), "attention with zero q / zero k tokens")


def crafted_mask_case():
    """head_scale 100, shift 4, q = u everywhere, k = +u in the regions of even id and -u in the odd ones (on the shifted grid): a query
    of an odd region sees its own region at -100 + bias and the MASKED even regions at +100 - 100 + bias, so its output comes from masked
    keys — with a -inf mask it would come from its own region."""
    key = "crafted"
    if key not in ATTN:
        b, h, w, heads, d = 1, 16, 16, 2, 30
        u = r16(seeded((heads, d), 77))
        ids = R.region_ids(h, w, 4)                                # the shifted grid
        sign = torch.where(ids.long() % 2 == 0, 1.0, -1.0)
        k_shifted = sign[None, :, :, None, None] * u[None, None, None]
        ATTN[key] = dict(q=u[None, None, None].expand(b, h, w, heads, d).contiguous(), k=torch.roll(k_shifted, (4, 4), (1, 2)).contiguous(),
                         v=r16(seeded((b, h, w, heads, d), 78)), table=16 * torch.sigmoid(seeded((225, heads), 79, 1.5)),
                         scale=torch.full((heads,), 100.0), graphs={})
    return ATTN[key]


def test_the_mask_is_minus_100_not_minus_infinity(dev):
    case = crafted_mask_case()
    ref, twin = graph(case, 4), graph(case, 4, r16d)
    yard = rel_l2(twin, ref)
    assert rel_l2(graph(case, 4, mask_value=-math.inf), ref) > 10 * yard        # the two masks differ on this input (on the CPU)
    got, _ = unslot(run_attn(dev, case, 4).cpu(), 2, 30)
    assert_parity(got, ref, twin, 3, (0, 1), "attention, crafted -100 mask case")


def test_cosine_attention_in_rows_wider_than_the_slots(dev):
    """ldq = 96 heads + 8, ldo = 32 heads + 8, the out buffer pre-filled: the excess keeps its bits, the result is bit-equal to the
    dense call."""
    case = attn_case(2, 16, 24, 2, 30, attn_seed(2, 16, 24, 2, 30))
    dense = run_attn(dev, case, 4)
    out = torch.full((2, 16, 24, 72), 3.0, dtype=torch.float16).to(dev)
    got = run_attn(dev, case, 4, ldq=200, out=out)
    assert got is out and bool((out.cpu()[..., 64:] == 3).all())
    assert same_bits(out[..., :64], dense)
    assert bool((unslot(out.cpu(), 2, 30)[1] == 0).all())


def test_cosine_attention_refuses_what_it_is_not_built_for(dev):
    """Every refusal returns non-zero with a message and writes nothing."""
    _lib = sub("_lib")
    qkv = torch.zeros((1, 16, 16, 200), dtype=torch.float16).to(dev)
    bias = torch.zeros((2, 64, 64), dtype=torch.float32).to(dev)
    hs = torch.ones((4,), dtype=torch.float32).to(dev)
    out = torch.full((1, 16, 16, 72), 7.0, dtype=torch.float16).to(dev)

    def desc(**kw):
        d = _lib.Swin2AttnDesc()
        d.qkv, d.bias, d.out, d.head_scale = qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), hs.data_ptr()
        d.B, d.H, d.W, d.heads, d.D, d.ldq, d.ldo, d.shift = 1, 16, 16, 2, 30, 200, 72, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert _lib.lib.sdmi_swin2_attention(ctypes.byref(desc()), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = [(dict(qkv=None), "null"), (dict(bias=None), "null"), (dict(out=None), "null"), (dict(head_scale=None), "null"),
           (dict(H=12), "multiples of the window size 8"), (dict(W=0), "multiples of the window size 8"), (dict(W=20), "multiples of the window size 8"),
           (dict(D=0), "1..32"), (dict(D=33), "1..32"), (dict(shift=2), "shift must be 0 or 4"), (dict(shift=-4), "shift must be 0 or 4"),
           (dict(ldq=184), "ldq >= 96 heads"), (dict(ldo=56), "ldo >= 32 heads"),
           (dict(qkv=qkv.data_ptr() + 2), "misaligned"), (dict(out=out.data_ptr() + 8), "misaligned"), (dict(bias=bias.data_ptr() + 4), "misaligned"),
           (dict(head_scale=hs.data_ptr() + 2), "misaligned"), (dict(ldq=196), "misaligned"), (dict(ldo=68), "misaligned")]
    for kw, msg in bad:
        assert _lib.lib.sdmi_swin2_attention(ctypes.byref(desc(**kw)), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.lib.sdmi_swin2_attention(None, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- res-post-norm LayerNorm ---------------------------------------------------------------------------------------------------------
def lnadd_ref(y, resid, g, b, c):
    y = y[..., :c].double()
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    return resid[..., :c].double() + (y - mu) / torch.sqrt(var + 1e-5) * g.double() + b.double()


def lnadd_inputs(rows, c, ld, seed, mean=None):
    y = torch.full((rows, ld), 1e4, dtype=torch.float32)                 # the pad columns of the inputs are never read
    y[:, :c] = (seeded((rows, c), seed, 1.5) + seeded((rows, 1), seed + 1, 0.5)) if mean is None else mean + seeded((rows, c), seed, 0.5)
    resid = torch.full((rows, ld), -1e4, dtype=torch.float32)
    resid[:, :c] = seeded((rows, c), seed + 2, 1.0)
    g, b = 0.5 + seeded((c,), seed + 3, 0.1), seeded((c,), seed + 4, 0.1)
    return r16(y), r16(resid), g, b


@pytest.mark.parametrize("rows", [130, 1])
@pytest.mark.parametrize("c,ld", [(60, 64), (180, 192), (240, 256)])
def test_swin_layernorm_add_vs_float64(dev, c, ld, rows):
    ops = sub("ops")
    y, resid, g, b = lnadd_inputs(rows, c, ld, 140 + c)
    out = torch.full((rows, ld), 3.0, dtype=torch.float16).to(dev)
    got = ops.swin_layernorm_add(y.half().to(dev), g.to(dev), b.to(dev), resid.half().to(dev), out=out)
    assert got is out
    assert bool((out.cpu()[:, c:] == 0).all())                           # C .. Cp - 1 (here = ld) are zeros in a pre-filled output
    ref = lnadd_ref(y, resid, g, b, c)
    assert_parity(out.cpu()[:, :c], ref, r16d(ref), 1, (0,), f"layernorm_add C {c} ld {ld} rows {rows}")


def test_swin_layernorm_add_in_place_and_on_offset_heavy_rows(dev):
    """out == resid: bit-equal to the out-of-place call.  y with row mean 50, spread 0.5: a variance taken as E[x^2] - mean^2 in fp32
    would lose the spread."""
    ops = sub("ops")
    c, ld, rows = 180, 192, 130
    y, resid, g, b = lnadd_inputs(rows, c, ld, 177, mean=50.0)
    yd, rd = y.half().to(dev), resid.half().to(dev)
    apart = ops.swin_layernorm_add(yd, g.to(dev), b.to(dev), rd)
    ref = lnadd_ref(y, resid, g, b, c)
    assert_parity(apart.cpu()[:, :c], ref, r16d(ref), 1, (0,), "layernorm_add, y mean 50 spread 0.5")
    assert bool((apart.cpu()[:, c:] == 0).all())
    stream = rd.clone()
    assert ops.swin_layernorm_add(yd, g.to(dev), b.to(dev), stream, out=stream) is stream
    assert same_bits(stream, apart)


def test_swin_layernorm_add_refusals(dev):
    _lib = sub("_lib")
    x = torch.zeros((4, 64), dtype=torch.float16).to(dev)
    g = torch.ones(70, dtype=torch.float32).to(dev)
    out = torch.full((4, 64), 7.0, dtype=torch.float16).to(dev)
    L, p, s = _lib.lib, _lib.ptr, _lib.stream_ptr()
    assert L.sdmi_swin_layernorm_add(p(x), p(g), p(g), p(x), p(out), 4, 70, 64, 1e-5, s) != 0
    assert "rounded up to 64" in _lib.last_error()
    assert L.sdmi_swin_layernorm_add(None, p(g), p(g), p(x), p(out), 4, 60, 64, 1e-5, s) != 0
    assert L.sdmi_swin_layernorm_add(p(x), p(g), p(g), None, p(out), 4, 60, 64, 1e-5, s) != 0
    assert L.sdmi_swin_layernorm_add(p(out), p(g), p(g), p(x), p(out), 4, 60, 64, 1e-5, s) != 0
    assert "must not be the output" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- network level ----------------------------------------------------------------------------------------------------------------
T60 = (60, (2, 2), 6, "1conv")                      # the tiny net: embed 60, heads 6 (head dim 10), depths (2, 2), hidden 120
NET_CASES = {                                       # name: (make_state_dict arguments, keywords, (b, h, w))
    "nearest-x4": (T60 + (4, "nearest+conv"), {}, (1, 20, 27)),                 # reflect pad 4 / 5, crop
    "pixelshuffle-x2": (T60 + (2, "pixelshuffle"), {}, (2, 16, 24)),
    "pixelshuffle-x3": (T60 + (3, "pixelshuffle"), {}, (1, 20, 27)),
    "pixelshuffle-x4": (T60 + (4, "pixelshuffle"), {}, (2, 16, 24)),
    "direct-x2": (T60 + (2, "pixelshuffledirect"), {}, (1, 20, 27)),
    "direct-x3": (T60 + (3, "pixelshuffledirect"), {}, (2, 16, 24)),
    "direct-x4-no-proj": (T60 + (4, "pixelshuffledirect"), {"proj": False}, (1, 20, 27)),      # a state dict without patch_embed.proj keys
    "3conv-pixelshuffle-x2": ((60, (2, 2), 6, "3conv", 2, "pixelshuffle"), {}, (1, 20, 27)),
    "c180-nearest-x4": ((180, (2,), 6, "1conv", 4, "nearest+conv"), {}, (2, 16, 24)),          # 180 -> 192, 360 -> 384, head dim 30
}
NETS, REFS, ENGINE = {}, {}, []


def shared_engine():
    if not ENGINE:
        ENGINE.append(sub("engine").Engine(0))
    return ENGINE[0]


def state_dict_for(name):
    args, kw, _ = NET_CASES[name]
    return R.make_state_dict(*args, **kw)


def net_for(name):
    if name not in NETS:
        sd = state_dict_for(name)
        NETS[name] = (sd, sub("upscaler").Swin2SRNet(sd, device=0, engine=shared_engine()))
    return NETS[name]


def reference_for(name):
    """(x, fp32 reference, fp16-storage twin) of a case: computed once, shared, never modified."""
    if name not in REFS:
        args, kw, (b, h, w) = NET_CASES[name]
        sd = state_dict_for(name)
        x = R.image(b, h, w, 20 + args[4])
        REFS[name] = (x, R.forward(sd, x), R.fp16_twin(sd, x))
    return REFS[name]


@pytest.mark.parametrize("name", list(NET_CASES))
def test_swin2sr_network_vs_reference(dev, name):
    args, kw, (b, h, w) = NET_CASES[name]
    sd, net = net_for(name)
    s = args[4]
    assert net.scale == s and net.config == R.config_of(sd) and net.config["upsampler"] == args[5]
    x, ref, twin = reference_for(name)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * s, w * s) and got.dtype == torch.float32
    assert 0 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    assert_parity(got, ref, twin, 1, (0, 2), f"network {name} {b}x{h}x{w}")


def test_swin2sr_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_swin2sr_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB)."""
    name = "direct-x2"
    args, kw, (b, h, w) = NET_CASES[name]
    engine = sub("engine").Engine(0)
    net = sub("upscaler").Swin2SRNet(state_dict_for(name), device=0, engine=engine)
    assert engine.arena_bytes() == 0
    got = net.run(R.image(b, h, w, 20 + args[4]).to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, h * args[4], w * args[4]) and 0 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


def twin_flip_share(name):
    """The share of output bytes on which the fp16-storage twin and the fp32 reference round to different uint8 values: what fp16
    storage alone moves across a rounding boundary."""
    to_u8 = sub("upscaler").model_output_to_u8
    _, ref, twin = reference_for(name)
    return float((to_u8(ref.numpy()) != to_u8(twin.numpy())).mean())


@pytest.mark.parametrize("name", ["nearest-x4", "direct-x2", "pixelshuffle-x3"])
def test_swin2sr_uint8_in_and_out(dev, name):
    """uint8 in is the same image: the same output.  uint8 out against model_output_to_u8 of the fp32 run: never more than 1 apart, and
    apart on no larger a share of the bytes than the reference twin itself flips (a few per cent on these inputs; printed)."""
    up = sub("upscaler")
    args, kw, (b, h, w) = NET_CASES[name]
    s = args[4]
    sd, net = net_for(name)
    x = reference_for(name)[0]
    x8 = torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    f32 = net.run(x8)
    assert float((f32.cpu() - net.run(x.to(dev)).cpu()).abs().max()) < 1e-6
    u8 = net.run(x8, out_u8=True)
    assert u8.shape == (b, h * s, w * s, 3) and u8.dtype == torch.uint8
    want = up.model_output_to_u8(f32.cpu().permute(0, 2, 3, 1).numpy())
    diff = np.abs(u8.cpu().numpy().astype(np.int16) - want.astype(np.int16))
    share, allowed = float((diff != 0).mean()), twin_flip_share(name)
    print(f"[swin2sr parity] uint8 {name}: bytes apart {share:.4f}, the twin flips {allowed:.4f}")
    assert int(diff.max()) <= 1 and share <= allowed and allowed < 0.1


def config_c(sd):
    _lib, up = sub("_lib"), sub("upscaler")
    cfg = R.config_of(sd)
    c = _lib.Swin2SRConfigC()
    c.embed_dim, c.num_layers, c.num_heads, c.mlp_hidden = cfg["embed_dim"], len(cfg["depths"]), cfg["num_heads"], cfg["mlp_hidden"]
    c.resi_3conv, c.upsampler, c.scale = cfg["resi_3conv"], up.SWIN2SR_UPSAMPLERS.index(cfg["upsampler"]), cfg["scale"]
    for i, d in enumerate(cfg["depths"]):
        c.depths[i] = d
    return c


def test_swin2sr_handle_entries_directly(dev):
    """The C entries by name: blob_floats, create (and what it refuses), scratch_bytes, run (and a side of 7), destroy."""
    _lib, up = sub("_lib"), sub("upscaler")
    L = _lib.lib
    name = "direct-x2"
    sd = state_dict_for(name)
    blob, config = up.parse_swin2sr_state_dict(sd)

    def cfg_c(**kw):
        c = config_c(sd)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    eng = shared_engine()
    assert L.sdmi_swin2sr_blob_floats(ctypes.byref(cfg_c())) == blob.size
    for other in NET_CASES:                                   # every tail's blob length
        sd2 = state_dict_for(other)
        assert L.sdmi_swin2sr_blob_floats(ctypes.byref(config_c(sd2))) == up.parse_swin2sr_state_dict(sd2)[0].size, other
    refused = [(dict(num_heads=1), "num_heads * 32 >= embed_dim"), (dict(upsampler=3), "upsampler 0"), (dict(upsampler=-1), "upsampler 0"),
               (dict(scale=5), "scale 4 with the nearest+conv"), (dict(scale=1), "scale 4 with the nearest+conv"),
               (dict(upsampler=0, scale=2), "scale 4 with the nearest+conv"), (dict(num_layers=17), "num_layers"), (dict(embed_dim=61), "multiple of num_heads")]
    for kw, msg in refused:
        assert L.sdmi_swin2sr_blob_floats(ctypes.byref(cfg_c(**kw))) == 0, kw
        assert not L.sdmi_swin2sr_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c(**kw))), kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert not L.sdmi_swin2sr_create(eng.handle, blob.ctypes.data, blob.size - 1, ctypes.byref(cfg_c()))
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_swin2sr_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c(scale=3)))      # another tail: another length
    assert "blob size" in _lib.last_error()
    h = L.sdmi_swin2sr_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(cfg_c()))
    assert h, _lib.last_error()
    try:
        assert L.sdmi_swin2sr_scratch_bytes(h, 1, 20, 27) > 0
        assert L.sdmi_swin2sr_scratch_bytes(h, 1, 7, 13) == 0
        assert L.sdmi_swin2sr_scratch_bytes(None, 1, 20, 27) == 0
        x, ref, twin = reference_for(name)
        xd = x.to(dev)
        out = torch.full((1, 3, 40, 54), 7.0, dtype=torch.float32).to(dev)
        small = torch.zeros((1, 3, 7, 13), dtype=torch.float32).to(dev)
        assert L.sdmi_swin2sr_run(h, _lib.ptr(small), 0, 1, 7, 13, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        assert "at least 8" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((out.cpu() == 7).all())
        _lib.check(L.sdmi_swin2sr_run(h, _lib.ptr(xd), 0, 1, 20, 27, _lib.ptr(out), 0, _lib.stream_ptr()), "sdmi_swin2sr_run")
        assert_parity(out, ref, twin, 1, (0, 2), "direct handle, 20x27")
    finally:
        L.sdmi_swin2sr_destroy(h)


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_swin2sr_checkpoint(dev, tmp_path):
    from PIL import Image
    up = sub("upscaler")
    sd, net = net_for("pixelshuffle-x2")
    path = str(tmp_path / "tiny_swin2sr_x2.pth")
    torch.save({"params_ema": sd}, path)
    src = np.random.RandomState(5).randint(90, 166, size=(19, 13, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0, engine=shared_engine())
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (26, 38) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.Swin2SRNet)
    direct = net.run(torch.from_numpy(src[None]).to(dev))[0].cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(img), up.model_output_to_u8(direct))


def test_resize_image_through_a_registered_swin2sr_upscaler(dev, tmp_path, monkeypatch):
    from PIL import Image
    up, shared = sub("upscaler"), sub("shared")
    sd = net_for("direct-x2")[0]
    path = str(tmp_path / "tiny_swin2sr_lightweight_x2.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    added = up.register_esrgan({"Tiny-Swin2SR 2x": path}, engine=shared_engine())
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-Swin2SR 2x"] and added[0].scale == 2
    im = Image.fromarray(np.random.RandomState(6).randint(90, 166, size=(16, 24, 3), dtype=np.uint8))
    got = up.resize_image(0, im, 48, 32, "Tiny-Swin2SR 2x")
    assert got.size == (48, 32) and isinstance(added[0].scaler._nets[path], up.Swin2SRNet)
    assert np.array_equal(np.asarray(got), np.asarray(added[0].scaler.do_upscale(im, path)))
