"""GPU parity tests of the DAT path: the window attention kernel through sdmi_dat_window_attention against a float64 graph written
independently of tests/dat_reference.py (explicit window gathers, a dense bias from the index formula), the channel attention's two
launches, the depthwise conv, the pooled gate and the AIM combine against float64, whole networks through sdmi_dat_run against
tests/dat_reference.py (fp32, CPU), the handle entries, UpscalerESRGAN.do_upscale on a DAT checkpoint and one resize through the registry.

Comparison rule: `assert_parity` of tests/test_gpu_swinir.py, restated — the yardstick is the distance of the fp16-storage twin from the
reference; the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per channel, per image row) within
2.5 x the yardstick, the yardstick itself is asserted above 1e-4 and the twin's own worst slice within 2.5 x of it.  The pooled gate is
fp32 in memory (no fp16 storage, so no yardstick): its bound 1e-5 is fp32's — sums of at most a few hundred terms in a fixed order
(relative error below 1e-6) through exp with a relative error of a few 1e-7.  Every case also runs on the host-emulated library
(tests/test_cpu_dat.py)."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dat_reference as R
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
    print(f"[dat parity] {ctx}: engine {err:.3e}  fp16-storage twin {yard:.3e}")
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


def ident(t):
    return t


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def rup(v, m):
    return (v + m - 1) // m * m


def to_slots(x, heads, d, ld=None, poison=0.0):
    """[..., heads * d] -> fp16 [..., ld] in 32-wide head slots (tails zero, `poison` past 32 heads)."""
    ld = ld or 32 * heads
    out = torch.full((*x.shape[:-1], ld), poison, dtype=torch.float32)
    out[..., :32 * heads] = 0
    out[..., :32 * heads].view(*x.shape[:-1], heads, 32)[..., :d] = x.reshape(*x.shape[:-1], heads, d).float()
    return out.half()


def from_slots(x, heads, d):
    """-> ([..., heads * d], the slot tails)."""
    o = x[..., :32 * heads].reshape(*x.shape[:-1], heads, 32)
    return o[..., :d].reshape(*x.shape[:-1], heads * d), o[..., d:]


# ---- window attention ---------------------------------------------------------------------------------------------------------------
WIN_CASES = [(1, 32, 32, 6, 30, (8, 32), False),            # one window per branch
             (2, 40, 72, 6, 30, (8, 32), True),             # padding and shift
             (1, 16, 16, 2, 32, (8, 16), True),             # one head per branch
             (1, 24, 40, 6, 10, (8, 16), True),
             (1, 33, 47, 4, 16, (8, 32), True)]             # odd sides
WIN = {}


def win_case(b, h, w, heads, d, split):
    """Seeded q, k, v [b, h, w, heads, d] (fp16 values) and the two bias tables N(0, 1.5^2); the float64 graphs are computed once per
    case and shared."""
    key = (b, h, w, heads, d, split)
    if key not in WIN:
        seed = 3000 + 7 * heads + d + h + split[1]
        q, k, v = (r16(seeded((b, h, w, heads, d), seed + i)) for i in range(3))
        n = (2 * split[0] - 1) * (2 * split[1] - 1)
        WIN[key] = dict(q=q, k=k, v=v, split=split, tables=(seeded((n, heads // 2), seed + 3, 1.5), seeded((n, heads // 2), seed + 4, 1.5)), graphs={})
    return WIN[key]


def region(u, n, s):
    return torch.where(u < n - s, 0, torch.where(u < n - s // 2, 1, 2))


def win_graph(case, shifted, rnd=ident, bias=True, mask=True, mask_value=-100.0, mask_padded_keys=False):
    """The float64 graph, window by window: gather the window's tokens off the zero-padded grid at their rolled positions, the dense
    bias from the index formula, the region mask from the shifted positions, softmax, P V, scatter back to the tokens inside the image."""
    key = (shifted, rnd is ident, bias, mask, mask_value, mask_padded_keys)
    if key in case["graphs"]:
        return case["graphs"][key]
    q, k, v = (case[n].double() for n in "qkv")
    b, h, w, heads, d = q.shape
    s0, s1 = case["split"]
    hp, wp, hh = rup(h, s1), rup(w, s1), heads // 2
    out = torch.zeros((b, h, w, heads, d), dtype=torch.float64)
    for br, (hs, ws) in enumerate(((s0, s1), (s1, s0))):
        table = case["tables"][br].double()
        pad = [torch.zeros((b, hp, wp, hh, d), dtype=torch.float64) for _ in range(3)]
        for dst, src in zip(pad, (q, k, v)):
            dst[:, :h, :w] = src[:, :, :, br * hh:(br + 1) * hh]
        shy, shx = (hs // 2, ws // 2) if shifted else (0, 0)
        ay, ax = torch.arange(hs * ws) // ws, torch.arange(hs * ws) % ws
        index = (ay[:, None] - ay[None, :] + hs - 1) * (2 * ws - 1) + (ax[:, None] - ax[None, :] + ws - 1)
        dense = table[index.view(-1)].view(hs * ws, hs * ws, hh).permute(2, 0, 1)                     # [hh, query, key]
        for wy in range(hp // hs):
            for wx in range(wp // ws):
                ys, xs = wy * hs + ay, wx * ws + ax                                                  # the shifted grid
                yy, xx = (ys + shy) % hp, (xs + shx) % wp                                            # the padded grid
                qw, kw, vw = (t[:, yy, xx] for t in pad)                                             # [b, N, hh, d]
                score = torch.einsum("bnhd,bmhd->bhnm", qw * d ** -0.5, kw)
                if bias:
                    score = score + dense[None]
                if shifted and mask:
                    ids = 3 * region(ys, hp, hs) + region(xs, wp, ws)
                    score = score + torch.where(ids[:, None] != ids[None, :], mask_value, 0.0).double()[None, None]
                inside = (yy < h) & (xx < w)
                if mask_padded_keys:
                    score = score.masked_fill(~inside[None, None, None, :], -math.inf)
                p = rnd(torch.softmax(score, dim=-1))
                o = rnd(torch.einsum("bhnm,bmhd->bnhd", p, vw))
                out[:, yy[inside], xx[inside], br * hh:(br + 1) * hh] = o[:, inside]
    case["graphs"][key] = out.flatten(3)
    return case["graphs"][key]


def win_desc(dev, case, shifted, ldq=None, out_tensor=None, fields=None):
    """-> (descriptor, the tensors it points at)."""
    _lib = sub("_lib")
    b, h, w, heads, d = case["q"].shape
    s0, s1 = case["split"]
    ldq = ldq or 96 * heads
    qkv = torch.full((b, h, w, ldq), 1e4, dtype=torch.float16)
    qkv[..., :96 * heads] = torch.cat([to_slots(case[n].flatten(3), heads, d) for n in "qkv"], dim=-1)
    hold = [qkv.to(dev), case["tables"][0].float().contiguous().to(dev), case["tables"][1].float().contiguous().to(dev),
            out_tensor if out_tensor is not None else torch.empty((b, h, w, 32 * heads), dtype=torch.float16, device=dev)]
    desc = _lib.DatAttnDesc()
    desc.qkv, desc.bias0, desc.bias1, desc.out = (t.data_ptr() for t in hold)
    desc.B, desc.H, desc.W, desc.heads, desc.D, desc.ldq, desc.ldo = b, h, w, heads, d, ldq, hold[3].shape[3]
    desc.s0, desc.s1, desc.shift_h, desc.shift_w, desc.scale = s0, s1, (s0 // 2 if shifted else 0), (s1 // 2 if shifted else 0), d ** -0.5
    for k, v in (fields or {}).items():
        setattr(desc, k, v)
    return desc, hold


def run_win(dev, case, shifted, **kw):
    _lib = sub("_lib")
    desc, hold = win_desc(dev, case, shifted, **kw)
    _lib.check(_lib.lib.sdmi_dat_window_attention(ctypes.byref(desc), _lib.stream_ptr()), "sdmi_dat_window_attention")
    torch.cuda.synchronize()
    return hold[3]


@pytest.mark.parametrize("b,h,w,heads,d,split,shifted", WIN_CASES)
def test_window_attention_vs_float64_graph(dev, b, h, w, heads, d, split, shifted):
    case = win_case(b, h, w, heads, d, split)
    out = run_win(dev, case, shifted)
    assert out.shape == (b, h, w, 32 * heads) and out.dtype == torch.float16
    got, tails = from_slots(out.cpu(), heads, d)
    assert bool((tails == 0).all())
    ref, twin = win_graph(case, shifted), win_graph(case, shifted, r16d)
    _, yard = assert_parity(got, ref, twin, 3, (0, 1), f"window attention B{b} {h}x{w} heads {heads} D {d} split {split} shifted {shifted}")
    assert rel_l2(got, win_graph(case, shifted, bias=False)) > 10 * yard                 # the bias is really applied
    if shifted:
        assert rel_l2(got, win_graph(case, shifted, mask=False)) > 10 * yard             # ... and the mask
    if h % split[1] or w % split[1]:                                                     # padded tokens are keys (score 0 + bias)
        assert rel_l2(got, win_graph(case, shifted, mask_padded_keys=True)) > 10 * yard


def crafted_mask_case():
    """Shifted, q = u everywhere with |u|^2 D^-1/2 = 80, k = +u in the regions of even id and -u in the odd ones (on each branch's own
    shifted grid): a query of an odd region sees its own region at -80 + bias and the MASKED even regions at +80 - 100 + bias, so its
    output comes from masked keys — with a -inf mask it would come from its own region."""
    if "crafted" not in WIN:
        b, h, w, heads, d, split = 1, 16, 16, 2, 32, (8, 16)
        u = seeded((heads, d), 77)
        u = r16(u * torch.sqrt(80.0 * math.sqrt(d) / (u * u).sum(-1, keepdim=True)))
        k = torch.zeros((b, h, w, heads, d))
        for hd, (hs, ws) in enumerate((split, split[::-1])):                             # head 0 is branch 0, head 1 branch 1
            ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
            sign = torch.where((3 * region(ys, h, hs) + region(xs, w, ws)) % 2 == 0, 1.0, -1.0)
            k[0, :, :, hd] = torch.roll(sign[:, :, None] * u[hd][None, None], (hs // 2, ws // 2), (0, 1))
        n = 15 * 31
        WIN["crafted"] = dict(q=u[None, None, None].expand(b, h, w, heads, d).contiguous(), k=k, v=r16(seeded((b, h, w, heads, d), 78)), split=split,
                              tables=(seeded((n, 1), 79, 1.5), seeded((n, 1), 80, 1.5)), graphs={})
    return WIN["crafted"]


def test_the_mask_is_minus_100_not_minus_infinity(dev):
    case = crafted_mask_case()
    ref, twin = win_graph(case, True), win_graph(case, True, r16d)
    yard = rel_l2(twin, ref)
    assert rel_l2(win_graph(case, True, mask_value=-math.inf), ref) > 10 * yard          # the two masks differ on this input (on the CPU)
    got, _ = from_slots(run_win(dev, case, True).cpu(), 2, 32)
    assert_parity(got, ref, twin, 3, (0, 1), "window attention, crafted -100 mask case")


def test_window_attention_in_rows_wider_than_the_slots(dev):
    """ldq = 96 heads + 8, ldo = 32 heads + 8, the out buffer pre-filled: the excess keeps its bits, the result is bit-equal to the dense
    call."""
    case = win_case(1, 24, 40, 6, 10, (8, 16))
    dense = run_win(dev, case, True)
    out = torch.full((1, 24, 40, 200), 3.0, dtype=torch.float16).to(dev)
    got = run_win(dev, case, True, ldq=584, out_tensor=out)
    assert got is out and bool((out.cpu()[..., 192:] == 3).all())
    assert same_bits(out[..., :192], dense)


def test_window_attention_refuses_what_it_is_not_built_for(dev):
    """Every refusal returns non-zero with a message and writes nothing."""
    _lib = sub("_lib")
    case = win_case(1, 16, 16, 2, 32, (8, 16))
    out = torch.full((1, 16, 16, 72), 7.0, dtype=torch.float16).to(dev)
    desc, hold = win_desc(dev, case, True, ldq=200, out_tensor=out)
    assert _lib.lib.sdmi_dat_window_attention(ctypes.byref(desc), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = [(dict(qkv=None), "null"), (dict(bias0=None), "null"), (dict(bias1=None), "null"), (dict(out=None), "null"),
           (dict(H=0), "empty token grid"), (dict(W=-1), "empty token grid"), (dict(B=0), "empty token grid"),
           (dict(heads=3), "heads must be even"), (dict(heads=0), "heads must be even"), (dict(D=0), "1..32"), (dict(D=33), "1..32"),
           (dict(s0=16), "split must be"), (dict(s1=8), "split must be"), (dict(s1=64), "split must be"),
           (dict(shift_h=2), "shift must be"), (dict(shift_w=0), "shift must be"), (dict(shift_h=0), "shift must be"),
           (dict(ldq=184), "ldq >= 96 heads"), (dict(ldo=56), "ldo >= 32 heads"),
           (dict(qkv=hold[0].data_ptr() + 2), "misaligned"), (dict(out=out.data_ptr() + 8), "misaligned"), (dict(bias0=hold[1].data_ptr() + 2), "misaligned"),
           (dict(ldq=196), "misaligned"), (dict(ldo=68), "misaligned")]
    for kw, msg in bad:
        d2, _ = win_desc(dev, case, True, ldq=200, out_tensor=out, fields=kw)
        assert _lib.lib.sdmi_dat_window_attention(ctypes.byref(d2), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.lib.sdmi_dat_window_attention(None, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- channel attention --------------------------------------------------------------------------------------------------------------
CH_CASES = [(2, 1, 6, 30, False), (1, 64, 2, 32, False), (2, 9 * 13, 6, 30, True), (1, 40 * 72, 6, 30, False), (1, 40 * 72, 2, 32, False)]


def channel_case(b, n, heads, d, zero_column):
    seed = 4000 + n + 7 * heads + d
    q, k = (r16(seeded((b, n, heads, d), seed + i)) for i in range(2))
    if zero_column:
        q[0, :, 1, 3] = 0                                          # an all-zero q column: the 1e-12 path, a uniform row
        k[b - 1, :, 0, 5] = 0
    u = torch.rand((heads,), generator=torch.Generator().manual_seed(seed + 2))
    return q, k, 0.5 + 9.5 * u                                     # temperatures up to 10


def channel_graph(q, k, temp):
    """float64: A[b, h] = softmax_j(temp[h] q^_i . k^_j), the norms over the tokens."""
    qn = q.double() / q.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    kn = k.double() / k.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.softmax(torch.einsum("bnhi,bnhj->bhij", qn, kn) * temp.double().view(1, -1, 1, 1), dim=-1)


def run_channel(dev, q, k, temp):
    """The two launches -> A fp16 [b, 32 heads, 32 heads] (on the CPU) and the partials."""
    _lib = sub("_lib")
    L, p, s = _lib.lib, _lib.ptr, _lib.stream_ptr()
    b, n, heads, d = q.shape
    qkv = torch.cat([to_slots(q.flatten(2), heads, d), to_slots(k.flatten(2), heads, d)], dim=-1).contiguous().to(dev)
    nblk = (n + 511) // 512
    part = torch.full((b, heads, nblk, 1088), 7.0, dtype=torch.float32).to(dev)
    a = torch.full((b, 32 * heads, 32 * heads), 7.0, dtype=torch.float16).to(dev)
    t = temp.float().contiguous().to(dev)
    _lib.check(L.sdmi_dat_channel_gram(p(qkv), p(part), b, n, heads, 64 * heads, s), "sdmi_dat_channel_gram")
    _lib.check(L.sdmi_dat_channel_softmax(p(part), p(t), p(a), b, n, heads, d, s), "sdmi_dat_channel_softmax")
    torch.cuda.synchronize()
    return a.cpu(), part.cpu()


@pytest.mark.parametrize("b,n,heads,d,zero_column", CH_CASES)
def test_channel_attention_matrix_vs_float64(dev, b, n, heads, d, zero_column):
    q, k, temp = channel_case(b, n, heads, d, zero_column)
    a, part = run_channel(dev, q, k, temp)
    assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(part).all())
    blocks = a.view(b, heads, 32, heads, 32)
    got = torch.stack([blocks[:, h, :d, h, :d] for h in range(heads)], dim=1)
    off = a.clone().view(b, heads, 32, heads, 32)
    for h in range(heads):
        off[:, h, :d, h, :d] = 0
    assert bool((off == 0).all())                                  # zeros outside the heads' D x D blocks
    ref = channel_graph(q, k, temp)
    assert_parity(got, ref, r16d(ref), 1, (0, 2), f"channel attention B{b} N{n} heads {heads} D {d}")
    if zero_column:
        assert float((got[0, 1, 3].float() - 1.0 / d).abs().max()) < 1e-3
    a2, part2 = run_channel(dev, q, k, temp)                       # fixed-order sums: two runs give the same bits
    assert same_bits(a, a2) and torch.equal(part, part2)


def test_channel_attention_refusals(dev):
    _lib = sub("_lib")
    L, s = _lib.lib, _lib.stream_ptr()

    def p(t):
        return t.data_ptr()
    qkv = torch.zeros((1, 64, 136), dtype=torch.float16).to(dev)
    part = torch.full((1, 2, 1, 1088), 7.0, dtype=torch.float32).to(dev)
    a = torch.full((1, 64, 64), 7.0, dtype=torch.float16).to(dev)
    t = torch.ones(3, dtype=torch.float32).to(dev)
    for args, msg in [((None, p(part), 1, 64, 2, 136), "null"), ((p(qkv), None, 1, 64, 2, 136), "null"), ((p(qkv), p(part), 0, 64, 2, 136), "empty"),
                      ((p(qkv), p(part), 1, 0, 2, 136), "empty"), ((p(qkv), p(part), 1, 64, 2, 120), "ldq >= 64 heads"),
                      ((p(qkv), p(part), 1, 64, 2, 132), "misaligned"), ((p(qkv) + 2, p(part), 1, 64, 2, 136), "misaligned")]:
        assert L.sdmi_dat_channel_gram(*args, s) != 0, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    for args, msg in [((None, p(t), p(a), 1, 64, 2, 30), "null"), ((p(part), None, p(a), 1, 64, 2, 30), "null"), ((p(part), p(t), None, 1, 64, 2, 30), "null"),
                      ((p(part), p(t), p(a), 1, 64, 2, 0), "1..32"), ((p(part), p(t), p(a), 1, 64, 2, 33), "1..32"),
                      ((p(part), p(t), p(a), 1, 0, 2, 30), "empty"), ((p(part), p(t) + 2, p(a), 1, 64, 2, 30), "misaligned")]:
        assert L.sdmi_dat_channel_softmax(*args, s) != 0, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((part.cpu() == 7).all()) and bool((a.cpu() == 7).all())


# ---- depthwise conv -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ep", [0, 1])
@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (1, 17)])
def test_dwconv3x3_vs_float64(dev, h, w, ep):
    _lib = sub("_lib")
    b, c, ldx, ldm, ldo = 2, 64, 80, 144, 72
    x = r16(seeded((b, h, w, c), 5000 + h + w))
    wt, bias = seeded((c, 1, 3, 3), 5001 + h, 0.5), seeded((c,), 5002 + h, 0.3)
    mul = r16(seeded((b, h, w, c), 5003 + w))
    conv = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), padding=1, groups=c).permute(0, 2, 3, 1)
    ref = F.gelu(conv) if ep == 0 else conv * mul.double()

    def wide(t, ld, fill):
        o = torch.full((b, h, w, ld), fill, dtype=torch.float16)
        o[..., :c] = t.half()
        return o.to(dev)
    xd, md, out = wide(x, ldx, 1e4), wide(mul, ldm, 1e4), torch.full((b, h, w, ldo), 3.0, dtype=torch.float16).to(dev)
    w9 = wt.view(c, 9).t().contiguous().to(dev)                    # [9][C]
    bd = bias.to(dev)
    p = _lib.ptr
    _lib.check(_lib.lib.sdmi_dat_dwconv3x3(p(xd), p(w9), p(bd), p(md) if ep else None, p(out), b, h, w, c, ldx, ldm if ep else 0, ldo, ep,
                                           _lib.stream_ptr()), "sdmi_dat_dwconv3x3")
    torch.cuda.synchronize()
    assert bool((out.cpu()[..., c:] == 3).all())
    assert_parity(out.cpu()[..., :c], ref, r16d(ref), 3, (0, 1), f"dwconv3x3 {h}x{w} ep {ep}")


def test_dwconv3x3_refusals(dev):
    _lib = sub("_lib")
    L, s = _lib.lib, _lib.stream_ptr()

    def p(t):
        return t.data_ptr()
    x = torch.zeros((1, 4, 4, 64), dtype=torch.float16).to(dev)
    out = torch.full((1, 4, 4, 64), 7.0, dtype=torch.float16).to(dev)
    w9, bias = torch.zeros((9, 64), dtype=torch.float32).to(dev), torch.zeros(64, dtype=torch.float32).to(dev)
    good = dict(x=p(x), w=p(w9), bias=p(bias), mul=None, out=p(out), B=1, H=4, W=4, C=64, ldx=64, ldm=0, ldo=64, ep=0)
    for kw, msg in [(dict(x=None), "null"), (dict(out=None), "null"), (dict(w=None), "null"), (dict(ep=2), "epilogue"), (dict(ep=1), "null mul"),
                    (dict(H=0), "empty"), (dict(C=60), "multiple of 8"), (dict(ldx=56), "narrower"), (dict(ldo=68), "misaligned"),
                    (dict(x=p(x) + 2), "misaligned"), (dict(out=p(x)), "alias")]:
        a = dict(good, **kw)
        assert L.sdmi_dat_dwconv3x3(a["x"], a["w"], a["bias"], a["mul"], a["out"], a["B"], a["H"], a["W"], a["C"], a["ldx"], a["ldm"], a["ldo"], a["ep"], s) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- the AIM gates ------------------------------------------------------------------------------------------------------------------
AIM = {}


def aim_case(n):
    """att, conv [2, n, 192] (fp16 values; 6 heads x 30 in slots, tails zero) and the two interaction MLPs (BatchNorm already folded)."""
    if n not in AIM:
        c, c8, c16, seed = 192, 22, 11, 6000 + n
        att, conv = (to_slots(r16(seeded((2, n, 180), seed + i)), 6, 30).float() for i in range(2))
        live = (att[0, 0] != 0) | (conv[0, 0] != 0)
        AIM[n] = dict(att=att, conv=conv, c8=c8, c16=c16,
                      ci_w1=seeded((c8, c), seed + 2, 3.0 / math.sqrt(c)) * live, ci_b1=seeded((c8,), seed + 3, 0.2),
                      ci_w2=seeded((c, c8), seed + 4, 2.0 / math.sqrt(c8)) * live[:, None], ci_b2=seeded((c,), seed + 5, 0.2) * live,
                      si_w1=seeded((c16, c), seed + 6, 1.5 / math.sqrt(c)) * live, si_b1=seeded((c16,), seed + 7, 0.2),
                      si_w2=seeded((c16,), seed + 8, 2.0 / math.sqrt(c16)), si_b2=0.1)
    return AIM[n]


def gate_ref(case, t):
    mean = t.double().mean(1)
    hid = F.gelu(mean @ case["ci_w1"].double().t() + case["ci_b1"].double())
    return torch.sigmoid(hid @ case["ci_w2"].double().t() + case["ci_b2"].double())


def run_gate(dev, case, t):
    _lib = sub("_lib")
    p = _lib.ptr
    b, n, c = t.shape
    hold = [t.half().to(dev)] + [case[k].float().contiguous().to(dev) for k in ("ci_w1", "ci_b1", "ci_w2", "ci_b2")]
    ws = torch.zeros((b, (n + 255) // 256, c), dtype=torch.float32).to(dev)
    gate = torch.full((b, c), 7.0, dtype=torch.float32).to(dev)
    _lib.check(_lib.lib.sdmi_dat_pool_gate(*(p(x) for x in hold), p(ws), p(gate), b, n, c, case["c8"], c, _lib.stream_ptr()), "sdmi_dat_pool_gate")
    torch.cuda.synchronize()
    return gate


@pytest.mark.parametrize("n", [9 * 13, 300])                       # one block of 256 tokens, and two
def test_pool_gate_vs_float64(dev, n):
    case = aim_case(n)
    for name in ("conv", "att"):
        got = run_gate(dev, case, case[name])
        ref = gate_ref(case, case[name])
        err = rel_l2(got.cpu(), ref)
        print(f"[dat parity] pool gate of {name}, N {n}: engine {err:.3e} (fp32 out: bound 1e-5)")
        assert err < 1e-5
        assert torch.equal(got.cpu(), run_gate(dev, case, case[name]).cpu())


@pytest.mark.parametrize("spatial", [True, False])
def test_aim_combine_vs_float64(dev, spatial):
    """Spatial block: out = att sigmoid(cmap(conv)) + sigmoid(smap(att)) conv; channel block: out = att sigmoid(smap(conv)) + conv sigmoid(cmap(att))."""
    _lib = sub("_lib")
    n = 300
    case = aim_case(n)
    s, t = (case["att"], case["conv"]) if spatial else (case["conv"], case["att"])
    hid = F.gelu(s.double() @ case["si_w1"].double().t() + case["si_b1"].double())
    sg = torch.sigmoid(hid @ case["si_w2"].double() + case["si_b2"])
    ref = s.double() * gate_ref(case, t)[:, None] + t.double() * sg[..., None]
    gate = run_gate(dev, case, t)
    hold = [s.half().to(dev), t.half().to(dev), gate] + [case[k].float().contiguous().to(dev) for k in ("si_w1", "si_b1", "si_w2")]
    out = torch.full((2, n, 200), 3.0, dtype=torch.float16).to(dev)
    d = _lib.DatAimDesc()
    d.s, d.t, d.gate, d.w1, d.b1, d.w2 = (x.data_ptr() for x in hold)
    d.b2, d.out, d.rows, d.rows_per_image, d.C, d.C16, d.lds, d.ldt, d.ldo = case["si_b2"], out.data_ptr(), 2 * n, n, 192, case["c16"], 192, 192, 200
    _lib.check(_lib.lib.sdmi_dat_aim_combine(ctypes.byref(d), _lib.stream_ptr()), "sdmi_dat_aim_combine")
    torch.cuda.synchronize()
    assert bool((out.cpu()[..., 192:] == 3).all())
    got, tails = from_slots(out.cpu(), 6, 30)
    assert bool((tails == 0).all())
    ref = from_slots(ref, 6, 30)[0]
    assert_parity(got, ref, r16d(ref), 2, (0, 1), f"aim_combine, {'spatial' if spatial else 'channel'} block")
    for kw, msg in [(dict(s=None), "null"), (dict(out=None), "null"), (dict(rows=2 * n + 1), "multiple of rows_per_image"), (dict(C=180), "multiple of 64"),
                    (dict(C16=0), "8192"), (dict(C16=64), "8192"), (dict(lds=128), "narrower"), (dict(gate=gate.data_ptr() + 2), "misaligned")]:
        for k, v in kw.items():
            old = getattr(d, k)
            setattr(d, k, v)
        assert _lib.lib.sdmi_dat_aim_combine(ctypes.byref(d), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
        setattr(d, k, old)
    assert _lib.lib.sdmi_dat_aim_combine(None, _lib.stream_ptr()) != 0


# ---- network level ----------------------------------------------------------------------------------------------------------------
T60 = dict(embed_dim=60, depths=(4, 2), heads=6, expansion=2)      # a shifted block in an even group (j = 2) and in an odd one (j = 0)
NET_CASES = {                                                      # name: (make_state_dict keywords, (b, h, w))
    "x2-s16": (dict(T60, scale=2, split=(8, 16)), (2, 24, 40)),
    "x3-s32": (dict(T60, scale=3, split=(8, 32)), (1, 37, 21)),
    "x4-s32": (dict(T60, scale=4, split=(8, 32)), (2, 24, 40)),
    "x4-s16": (dict(T60, scale=4, split=(8, 16)), (1, 37, 21)),
    "c180-x2": (dict(embed_dim=180, depths=(2,), heads=6, expansion=4, scale=2, split=(8, 32)), (1, 32, 40)),
}
NETS, REFS, ENGINE = {}, {}, []


def shared_engine():
    if not ENGINE:
        ENGINE.append(sub("engine").Engine(0))
    return ENGINE[0]


def state_dict_for(name):
    return R.make_state_dict(**NET_CASES[name][0])


def net_for(name):
    if name not in NETS:
        sd = state_dict_for(name)
        NETS[name] = (sd, sub("upscaler").DATNet(sd, device=0, engine=shared_engine()))
    return NETS[name]


def reference_for(name):
    """(x, fp32 reference, fp16-storage twin) of a case: computed once, shared, never modified."""
    if name not in REFS:
        kw, (b, h, w) = NET_CASES[name]
        sd = state_dict_for(name)
        x = R.image(b, h, w, 40 + kw["scale"])
        REFS[name] = (x, R.forward(sd, x), R.fp16_twin(sd, x))
    return REFS[name]


@pytest.mark.parametrize("name", list(NET_CASES))
def test_dat_network_vs_reference(dev, name):
    kw, (b, h, w) = NET_CASES[name]
    sd, net = net_for(name)
    s = kw["scale"]
    assert net.scale == s and net.config == R.config_of(sd)
    x, ref, twin = reference_for(name)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * s, w * s) and got.dtype == torch.float32
    assert 0 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    assert_parity(got, ref, twin, 1, (0, 2), f"network {name} {b}x{h}x{w}")


def test_dat_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_dat_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB)."""
    name = "x3-s32"
    kw, (b, h, w) = NET_CASES[name]
    engine = sub("engine").Engine(0)
    net = sub("upscaler").DATNet(state_dict_for(name), device=0, engine=engine)
    assert engine.arena_bytes() == 0
    got = net.run(reference_for(name)[0].to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, h * 3, w * 3) and 0 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


@pytest.mark.parametrize("name", ["x2-s16", "x3-s32"])
def test_dat_uint8_in_and_out(dev, name):
    """uint8 in is the same image: the same output.  uint8 out: the bytes equal model_output_to_u8 of the same run's fp32 output."""
    up = sub("upscaler")
    kw, (b, h, w) = NET_CASES[name]
    s = kw["scale"]
    sd, net = net_for(name)
    x = reference_for(name)[0]
    x8 = torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    f32 = net.run(x8)
    assert float((f32.cpu() - net.run(x.to(dev)).cpu()).abs().max()) < 1e-6
    u8 = net.run(x8, out_u8=True)
    assert u8.shape == (b, h * s, w * s, 3) and u8.dtype == torch.uint8
    assert np.array_equal(u8.cpu().numpy(), up.model_output_to_u8(f32.cpu().permute(0, 2, 3, 1).numpy()))


def config_c(sd, **kw):
    _lib = sub("_lib")
    cfg = R.config_of(sd)
    c = _lib.DATConfigC()
    c.embed_dim, c.num_layers, c.num_heads, c.ffn_hidden, c.scale = cfg["embed_dim"], len(cfg["depths"]), cfg["num_heads"], cfg["ffn_hidden"], cfg["scale"]
    c.split0, c.split1 = cfg["split"]
    for i, d in enumerate(cfg["depths"]):
        c.depths[i] = d
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_dat_handle_entries_directly(dev):
    """The C entries by name: blob_floats, create (and what it refuses), scratch_bytes, run (and an empty image), destroy."""
    _lib, up = sub("_lib"), sub("upscaler")
    L = _lib.lib
    name = "x3-s32"
    sd = state_dict_for(name)
    blob, config = up.parse_dat_state_dict(sd)
    eng = shared_engine()
    assert L.sdmi_dat_blob_floats(ctypes.byref(config_c(sd))) == blob.size
    for other in NET_CASES:
        sd2 = state_dict_for(other)
        assert L.sdmi_dat_blob_floats(ctypes.byref(config_c(sd2))) == up.parse_dat_state_dict(sd2)[0].size, other
    refused = [(dict(num_heads=1), "multiple of num_heads"), (dict(num_heads=5), "num_heads must be even"), (dict(embed_dim=96, num_heads=2), "<= 32"),
               (dict(embed_dim=61), "multiple of num_heads"), (dict(embed_dim=640, num_heads=20), "<= 512"), (dict(split0=16), "split must be"),
               (dict(split1=24), "split must be"), (dict(ffn_hidden=121), "ffn_hidden must be even"), (dict(scale=5), "scale 2 | 3 | 4"),
               (dict(scale=1), "scale 2 | 3 | 4"), (dict(num_layers=17), "num_layers"), (dict(num_layers=0), "num_layers")]
    for kw, msg in refused:
        assert L.sdmi_dat_blob_floats(ctypes.byref(config_c(sd, **kw))) == 0, kw
        assert not L.sdmi_dat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd, **kw))), kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert not L.sdmi_dat_create(eng.handle, blob.ctypes.data, blob.size - 1, ctypes.byref(config_c(sd)))
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_dat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd, scale=4)))      # another tail: another length
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_dat_create(eng.handle, None, blob.size, ctypes.byref(config_c(sd)))
    h = L.sdmi_dat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd)))
    assert h, _lib.last_error()
    try:
        assert L.sdmi_dat_scratch_bytes(h, 1, 37, 21) > 0
        assert L.sdmi_dat_scratch_bytes(h, 1, 0, 21) == 0
        assert L.sdmi_dat_scratch_bytes(None, 1, 37, 21) == 0
        x, ref, twin = reference_for(name)
        xd = x.to(dev)
        out = torch.full((1, 3, 111, 63), 7.0, dtype=torch.float32).to(dev)
        assert L.sdmi_dat_run(h, _lib.ptr(xd), 0, 1, 0, 21, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        assert "empty image" in _lib.last_error()
        assert L.sdmi_dat_run(h, None, 0, 1, 37, 21, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        torch.cuda.synchronize()
        assert bool((out.cpu() == 7).all())
        _lib.check(L.sdmi_dat_run(h, _lib.ptr(xd), 0, 1, 37, 21, _lib.ptr(out), 0, _lib.stream_ptr()), "sdmi_dat_run")
        assert_parity(out, ref, twin, 1, (0, 2), "direct handle, 37x21")
    finally:
        L.sdmi_dat_destroy(h)


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_dat_checkpoint(dev, tmp_path):
    from PIL import Image
    up = sub("upscaler")
    sd, net = net_for("x2-s16")
    path = str(tmp_path / "tiny_dat_x2.pth")
    torch.save({"params": sd}, path)
    src = np.random.RandomState(5).randint(90, 166, size=(19, 13, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0, engine=shared_engine())
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (26, 38) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.DATNet)
    direct = net.run(torch.from_numpy(src[None]).to(dev))[0].cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(img), up.model_output_to_u8(direct))


def test_resize_image_through_a_registered_dat_upscaler(dev, tmp_path, monkeypatch):
    from PIL import Image
    up, shared = sub("upscaler"), sub("shared")
    sd = net_for("x2-s16")[0]
    path = str(tmp_path / "tiny_dat_x2.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    added = up.register_esrgan({"Tiny-DAT 2x": path}, engine=shared_engine())
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-DAT 2x"] and added[0].scale == 2
    im = Image.fromarray(np.random.RandomState(6).randint(90, 166, size=(16, 24, 3), dtype=np.uint8))
    got = up.resize_image(0, im, 48, 32, "Tiny-DAT 2x")
    assert got.size == (48, 32) and isinstance(added[0].scaler._nets[path], up.DATNet)
    assert np.array_equal(np.asarray(got), np.asarray(added[0].scaler.do_upscale(im, path)))
