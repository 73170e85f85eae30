"""GPU parity tests of the HAT path: the window attention kernel through sdmi_hat_window_attention, in its self and its overlap form, against
float64 graphs written independently of tests/hat_reference.py (every window's tokens gathered by their coordinates: no roll, no
partition, no unfold; a dense bias from the index formulas), the channel gate and the branch sum against float64, whole networks
through sdmi_hat_run against tests/hat_reference.py (fp32, CPU), the handle entries, UpscalerESRGAN.do_upscale on a HAT checkpoint and
one resize through the registry.

Comparison rule: `assert_parity` of tests/test_gpu_dat.py, unchanged — the yardstick is the distance of the fp16-storage twin from the
reference; the engine's rel_l2 from the same reference stays within 1.25 x the yardstick, every slice (per channel, per image row) within
2.5 x the yardstick, the yardstick itself is asserted above 1e-4 and the twin's own worst slice within 2.5 x of it.  The channel gate is
fp32 in memory (no fp16 storage, so no yardstick): its bound 1e-5 is fp32's — sums of at most a few hundred terms in a fixed order
(relative error below 1e-6) through exp with a relative error of a few 1e-7.  Every case also runs on the host-emulated library
(tests/test_cpu_hat.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import hat_reference as R
from fp16_emu import r16
from helpers import rel_l2, seeded
from test_gpu_dat import assert_parity, from_slots, ident, r16d, same_bits, sub, to_slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


# ---- window attention ---------------------------------------------------------------------------------------------------------------
SELF_CASES = [(1, 16, 16, 6, 30, 0),                         # one window
              (2, 32, 32, 6, 30, 8),                         # all nine regions
              (1, 48, 32, 2, 32, 8),
              (1, 32, 48, 5, 24, 0)]                         # an odd head count
OVERLAP_CASES = [(1, 16, 16, 6, 30),                         # 320 of the 576 keys are padding
                 (2, 32, 48, 6, 30),
                 (1, 48, 48, 2, 32),                         # the centre window has no padding
                 (1, 32, 32, 5, 24)]
WIN = {}


def win_case(mode, b, h, w, heads, d):
    """Seeded q, k, v [b, h, w, heads, d] (fp16 values) and the bias table N(0, 1.5^2): [961, heads] for the self form, [1521, heads] in
    offset order for the overlap form.  The float64 graphs are computed once per case and shared."""
    key = (mode, b, h, w, heads, d)
    if key not in WIN:
        seed = 7000 + 1000 * mode + 7 * heads + d + h + 3 * w
        q, k, v = (r16(seeded((b, h, w, heads, d), seed + i)) for i in range(3))
        WIN[key] = dict(q=q, k=k, v=v, mode=mode, table=seeded((1521 if mode else 961, heads), seed + 3, 1.5), graphs={})
    return WIN[key]


def region(u, n):
    return torch.where(u < n - 16, 0, torch.where(u < n - 8, 1, 2))


def win_graph(case, shift=0, rnd=ident, bias=True, mask=True, mask_value=-100.0, mask_padded_keys=False, transpose_table=False):
    """The float64 graph, window by window, by coordinates.  Self: query / key a of window (wy, wx) is the token at ((16 wy + a / 16 +
    shift) % h, (16 wx + a % 16 + shift) % w); its region id comes from (16 wy + a / 16, 16 wx + a % 16).  Overlap: key b is the token at
    (16 wy - 4 + b / 24, 16 wx - 4 + b % 24), a zero row outside the grid.  Dense bias from the index formula of the descriptor."""
    key = (shift, rnd is ident, bias, mask, mask_value, mask_padded_keys, transpose_table)
    if key in case["graphs"]:
        return case["graphs"][key]
    q, k, v = (case[n].double() for n in "qkv")
    b, h, w, heads, d = q.shape
    table = case["table"].double()
    ay, ax = torch.arange(256) // 16, torch.arange(256) % 16
    if case["mode"]:
        by, bx = torch.arange(576) // 24, torch.arange(576) % 24
        if transpose_table:
            table = table.view(39, 39, heads).transpose(0, 1).reshape(1521, heads)
        index = (by[None, :] - ay[:, None] + 15) * 39 + (bx[None, :] - ax[:, None] + 15)
    else:
        by, bx = ay, ax
        if transpose_table:
            table = table.view(31, 31, heads).transpose(0, 1).reshape(961, heads)
        index = (ay[:, None] - by[None, :] + 15) * 31 + (ax[:, None] - bx[None, :] + 15)
    dense = table[index.reshape(-1)].view(256, len(by), heads).permute(2, 0, 1)                       # [heads, query, key]
    out = torch.zeros((b, h, w, heads, d), dtype=torch.float64)
    for wy in range(h // 16):
        for wx in range(w // 16):
            qy, qx = (16 * wy + ay + shift) % h, (16 * wx + ax + shift) % w
            if case["mode"]:
                ky, kx = 16 * wy - 4 + by, 16 * wx - 4 + bx
                inside = (ky >= 0) & (ky < h) & (kx >= 0) & (kx < w)
                kw = torch.where(inside[None, :, None, None], k[:, ky.clamp(0, h - 1), kx.clamp(0, w - 1)], 0.0)
                vw = torch.where(inside[None, :, None, None], v[:, ky.clamp(0, h - 1), kx.clamp(0, w - 1)], 0.0)
            else:
                kw, vw = k[:, qy, qx], v[:, qy, qx]
            score = torch.einsum("bnhd,bmhd->bhnm", q[:, qy, qx] * d ** -0.5, kw)
            if bias:
                score = score + dense[None]
            if shift and mask:
                ids = 3 * region(16 * wy + ay, h) + region(16 * wx + ax, w)
                score = score + torch.where(ids[:, None] != ids[None, :], mask_value, 0.0).double()[None, None]
            if mask_padded_keys:
                score = score.masked_fill(~inside[None, None, None, :], -math.inf)
            p = rnd(torch.softmax(score, dim=-1))
            out[:, qy, qx] = rnd(torch.einsum("bhnm,bmhd->bnhd", p, vw))
    case["graphs"][key] = out.flatten(3)
    return case["graphs"][key]


def win_desc(dev, case, shift=0, ldq=None, out_tensor=None, fields=None):
    """-> (descriptor, the tensors it points at)."""
    _lib = sub("_lib")
    b, h, w, heads, d = case["q"].shape
    ldq = ldq or 96 * heads
    qkv = torch.full((b, h, w, ldq), 1e4, dtype=torch.float16)
    qkv[..., :96 * heads] = torch.cat([to_slots(case[n].flatten(3), heads, d) for n in "qkv"], dim=-1)
    hold = [qkv.to(dev), case["table"].float().contiguous().to(dev),
            out_tensor if out_tensor is not None else torch.empty((b, h, w, 32 * heads), dtype=torch.float16, device=dev)]
    desc = _lib.HatAttnDesc()
    desc.qkv, desc.bias, desc.out = (t.data_ptr() for t in hold)
    desc.B, desc.H, desc.W, desc.heads, desc.D, desc.ldq, desc.ldo = b, h, w, heads, d, ldq, hold[2].shape[3]
    desc.mode, desc.shift, desc.scale = case["mode"], shift, d ** -0.5
    for k, v in (fields or {}).items():
        setattr(desc, k, v)
    return desc, hold


def run_win(dev, case, shift=0, **kw):
    _lib = sub("_lib")
    desc, hold = win_desc(dev, case, shift, **kw)
    _lib.check(_lib.lib.sdmi_hat_window_attention(ctypes.byref(desc), _lib.stream_ptr()), "sdmi_hat_window_attention")
    torch.cuda.synchronize()
    return hold[2]


@pytest.mark.parametrize("b,h,w,heads,d,shift", SELF_CASES)
def test_self_attention_vs_float64_graph(dev, b, h, w, heads, d, shift):
    case = win_case(0, b, h, w, heads, d)
    out = run_win(dev, case, shift)
    assert out.shape == (b, h, w, 32 * heads) and out.dtype == torch.float16
    got, tails = from_slots(out.cpu(), heads, d)
    assert bool((tails == 0).all())
    ref, twin = win_graph(case, shift), win_graph(case, shift, r16d)
    _, yard = assert_parity(got, ref, twin, 3, (0, 1), f"hat self attention B{b} {h}x{w} heads {heads} D {d} shift {shift}")
    assert rel_l2(got, win_graph(case, shift, bias=False)) > 10 * yard                   # the bias is really applied
    assert rel_l2(got, win_graph(case, shift, transpose_table=True)) > 10 * yard         # ... at (dy, dx), not (dx, dy)
    if shift:
        assert rel_l2(got, win_graph(case, shift, mask=False)) > 10 * yard               # ... and the mask


@pytest.mark.parametrize("b,h,w,heads,d", OVERLAP_CASES)
def test_overlap_attention_vs_float64_graph(dev, b, h, w, heads, d):
    case = win_case(1, b, h, w, heads, d)
    out = run_win(dev, case)
    assert out.shape == (b, h, w, 32 * heads) and out.dtype == torch.float16
    got, tails = from_slots(out.cpu(), heads, d)
    assert bool((tails == 0).all())
    ref, twin = win_graph(case), win_graph(case, 0, r16d)
    _, yard = assert_parity(got, ref, twin, 3, (0, 1), f"hat overlap attention B{b} {h}x{w} heads {heads} D {d}")
    assert rel_l2(got, win_graph(case, bias=False)) > 10 * yard
    assert rel_l2(got, win_graph(case, transpose_table=True)) > 10 * yard
    assert rel_l2(got, win_graph(case, mask_padded_keys=True)) > 10 * yard               # keys outside the grid are keys (score 0 + bias)


def crafted_mask_case():
    """Self form, shift 8, one 16 x 16 grid (regions 4, 5, 7, 8 in its one window): q = u everywhere with |u|^2 D^-1/2 = 80, k = +u in the
    regions of even id and -u in the odd ones: a query of an odd region sees its own region at -80 + bias and the MASKED even regions at
    +80 - 100 + bias, so its output comes from masked keys — with a -inf mask it would come from its own region."""
    if "crafted" not in WIN:
        b, h, w, heads, d = 1, 16, 16, 2, 32
        u = seeded((heads, d), 177)
        u = r16(u * torch.sqrt(80.0 * math.sqrt(d) / (u * u).sum(-1, keepdim=True)))
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")        # the shifted grid
        sign = torch.where((3 * region(ys, h) + region(xs, w)) % 2 == 0, 1.0, -1.0)
        k = torch.roll(sign[:, :, None, None] * u[None, None], (8, 8), (0, 1))[None]    # token (ys, xs) of the shifted grid sits at (ys + 8, xs + 8)
        WIN["crafted"] = dict(q=u[None, None, None].expand(b, h, w, heads, d).contiguous(), k=k.contiguous(), v=r16(seeded((b, h, w, heads, d), 178)),
                              mode=0, table=seeded((961, heads), 179, 1.5), graphs={})
    return WIN["crafted"]


def test_the_mask_is_minus_100_not_minus_infinity(dev):
    case = crafted_mask_case()
    ref, twin = win_graph(case, 8), win_graph(case, 8, r16d)
    yard = rel_l2(twin, ref)
    assert rel_l2(win_graph(case, 8, mask_value=-math.inf), ref) > 10 * yard             # the two masks differ on this input (on the CPU)
    got, _ = from_slots(run_win(dev, case, 8).cpu(), 2, 32)
    assert_parity(got, ref, twin, 3, (0, 1), "hat self attention, crafted -100 mask case")


@pytest.mark.parametrize("mode", [0, 1])
def test_window_attention_in_rows_wider_than_the_slots_and_twice(dev, mode):
    """ldq = 96 heads + 8, ldo = 32 heads + 40 (an odd head count), the out buffer pre-filled: the excess keeps its bits, the result is
    bit-equal to the dense call, and a second dense call gives the same bits."""
    case = win_case(mode, 1, 32, 48 if mode == 0 else 32, 5, 24)
    shift = 0 if mode else 8
    dense = run_win(dev, case, shift)
    assert same_bits(dense, run_win(dev, case, shift))
    out = torch.full((1, 32, case["q"].shape[2], 200), 3.0, dtype=torch.float16).to(dev)
    got = run_win(dev, case, shift, ldq=488, out_tensor=out)
    assert got is out and bool((out.cpu()[..., 160:] == 3).all())
    assert same_bits(out[..., :160], dense)


def test_window_attention_refuses_what_it_is_not_built_for(dev):
    """Every refusal returns non-zero with a message and writes nothing."""
    _lib = sub("_lib")
    case = win_case(0, 1, 16, 16, 6, 30)
    out = torch.full((1, 16, 16, 200), 7.0, dtype=torch.float16).to(dev)
    desc, hold = win_desc(dev, case, 8, ldq=584, out_tensor=out)
    assert _lib.lib.sdmi_hat_window_attention(ctypes.byref(desc), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = [(dict(qkv=None), "null"), (dict(bias=None), "null"), (dict(out=None), "null"), (dict(mode=2), "mode 0"), (dict(mode=-1), "mode 0"),
           (dict(H=0), "empty token grid"), (dict(W=-16), "empty token grid"), (dict(B=0), "empty token grid"),
           (dict(H=24), "multiples of 16"), (dict(W=8), "multiples of 16"), (dict(heads=0), "heads must be"), (dict(D=0), "1..32"), (dict(D=33), "1..32"),
           (dict(shift=4), "shift must be"), (dict(shift=-8), "shift must be"), (dict(mode=1, shift=8), "shift must be"),
           (dict(ldq=568), "ldq >= 96 heads"), (dict(ldo=184), "ldo >= 32 heads"),
           (dict(qkv=hold[0].data_ptr() + 2), "misaligned"), (dict(out=out.data_ptr() + 8), "misaligned"), (dict(bias=hold[1].data_ptr() + 2), "misaligned"),
           (dict(ldq=580), "misaligned"), (dict(ldo=196), "misaligned"), (dict(out="qkv"), "alias")]
    for kw, msg in bad:
        d2, _ = win_desc(dev, case, 8, ldq=584, out_tensor=out, fields={k: v for k, v in kw.items() if v != "qkv"})
        if kw.get("out") == "qkv":
            d2.out = d2.qkv
        assert _lib.lib.sdmi_hat_window_attention(ctypes.byref(d2), _lib.stream_ptr()) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert _lib.lib.sdmi_hat_window_attention(None, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == 7).all())


# ---- the conv branch's gate and sum -----------------------------------------------------------------------------------------------
CAB_CASES = [(256, 64, 2), (48 * 32, 192, 6), (300, 192, 6), (300, 64, 2)]     # N: one block of 256 tokens, six, two (the second partial)
CAB = {}


def cab_case(n, c, cs):
    """t, conv [2, n, c] (fp16 values) and ChannelAttention's two 1x1 convs."""
    if (n, c, cs) not in CAB:
        seed = 8000 + n + c
        CAB[(n, c, cs)] = dict(t=r16(seeded((2, n, c), seed)), conv=r16(seeded((2, n, c), seed + 1) + 0.3 * seeded((2, 1, c), seed + 6)),
                               w1=seeded((cs, c), seed + 2, 3.0 / math.sqrt(c)), b1=seeded((cs,), seed + 3, 0.2),
                               w3=seeded((c, cs), seed + 4, 2.0 / math.sqrt(cs)), b3=seeded((c,), seed + 5, 0.2))
    return CAB[(n, c, cs)]


def gate_ref(case):
    hid = torch.relu(case["conv"].double().mean(1) @ case["w1"].double().t() + case["b1"].double())
    return torch.sigmoid(hid @ case["w3"].double().t() + case["b3"].double())


def run_gate(dev, case, ld=None):
    _lib = sub("_lib")
    p = _lib.ptr
    b, n, c = case["conv"].shape
    ld = ld or c
    y = torch.full((b, n, ld), 1e4, dtype=torch.float16)
    y[..., :c] = case["conv"].half()
    hold = [y.to(dev)] + [case[k].float().contiguous().to(dev) for k in ("w1", "b1", "w3", "b3")]
    ws = torch.zeros((b, (n + 255) // 256, c), dtype=torch.float32).to(dev)
    gate = torch.full((b, c), 7.0, dtype=torch.float32).to(dev)
    _lib.check(_lib.lib.sdmi_hat_channel_gate(*(p(x) for x in hold), p(ws), p(gate), b, n, c, case["w1"].shape[0], ld, _lib.stream_ptr()),
               "sdmi_hat_channel_gate")
    torch.cuda.synchronize()
    return gate


@pytest.mark.parametrize("n,c,cs", CAB_CASES)
def test_channel_gate_vs_float64(dev, n, c, cs):
    case = cab_case(n, c, cs)
    got, ref = run_gate(dev, case), gate_ref(case)
    err = rel_l2(got.cpu(), ref)
    print(f"[hat parity] channel gate N {n} C {c}: engine {err:.3e} (fp32 out: bound 1e-5)")
    assert err < 1e-5 and float(ref.std()) > 0.05
    assert torch.equal(got.cpu(), run_gate(dev, case).cpu())                             # fixed-order sums: two runs give the same bits
    assert torch.equal(got.cpu(), run_gate(dev, case, ld=c + 16).cpu())                  # rows wider than the channels


@pytest.mark.parametrize("n,c,cs", CAB_CASES[:3])
def test_cab_add_vs_float64(dev, n, c, cs):
    """out = t + conv_scale * gate[image] * conv, in rows wider than the channels, then with out aliasing t.  conv_scale 0.5 here: at the
    network's 0.01 the term would sit below the sum's own rounding."""
    _lib = sub("_lib")
    p = _lib.ptr
    case = cab_case(n, c, cs)
    gate = run_gate(dev, case)
    ref = case["t"].double() + 0.5 * gate_ref(case)[:, None] * case["conv"].double()
    t, conv = case["t"].half().to(dev), case["conv"].half().to(dev)
    out = torch.full((2, n, c + 8), 3.0, dtype=torch.float16).to(dev)
    _lib.check(_lib.lib.sdmi_hat_cab_add(p(t), p(conv), p(gate), p(out), 2 * n, n, c, c, c, c + 8, 0.5, _lib.stream_ptr()), "sdmi_hat_cab_add")
    torch.cuda.synchronize()
    assert bool((out.cpu()[..., c:] == 3).all())
    assert_parity(out.cpu()[..., :c], ref, r16d(ref), 2, (0, 1), f"cab_add N {n} C {c}")
    alias = t.clone()
    _lib.check(_lib.lib.sdmi_hat_cab_add(p(alias), p(conv), p(gate), p(alias), 2 * n, n, c, c, c, c, 0.5, _lib.stream_ptr()), "sdmi_hat_cab_add")
    torch.cuda.synchronize()
    assert same_bits(alias, out[..., :c].contiguous())


def test_channel_gate_and_cab_add_refusals(dev):
    _lib = sub("_lib")
    L, s = _lib.lib, _lib.stream_ptr()

    def p(t):
        return t.data_ptr()
    y = torch.zeros((1, 64, 72), dtype=torch.float16).to(dev)
    w1, b1 = torch.zeros((2, 64), dtype=torch.float32).to(dev), torch.zeros(2, dtype=torch.float32).to(dev)
    w3, b3 = torch.zeros((64, 2), dtype=torch.float32).to(dev), torch.zeros(64, dtype=torch.float32).to(dev)
    ws, gate = torch.full((1, 1, 64), 7.0, dtype=torch.float32).to(dev), torch.full((1, 64), 7.0, dtype=torch.float32).to(dev)
    good = dict(y=p(y), w1=p(w1), b1=p(b1), w3=p(w3), b3=p(b3), ws=p(ws), gate=p(gate), B=1, N=64, C=64, Cs=2, ld=72)
    for kw, msg in [(dict(y=None), "null"), (dict(w3=None), "null"), (dict(gate=None), "null"), (dict(B=0), "empty"), (dict(N=0), "empty"),
                    (dict(C=60), "multiple of 8"), (dict(C=1032), "multiple of 8"), (dict(Cs=0), "squeezed width"), (dict(Cs=129), "squeezed width"),
                    (dict(ld=56), "narrower"), (dict(ld=68), "misaligned"), (dict(y=p(y) + 2), "misaligned"), (dict(b1=p(b1) + 2), "misaligned")]:
        a = dict(good, **kw)
        assert L.sdmi_hat_channel_gate(a["y"], a["w1"], a["b1"], a["w3"], a["b3"], a["ws"], a["gate"], a["B"], a["N"], a["C"], a["Cs"], a["ld"], s) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    out = torch.full((1, 64, 72), 7.0, dtype=torch.float16).to(dev)
    good = dict(t=p(y), conv=p(y) + 16, gate=p(gate), out=p(out), rows=64, rpi=64, C=64, ldt=72, ldc=72, ldo=72)
    for kw, msg in [(dict(t=None), "null"), (dict(out=None), "null"), (dict(gate=None), "null"), (dict(rows=0), "multiple of rows_per_image"),
                    (dict(rows=65), "multiple of rows_per_image"), (dict(rpi=0), "multiple of rows_per_image"), (dict(C=60), "multiple of 8"),
                    (dict(C=0), "multiple of 8"), (dict(ldt=56), "narrower"), (dict(ldo=68, C=8), "misaligned"), (dict(t=p(y) + 2), "misaligned"),
                    (dict(gate=p(gate) + 2), "misaligned"), (dict(out=p(y) + 16), "alias")]:
        a = dict(good, **kw)
        assert L.sdmi_hat_cab_add(a["t"], a["conv"], a["gate"], a["out"], a["rows"], a["rpi"], a["C"], a["ldt"], a["ldc"], a["ldo"], 0.01, s) != 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((ws.cpu() == 7).all()) and bool((gate.cpu() == 7).all()) and bool((out.cpu() == 7).all())


# ---- network level ----------------------------------------------------------------------------------------------------------------
NET_CASES = {                                                      # name: (make_state_dict keywords, (b, h, w))
    "x2-c60": (dict(embed_dim=60, depths=(2,), heads=6, compress_ratio=3, squeeze_factor=30, mlp_ratio=2, scale=2), (2, 24, 40)),     # pads to 32 x 48
    "x3-c48": (dict(embed_dim=48, depths=(2, 1), heads=2, compress_ratio=24, squeeze_factor=24, mlp_ratio=2, scale=3), (1, 32, 32)),  # HAT-S's ratios
    "x4-c60": (dict(embed_dim=60, depths=(3,), heads=6, compress_ratio=3, squeeze_factor=30, mlp_ratio=2, scale=4), (1, 17, 33)),
    "x4-c180": (dict(embed_dim=180, depths=(2, 2), heads=6, compress_ratio=3, squeeze_factor=30, mlp_ratio=2, scale=4), (1, 32, 32)),  # the true width
}
NETS, REFS, ENGINE = {}, {}, []


def shared_engine():
    if not ENGINE:
        ENGINE.append(sub("engine").Engine(0))
    return ENGINE[0]


def state_dict_for(name, **kw):
    return R.make_state_dict(**dict(NET_CASES[name][0], **kw))


def net_for(name):
    if name not in NETS:
        sd = state_dict_for(name)
        NETS[name] = (sd, sub("upscaler").HATNet(sd, device=0, engine=shared_engine()))
    return NETS[name]


def reference_for(name):
    """(x, fp32 reference, fp16-storage twin) of a case: computed once, shared, never modified."""
    if name not in REFS:
        kw, (b, h, w) = NET_CASES[name]
        sd = state_dict_for(name)
        x = R.image(b, h, w, 50 + kw["scale"] + kw["embed_dim"])
        REFS[name] = (x, R.forward(sd, x), R.fp16_twin(sd, x))
    return REFS[name]


@pytest.mark.parametrize("name", list(NET_CASES))
def test_hat_network_vs_reference(dev, name):
    kw, (b, h, w) = NET_CASES[name]
    sd, net = net_for(name)
    s = kw["scale"]
    assert net.scale == s and net.config == R.config_of(sd)
    x, ref, twin = reference_for(name)
    got = net.run(x.to(dev))
    assert got.shape == (b, 3, h * s, w * s) and got.dtype == torch.float32
    assert 0 < net.scratch_bytes(b, h, w) <= net.engine.arena_bytes()
    assert_parity(got, ref, twin, 1, (0, 2), f"network {name} {b}x{h}x{w}")


def test_the_other_index_layout_is_the_same_network(dev):
    """The same function stored through the plain OCA index (another table order in the checkpoint): the loader follows the buffer, the
    engine gives the same bits."""
    name = "x2-c60"
    sd, net = net_for(name)
    plain = state_dict_for(name, index_layout="plain")
    o = "layers.0.residual_group.overlap_attn.relative_position_bias_table"
    assert not torch.equal(plain[o], sd[o]) and not torch.equal(plain["relative_position_index_OCA"], sd["relative_position_index_OCA"])
    other = sub("upscaler").HATNet(plain, device=0, engine=shared_engine())
    x = reference_for(name)[0].to(dev)
    assert torch.equal(other.run(x).cpu(), net.run(x).cpu())
    other.close()


def test_hat_run_takes_the_arena_its_scratch_bytes_sizes(dev):
    """Sizing and running are one walk over the arena: on an engine that has run nothing, one run leaves the arena at what
    sdmi_hat_scratch_bytes reports, grown by the engine's rule (csrc/engine.cpp ensure_arena: need + need / 16 + 1 MiB)."""
    name = "x3-c48"
    kw, (b, h, w) = NET_CASES[name]
    engine = sub("engine").Engine(0)
    net = sub("upscaler").HATNet(state_dict_for(name), device=0, engine=engine)
    assert engine.arena_bytes() == 0
    got = net.run(reference_for(name)[0].to(dev))
    n = net.scratch_bytes(b, h, w)
    assert got.shape == (b, 3, h * 3, w * 3) and 0 < n
    assert engine.arena_bytes() == n + (n >> 4) + (1 << 20)
    net.close()


@pytest.mark.parametrize("name", ["x2-c60", "x4-c60"])
def test_hat_uint8_in_and_out(dev, name):
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
    c = _lib.HATConfigC()
    c.embed_dim, c.num_layers, c.num_heads, c.mlp_hidden, c.scale = cfg["embed_dim"], len(cfg["depths"]), cfg["num_heads"], cfg["mlp_hidden"], cfg["scale"]
    c.cab_mid, c.cab_squeeze, c.conv_scale = cfg["cab_mid"], cfg["cab_squeeze"], cfg["conv_scale"]
    for i, d in enumerate(cfg["depths"]):
        c.depths[i] = d
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_hat_handle_entries_directly(dev):
    """The C entries by name: blob_floats, create (and what it refuses), scratch_bytes, run (and a side below 9), destroy."""
    _lib, up = sub("_lib"), sub("upscaler")
    L = _lib.lib
    name = "x3-c48"
    sd = state_dict_for(name)
    blob, config = up.parse_hat_state_dict(sd)
    eng = shared_engine()
    assert L.sdmi_hat_blob_floats(ctypes.byref(config_c(sd))) == blob.size
    for other in NET_CASES:
        sd2 = state_dict_for(other)
        assert L.sdmi_hat_blob_floats(ctypes.byref(config_c(sd2))) == up.parse_hat_state_dict(sd2)[0].size, other
    refused = [(dict(num_heads=5), "multiple of num_heads"), (dict(num_heads=0), "multiple of num_heads"), (dict(embed_dim=96, num_heads=2), "<= 32"),
               (dict(embed_dim=2048, num_heads=64), "<= 1024"), (dict(mlp_hidden=0), "mlp_hidden"), (dict(cab_mid=0), "cab_mid"), (dict(cab_mid=65), "cab_mid"),
               (dict(cab_squeeze=0), "cab_squeeze"), (dict(cab_squeeze=129), "cab_squeeze"), (dict(conv_scale=float("nan")), "conv_scale"),
               (dict(scale=5), "scale 2 | 3 | 4"), (dict(scale=1), "scale 2 | 3 | 4"), (dict(num_layers=17), "num_layers"), (dict(num_layers=0), "num_layers")]
    for kw, msg in refused:
        assert L.sdmi_hat_blob_floats(ctypes.byref(config_c(sd, **kw))) == 0, kw
        assert not L.sdmi_hat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd, **kw))), kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert not L.sdmi_hat_create(eng.handle, blob.ctypes.data, blob.size - 1, ctypes.byref(config_c(sd)))
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_hat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd, scale=4)))      # another tail: another length
    assert "blob size" in _lib.last_error()
    assert not L.sdmi_hat_create(eng.handle, None, blob.size, ctypes.byref(config_c(sd)))
    h = L.sdmi_hat_create(eng.handle, blob.ctypes.data, blob.size, ctypes.byref(config_c(sd)))
    assert h, _lib.last_error()
    try:
        assert L.sdmi_hat_scratch_bytes(h, 1, 32, 32) > 0
        assert L.sdmi_hat_scratch_bytes(h, 1, 8, 32) == 0
        assert L.sdmi_hat_scratch_bytes(None, 1, 32, 32) == 0
        x, ref, twin = reference_for(name)
        xd = x.to(dev)
        out = torch.full((1, 3, 96, 96), 7.0, dtype=torch.float32).to(dev)
        assert L.sdmi_hat_run(h, _lib.ptr(xd), 0, 1, 8, 32, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        assert "at least 9" in _lib.last_error()
        assert L.sdmi_hat_run(h, None, 0, 1, 32, 32, _lib.ptr(out), 0, _lib.stream_ptr()) != 0
        torch.cuda.synchronize()
        assert bool((out.cpu() == 7).all())
        _lib.check(L.sdmi_hat_run(h, _lib.ptr(xd), 0, 1, 32, 32, _lib.ptr(out), 0, _lib.stream_ptr()), "sdmi_hat_run")
        assert_parity(out, ref, twin, 1, (0, 2), "direct handle, 32x32")
    finally:
        L.sdmi_hat_destroy(h)


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_upscaler_do_upscale_runs_a_hat_checkpoint(dev, tmp_path):
    from PIL import Image
    up = sub("upscaler")
    sd, net = net_for("x2-c60")
    path = str(tmp_path / "tiny_hat_x2.pth")
    torch.save({"params_ema": sd}, path)
    src = np.random.RandomState(5).randint(90, 166, size=(19, 13, 3), dtype=np.uint8)
    scaler = up.UpscalerESRGAN(0, engine=shared_engine())
    img = scaler.do_upscale(Image.fromarray(src), path)
    assert isinstance(img, Image.Image) and img.size == (26, 38) and img.mode == "RGB"
    assert len(scaler._nets) == 1 and isinstance(scaler._nets[path], up.HATNet)
    direct = net.run(torch.from_numpy(src[None]).to(dev))[0].cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(img), up.model_output_to_u8(direct))


def test_resize_image_through_a_registered_hat_upscaler(dev, tmp_path, monkeypatch):
    from PIL import Image
    up, shared = sub("upscaler"), sub("shared")
    sd = net_for("x2-c60")[0]
    path = str(tmp_path / "tiny_hat_x2.pth")
    torch.save(sd, path)
    monkeypatch.setattr(shared, "sd_upscalers", [])
    added = up.register_esrgan({"Tiny-HAT 2x": path}, engine=shared_engine())
    assert [d.name for d in shared.sd_upscalers] == ["None", "Lanczos", "Nearest", "Tiny-HAT 2x"] and added[0].scale == 2
    im = Image.fromarray(np.random.RandomState(6).randint(90, 166, size=(16, 24, 3), dtype=np.uint8))
    got = up.resize_image(0, im, 48, 32, "Tiny-HAT 2x")
    assert got.size == (48, 32) and isinstance(added[0].scaler._nets[path], up.HATNet)
    assert np.array_equal(np.asarray(got), np.asarray(added[0].scaler.do_upscale(im, path)))
