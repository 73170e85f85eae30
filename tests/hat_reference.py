"""Plain torch restatement of HAT (Chen et al., "Activating More Pixels in Image Super-Resolution Transformer", CVPR 2023; hat_arch.py
with upsampler 'pixelshuffle', resi_connection '1conv', window_size 16, overlap_ratio 0.5, img_range 1, no ape) — the reference of the HAT
tests (test infrastructure; fp32 / float64 on the CPU).  Restated, unpinned: the original source is not available to the tests; the
parameter names below are the original key layout.  Its parts are pinned to torch in tests/test_cpu_hat.py.

    x = conv_first(reflect_pad_16(img) - mean);  t = patch_embed.norm(tokens(x))
    per group i:  t = t + layers.i.conv(overlap_attn(blocks...(t)))
    t = norm(t);  x = conv_after_body(t) + x
    y = LeakyReLU(0.01)(conv_before_upsample.0(x));  per step y = PixelShuffle(upsample.{0,2}(y));  conv_last(y) + mean;  crop
    HAB j (shift 8 for odd j):
        n = norm1(t);  conv = cab.2(GELU(cab.0(n)));  conv = conv * sigmoid(attention.3(relu(attention.1(mean over pixels of conv))))
        attn = proj(W-MSA_16(qkv(n)))  — roll(-8, -8) when shifted, (q D^-1/2) k^T + table[index_SA] (+ Swin's -100 region mask), softmax, @ v
        t = t + attn + conv_scale * conv;  t = t + fc2(GELU(fc1(norm2(t))))
    OCAB (once per group, after the blocks):
        n = norm1(t);  q, k, v = qkv(n);  q in 16 x 16 windows, k and v in the 24 x 24 windows around them (nn.Unfold(24, stride 16,
        padding 4): zeros outside the grid, put in AFTER the linear, so a padded key scores 0 + bias);
        t = t + proj(softmax((q D^-1/2) k^T + table[index_OCA]) v);  t = t + fc2(GELU(fc1(norm2(t))))

`forward(sd, x, q)` takes a rounding hook q, applied wherever the engine stores fp16 or feeds an MFMA: the mean-subtracted input, every
conv / linear output (after its fused activation, with its residual: one rounding of the sum), LayerNorm outputs, the softmax
probabilities, the attention outputs, the sum that adds the conv branch.  The bias, mask, softmax and the channel gate stay in the working
precision; conv_last's output stays fp32.  `fp16_twin` is q = fp16_emu.r16 with the weights of the layers that run as GEMMs rounded to
fp16 (the channel attention's two 1x1 convs and the bias tables stay fp32, as in the engine)."""
import math

import torch
import torch.nn.functional as F

from dat_reference import shift_mask as _rect_shift_mask, tail  # noqa: F401
from swinir_reference import MEAN, ident, image  # noqa: F401

WS, EXT, PAD = 16, 24, 4                                      # window, overlapping window, its margin
CONV_SCALE = 0.01


def window_partition(x):
    """[B, H, W, C] -> [B * nW, 256, C], windows row-major."""
    b, h, w, c = x.shape
    return x.view(b, h // WS, WS, w // WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, WS * WS, c)


def window_reverse(win, b, h, w):
    c = win.shape[-1]
    return win.view(b, h // WS, w // WS, WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def sa_index():
    """[256, 256]: Swin's index, (ya - yb + 15) * 31 + (xa - xb + 15)."""
    y, x = torch.arange(256) // 16, torch.arange(256) % 16
    return (y[:, None] - y[None, :] + 15) * 31 + (x[:, None] - x[None, :] + 15)


def oca_offsets():
    """([256, 576], [256, 576]): (dy, dx) = (yb - ya, xb - xa) of query a (16 x 16) and key b (24 x 24)."""
    ya, xa = torch.arange(256) // 16, torch.arange(256) % 16
    yb, xb = torch.arange(576) // 24, torch.arange(576) % 24
    return yb[None, :] - ya[:, None], xb[None, :] - xa[:, None]


def oca_index(layout="reference"):
    """[256, 576] relative_position_index_OCA.  "reference": the architecture's (dy + 16 - 24 + 1) * 39 + (dx + 16 - 24 + 1), -880 .. 640
    (negative rows count from the end of the table); "plain": (dy + 15) * 39 + (dx + 15)."""
    dy, dx = oca_offsets()
    return (dy - 7) * 39 + (dx - 7) if layout == "reference" else (dy + 15) * 39 + (dx + 15)


def shift_mask(h, w, value=-100.0):
    """[nW, 256, 256]: Swin's region mask of the shifted grid at window 16, shift 8."""
    return _rect_shift_mask(h, w, WS, WS, value)


_MASKS = {}


def _cached_mask(h, w, value, device, dtype):
    """The mask on the device of the run, built once per size (the original builds it once per input size too)."""
    key = (h, w, value, str(device), dtype)
    if key not in _MASKS:
        _MASKS[key] = shift_mask(h, w, value).to(device, dtype)
    return _MASKS[key]


def window_attention(qkv, table, heads, shift, q=ident, index=None, use_bias=True, use_mask=True, mask_value=-100.0):
    """qkv [B, H, W, 3C] (H, W multiples of 16; already rounded by the caller), table [961, heads] -> [B, H, W, C]."""
    b, h, w, c3 = qkv.shape
    c, n = c3 // 3, WS * WS
    d = c // heads
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    qq, kk, vv = window_partition(x).view(-1, n, 3, heads, d).permute(2, 0, 3, 1, 4)            # [nWB, heads, 256, d]
    s = (qq * d ** -0.5) @ kk.transpose(-2, -1)
    if use_bias:
        index = (sa_index() if index is None else index).to(s.device)
        s = s + table.to(s.dtype)[index.reshape(-1)].view(n, n, heads).permute(2, 0, 1)[None]
    if shift and use_mask:
        m = _cached_mask(h, w, mask_value, s.device, s.dtype)
        s = (s.view(b, m.shape[0], heads, n, n) + m[None, :, None]).view(-1, heads, n, n)
    p = q(torch.softmax(s, dim=-1))
    o = window_reverse(q((p @ vv).transpose(1, 2).reshape(-1, n, c)), b, h, w)
    return torch.roll(o, (shift, shift), (1, 2)) if shift else o


def overlap_windows(x):
    """[B, H, W, C] -> [B * nW, 576, C]: the 24 x 24 windows at stride 16 around the 16 x 16 windows, zeros outside the grid."""
    b, h, w, c = x.shape
    p = F.pad(x, (0, 0, PAD, PAD, PAD, PAD))
    win = p.unfold(1, EXT, WS).unfold(2, EXT, WS)                                                # [B, nwy, nwx, C, 24, 24]
    return win.permute(0, 1, 2, 4, 5, 3).reshape(-1, EXT * EXT, c)


def overlap_attention(qkv, table, heads, q=ident, index=None, use_bias=True, mask_padded_keys=False):
    """qkv [B, H, W, 3C] (already rounded), table [1521, heads] read through index [256, 576] -> [B, H, W, C]."""
    b, h, w, c3 = qkv.shape
    c, n, m = c3 // 3, WS * WS, EXT * EXT
    d = c // heads
    qq = window_partition(qkv[..., :c]).view(-1, n, heads, d).transpose(1, 2)
    kk = overlap_windows(qkv[..., c:2 * c]).view(-1, m, heads, d).transpose(1, 2)
    vv = overlap_windows(qkv[..., 2 * c:]).view(-1, m, heads, d).transpose(1, 2)
    s = (qq * d ** -0.5) @ kk.transpose(-2, -1)
    if use_bias:
        index = (oca_index() if index is None else index).to(s.device)
        s = s + table.to(s.dtype)[index.reshape(-1)].view(n, m, heads).permute(2, 0, 1)[None]
    if mask_padded_keys:
        inside = overlap_windows(torch.ones((b, h, w, 1), dtype=s.dtype))[..., 0] > 0             # [nWB, 576]
        s = s.masked_fill(~inside[:, None, None, :], -math.inf)
    p = q(torch.softmax(s, dim=-1))
    return window_reverse(q((p @ vv).transpose(1, 2).reshape(-1, n, c)), b, h, w)


def _conv(sd, name, x, pad=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)


def channel_gate(sd, pre, y):
    """ChannelAttention's factor of y NCHW -> [B, C, 1, 1]; pre = "...conv_block.cab.3."."""
    z = F.relu(_conv(sd, pre + "attention.1", y.mean((2, 3), keepdim=True), 0))
    return torch.sigmoid(_conv(sd, pre + "attention.3", z, 0))


def cab(sd, pre, n, q=ident):
    """The conv branch of norm1(t) NCHW -> (conv, gate): cab.2(GELU(cab.0(n))) and its channel attention factor; pre = "...conv_block."."""
    y = q(_conv(sd, pre + "cab.2", q(F.gelu(_conv(sd, pre + "cab.0", n)))))
    return y, channel_gate(sd, pre + "cab.3.", y)


def _mlp(sd, pre, x, q):
    c = x.shape[-1]
    y = q(F.layer_norm(x, (c,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-5))
    y = q(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])))
    return q(x + F.linear(y, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"]))


def hab(sd, pre, x, heads, shift, q=ident, conv_scale=CONV_SCALE):
    """One hybrid attention block on [B, H, W, C]; pre = "layers.i.residual_group.blocks.j."."""
    c = x.shape[-1]
    n = q(F.layer_norm(x, (c,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    qkv = q(F.linear(n, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]))
    att = window_attention(qkv, sd[pre + "attn.relative_position_bias_table"], heads, shift, q, sd.get("relative_position_index_SA"))
    x = q(x + F.linear(att, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"]))
    conv, gate = cab(sd, pre + "conv_block.", n.permute(0, 3, 1, 2), q)
    x = q(x + conv_scale * (conv * gate).permute(0, 2, 3, 1))
    return _mlp(sd, pre, x, q)


def ocab(sd, pre, x, heads, q=ident):
    """The overlapping cross-attention block on [B, H, W, C]; pre = "layers.i.residual_group.overlap_attn."."""
    c = x.shape[-1]
    n = q(F.layer_norm(x, (c,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    qkv = q(F.linear(n, sd[pre + "qkv.weight"], sd[pre + "qkv.bias"]))
    att = overlap_attention(qkv, sd[pre + "relative_position_bias_table"], heads, q, sd.get("relative_position_index_OCA"))
    x = q(x + F.linear(att, sd[pre + "proj.weight"], sd[pre + "proj.bias"]))
    return _mlp(sd, pre, x, q)


def config_of(sd, conv_scale=CONV_SCALE):
    c = sd["conv_first.weight"].shape[0]
    depths = []
    while f"layers.{len(depths)}.residual_group.blocks.0.norm1.weight" in sd:
        i, j = len(depths), 0
        while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    b0 = "layers.0.residual_group.blocks.0."
    scale = 4 if "upsample.2.weight" in sd else (3 if sd["upsample.0.weight"].shape[0] == 576 else 2)
    return dict(embed_dim=c, depths=tuple(depths), num_heads=sd[b0 + "attn.relative_position_bias_table"].shape[1],
                mlp_hidden=sd[b0 + "mlp.fc1.weight"].shape[0], cab_mid=sd[b0 + "conv_block.cab.0.weight"].shape[0],
                cab_squeeze=sd[b0 + "conv_block.cab.3.attention.1.weight"].shape[0], conv_scale=float(conv_scale), scale=scale)


def forward(sd, x, q=ident, conv_scale=CONV_SCALE):
    """x [B, 3, H, W] in [0, 1] (H, W >= 9) -> [B, 3, H s, W s], in the dtype of x and the state dict."""
    cfg = config_of(sd)
    heads, s = cfg["num_heads"], cfg["scale"]
    h, w = x.shape[2:]
    mean = torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    x = F.pad(x, (0, -w % WS, 0, -h % WS), mode="reflect")
    f = q(_conv(sd, "conv_first", q(x - mean)))
    c = f.shape[1]
    t = q(F.layer_norm(f.permute(0, 2, 3, 1), (c,), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], 1e-5))
    for i, depth in enumerate(cfg["depths"]):
        y = t
        for j in range(depth):
            y = hab(sd, f"layers.{i}.residual_group.blocks.{j}.", y, heads, 8 if j % 2 else 0, q, conv_scale)
        y = ocab(sd, f"layers.{i}.residual_group.overlap_attn.", y, heads, q)
        t = q(_conv(sd, f"layers.{i}.conv", y.permute(0, 3, 1, 2)) + t.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    t = q(F.layer_norm(t, (c,), sd["norm.weight"], sd["norm.bias"], 1e-5))
    f = q(_conv(sd, "conv_after_body", t.permute(0, 3, 1, 2)) + f)
    return (tail(sd, f, s, q) + mean)[:, :, :h * s, :w * s].contiguous()


def round_weights(sd):
    """The weights of the layers that run as GEMMs rounded to fp16: every conv / linear but the channel attention's two 1x1 convs."""
    from fp16_emu import r16
    return {k: (r16(v) if k.endswith(".weight") and v.dim() >= 2 and ".attention." not in k else v) for k, v in sd.items()}


def fp16_twin(sd, x, conv_scale=CONV_SCALE):
    from fp16_emu import r16
    return forward(round_weights(sd), x, r16, conv_scale)


def make_state_dict(embed_dim=60, depths=(2,), heads=6, compress_ratio=3, squeeze_factor=30, mlp_ratio=2, scale=4, index_layout="reference", seed=0):
    """Seeded weights in the original key layout with the two index buffers.  The overlap block's table is drawn in offset order and stored
    through the layout's index, so the two layouts ("reference" | "plain") are the same function in two different checkpoints."""
    g = torch.Generator().manual_seed(0x48 + 977 * seed + 31 * embed_dim + 7 * sum(depths) + 3 * heads + scale + 13 * compress_ratio + 1000 * int(mlp_ratio))
    c, hid, mid, sq, sd = embed_dim, int(mlp_ratio * embed_dim), embed_dim // compress_ratio, embed_dim // squeeze_factor, {}

    def lin(name, o, i, k=0, gain=1.0, bias=0.05):              # k = 0: a Linear [o, i]; k = 1 | 3: a conv [o, i, k, k]
        fan = i * max(k, 1) ** 2
        sd[name + ".weight"] = torch.randn((o, i) if k == 0 else (o, i, k, k), generator=g) * gain / math.sqrt(fan)
        sd[name + ".bias"] = torch.randn((o,), generator=g) * bias

    def norm(name):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn((c,), generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn((c,), generator=g)

    dy, dx = oca_offsets()
    plain, stored = ((dy + 15) * 39 + (dx + 15)).reshape(-1), oca_index(index_layout).reshape(-1)
    lin("conv_first", c, 3, 3, 4.0)
    norm("patch_embed.norm")
    sd["relative_position_index_SA"] = sa_index()
    sd["relative_position_index_OCA"] = oca_index(index_layout)
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            norm(b + "norm1")
            sd[b + "attn.relative_position_bias_table"] = 0.5 * torch.randn((961, heads), generator=g)
            lin(b + "attn.qkv", 3 * c, c, gain=1.5)
            lin(b + "attn.proj", c, c, gain=0.7)
            lin(b + "conv_block.cab.0", mid, c, 3, 1.5)
            lin(b + "conv_block.cab.2", c, mid, 3, 3.0)
            lin(b + "conv_block.cab.3.attention.1", sq, c, 1, 3.0, bias=0.2)
            lin(b + "conv_block.cab.3.attention.3", c, sq, 1, 2.0, bias=0.2)
            if j % 2:
                sd[b + "attn_mask"] = shift_mask(64, 64)
            norm(b + "norm2")
            lin(b + "mlp.fc1", hid, c)
            lin(b + "mlp.fc2", c, hid, gain=0.7)
        o = f"layers.{i}.residual_group.overlap_attn."
        norm(o + "norm1")
        lin(o + "qkv", 3 * c, c, gain=1.5)
        by_offset = 0.5 * torch.randn((1521, heads), generator=g)
        table = torch.zeros((1521, heads))
        table[stored] = by_offset[plain]                         # negative rows count from the end
        sd[o + "relative_position_bias_table"] = table
        lin(o + "proj", c, c, gain=0.7)
        norm(o + "norm2")
        lin(o + "mlp.fc1", hid, c)
        lin(o + "mlp.fc2", c, hid, gain=0.7)
        lin(f"layers.{i}.conv", c, c, 3, 0.5)
    norm("norm")
    lin("conv_after_body", c, c, 3, 1.0)
    lin("conv_before_upsample.0", 64, c, 3, 1.0)
    f2 = 9 if scale == 3 else 4
    for k in ((0, 2) if scale == 4 else (0,)):
        lin(f"upsample.{k}", f2 * 64, 64, 3, 1.0)
    lin("conv_last", 3, 64, 3, 0.15, bias=0.02)
    return sd

