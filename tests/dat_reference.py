"""Plain torch restatement of DAT (Chen et al., "Dual Aggregation Transformer for Image Super-Resolution", ICCV 2023; basicsr's
dat_arch.py with upsampler 'pixelshuffle' and resi_connection '1conv') — the reference of the DAT tests (test infrastructure; fp32 /
float64 on the CPU).  Restated, unpinned: the original source is not available to the tests; the parameter names below are the original
key layout.

    x = conv_first(x - mean);  t = before_RG.1(tokens(x))                                    (a LayerNorm)
    t = t + layers.i.conv(blocks_i(t))                                                       for every residual group i
    x = conv_after_body(norm(t)) + x
    y = LeakyReLU(0.01)(conv_before_upsample.0(x));  per step y = PixelShuffle(upsample.{0,2}(y));  conv_last(y) + mean
    block j:  x = x + attn(norm1(x));  x = x + ffn(norm2(x));  even j: adaptive spatial attention, odd j: adaptive channel attention
    spatial:  qkv = Linear(C, 3C);  the q, k, v grids zero-padded right / bottom to multiples of max(split) AFTER the linear (padded tokens
              are q = k = v = 0; they are keys, score 0 + bias);  branch 0 = channels [0, C/2) in windows split[0] x split[1], branch 1 =
              channels [C/2, C) in windows split[1] x split[0], heads / 2 heads each;  shifted blocks roll each branch by minus half its
              window on the padded grid and add Swin's region mask (-100) of the padded grid;
              softmax((q D^-1/2) k^T + pos(offsets)[index] + mask) v;  crop, concatenate -> att
              conv = GELU(BN(dwconv3x3(v as image)));  cmap = channel_interaction(conv);  smap = spatial_interaction(att)
              out = proj(att sigmoid(cmap) + sigmoid(smap) conv)
    channel:  per head q, k, v [d, N];  A = softmax(temperature normalize(q) normalize(k)^T);  att = A v
              cmap = channel_interaction(att);  smap = spatial_interaction(conv);  out = proj(att sigmoid(smap) + conv sigmoid(cmap))
    ffn:      x1 | x2 = GELU(fc1(x));  fc2(x1 * dwconv3x3(LayerNorm(x2)))
    shifted:  (i even and j > 0 and (j - 2) % 4 == 0) or (i odd and j % 4 == 0)

`forward(sd, x, q)` takes a rounding hook q, applied wherever the engine stores fp16 or feeds an MFMA: the mean-subtracted input, every
conv / linear output (after its fused activation, with its residual: one rounding of the sum), LayerNorm outputs, q / k / v, the softmax
probabilities of both attentions (the channel attention's matrix is stored as fp16), the attention outputs, GELU(BN(dwconv)), the AIM
sum, the feed-forward gate product.  The position bias, BatchNorms, gates and softmax stay in the working precision; conv_last's output
stays fp32.  `fp16_twin` is q = fp16_emu.r16 with the weights of the layers that run as GEMMs rounded to fp16 (the depthwise convs, the
interaction MLPs and the position MLP stay fp32, as in the engine)."""
import math

import torch
import torch.nn.functional as F

from swinir_reference import MEAN, ident, image  # noqa: F401

BN_EPS = 1e-5


def is_shifted(i, j):
    return j % 2 == 0 and ((i % 2 == 0 and j > 0 and (j - 2) % 4 == 0) or (i % 2 == 1 and j % 4 == 0))


def relative_position_index(hs, ws):
    """[N, N]: index[a][b] = (ya - yb + hs - 1)(2 ws - 1) + (xa - xb + ws - 1) for window-local tokens a, b (row-major, hs x ws)."""
    coords = torch.stack(torch.meshgrid(torch.arange(hs), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0)
    return (rel[..., 0] + hs - 1) * (2 * ws - 1) + rel[..., 1] + ws - 1


def offsets(hs, ws, dtype=torch.float32):
    """[(2 hs - 1)(2 ws - 1), 2]: (dy, dx), dy in [1 - hs, hs - 1] outer, dx in [1 - ws, ws - 1] inner."""
    dy, dx = torch.meshgrid(torch.arange(1 - hs, hs), torch.arange(1 - ws, ws), indexing="ij")
    return torch.stack([dy.flatten(), dx.flatten()], dim=1).to(dtype)


def position_bias(sd, pre, hs, ws):
    """pos3(pos2(pos1(pos_proj(offsets)))) -> [(2 hs - 1)(2 ws - 1), heads / 2]; pre = "...attn.attns.k.pos."; posK = LayerNorm, ReLU, Linear."""
    w = sd[pre + "pos_proj.weight"]
    x = F.linear(offsets(hs, ws, w.dtype).to(w.device), w, sd[pre + "pos_proj.bias"])
    for k in ("pos1", "pos2", "pos3"):
        x = F.relu(F.layer_norm(x, (x.shape[-1],), sd[pre + k + ".0.weight"], sd[pre + k + ".0.bias"], 1e-5))
        x = F.linear(x, sd[pre + k + ".2.weight"], sd[pre + k + ".2.bias"])
    return x


def window_partition(x, hs, ws):
    """[B, H, W, C] -> [B * nW, hs * ws, C], windows row-major."""
    b, h, w, c = x.shape
    return x.view(b, h // hs, hs, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, hs * ws, c)


def window_reverse(win, b, h, w, hs, ws):
    c = win.shape[-1]
    return win.view(b, h // hs, w // ws, hs, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def region_ids(h, w, hs, ws):
    """[h, w] id image of the SHIFTED padded grid: 3 r(y) + r(x), the slices [0, -s), [-s, -s/2), [-s/2, end) with s = hs | ws."""
    img = torch.zeros((h, w))
    cnt = 0
    for a in (slice(0, -hs), slice(-hs, -(hs // 2)), slice(-(hs // 2), None)):
        for b in (slice(0, -ws), slice(-ws, -(ws // 2)), slice(-(ws // 2), None)):
            img[a, b] = cnt
            cnt += 1
    return img


def shift_mask(h, w, hs, ws, value=-100.0):
    """[nW, N, N]: `value` where the region ids of two tokens of a window differ, else 0."""
    ids = window_partition(region_ids(h, w, hs, ws)[None, :, :, None], hs, ws).squeeze(-1)
    diff = ids[:, None, :] - ids[:, :, None]
    return torch.where(diff != 0, torch.tensor(float(value)), torch.tensor(0.0))


_BUFFERS = {}


def _cached(kind, hs, ws, device, dtype, make):
    """relative_position_index / shift_mask on the device of the run, built once per size (the original keeps them as buffers)."""
    key = (kind, hs, ws, str(device), dtype)
    if key not in _BUFFERS:
        _BUFFERS[key] = make().to(device) if dtype is None else make().to(device, dtype)
    return _BUFFERS[key]


def branch_attention(qkv, table, heads, hs, ws, shifted, q=ident):
    """One branch on its half of the channels: qkv [3, B, Hp, Wp, Cb] on the padded grid, table [(2 hs - 1)(2 ws - 1), heads] -> [B, Hp, Wp, Cb]."""
    _, b, hp, wp, cb = qkv.shape
    d = cb // heads
    if shifted:
        qkv = torch.roll(qkv, (-(hs // 2), -(ws // 2)), (2, 3))
    qq, kk, vv = (window_partition(t, hs, ws).view(-1, hs * ws, heads, d).transpose(1, 2) for t in qkv)       # [nWB, heads, N, d]
    s = (qq * d ** -0.5) @ kk.transpose(-2, -1)
    n = hs * ws
    index = _cached("index", hs, ws, s.device, None, lambda: relative_position_index(hs, ws).view(-1))
    s = s + table.to(s.dtype)[index].view(n, n, heads).permute(2, 0, 1)[None]
    if shifted:
        m = _cached(("mask", hp, wp), hs, ws, s.device, s.dtype, lambda: shift_mask(hp, wp, hs, ws))
        s = (s.view(b, m.shape[0], heads, n, n) + m[None, :, None]).view(-1, heads, n, n)
    p = q(torch.softmax(s, dim=-1))
    o = q((p @ vv).transpose(1, 2).reshape(-1, n, cb))
    o = window_reverse(o, b, hp, wp, hs, ws)
    return torch.roll(o, (hs // 2, ws // 2), (1, 2)) if shifted else o


def spatial_attention(qkv, tables, heads, split, shifted, q=ident):
    """qkv [B, H, W, 3C] (already rounded by the caller), tables = (branch 0's, branch 1's) -> att [B, H, W, C]."""
    b, h, w, c3 = qkv.shape
    c, big = c3 // 3, max(split)
    t = F.pad(qkv, (0, 0, 0, -w % big, 0, -h % big))                             # zeros AFTER the linear
    t = t.view(b, t.shape[1], t.shape[2], 3, c).permute(3, 0, 1, 2, 4)
    o0 = branch_attention(t[..., :c // 2], tables[0], heads // 2, split[0], split[1], shifted, q)
    o1 = branch_attention(t[..., c // 2:], tables[1], heads // 2, split[1], split[0], shifted, q)
    return torch.cat([o0, o1], dim=-1)[:, :h, :w].contiguous()


def channel_attention(qkv, temperature, heads, q=ident):
    """qkv [B, N, 3C] (already rounded) -> att [B, N, C]: A = softmax(temperature normalize(q) normalize(k)^T) over the channels of a head."""
    b, n, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    qq, kk, vv = qkv.view(b, n, 3, heads, d).permute(2, 0, 3, 4, 1)              # [B, heads, d, N]
    a = (F.normalize(qq, dim=-1) @ F.normalize(kk, dim=-1).transpose(-2, -1)) * temperature.to(qq.dtype).view(1, heads, 1, 1)
    a = q(torch.softmax(a, dim=-1))
    return q((a @ vv).permute(0, 3, 1, 2).reshape(b, n, c))


def batchnorm(sd, name, x):
    w, b, m, v = (sd[name + k].view(1, -1, 1, 1) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    return (x - m) / torch.sqrt(v + BN_EPS) * w + b


def aim_conv(sd, pre, v_img, q=ident):
    """GELU(BN(dwconv3x3(v))) on NCHW."""
    c = v_img.shape[1]
    return q(F.gelu(batchnorm(sd, pre + "attn.dwconv.1", F.conv2d(v_img, sd[pre + "attn.dwconv.0.weight"], sd[pre + "attn.dwconv.0.bias"], padding=1, groups=c))))


def channel_interaction(sd, pre, x):
    """NCHW -> [B, C, 1, 1]: pool, Conv1x1 C -> C/8, BN, GELU, Conv1x1 C/8 -> C."""
    p = pre + "attn.channel_interaction."
    y = F.conv2d(x.mean((2, 3), keepdim=True), sd[p + "1.weight"], sd[p + "1.bias"])
    return F.conv2d(F.gelu(batchnorm(sd, p + "2", y)), sd[p + "4.weight"], sd[p + "4.bias"])


def spatial_interaction(sd, pre, x):
    """NCHW -> [B, 1, H, W]: Conv1x1 C -> C/16, BN, GELU, Conv1x1 C/16 -> 1."""
    p = pre + "attn.spatial_interaction."
    y = F.conv2d(x, sd[p + "0.weight"], sd[p + "0.bias"])
    return F.conv2d(F.gelu(batchnorm(sd, p + "1", y)), sd[p + "3.weight"], sd[p + "3.bias"])


def aim(sd, pre, att, conv, spatial, q=ident):
    """att, conv NCHW -> the tensor proj reads, NCHW."""
    if spatial:
        return q(att * torch.sigmoid(channel_interaction(sd, pre, conv)) + torch.sigmoid(spatial_interaction(sd, pre, att)) * conv)
    return q(att * torch.sigmoid(spatial_interaction(sd, pre, conv)) + conv * torch.sigmoid(channel_interaction(sd, pre, att)))


def sgfn(sd, pre, x, q=ident):
    """fc2(x1 * dwconv(LayerNorm(x2))) of [B, H, W, C], before the residual add (the caller rounds the sum)."""
    y = q(F.gelu(F.linear(x, sd[pre + "ffn.fc1.weight"], sd[pre + "ffn.fc1.bias"])))
    half = y.shape[-1] // 2
    x1, x2 = y[..., :half], y[..., half:]
    x2 = q(F.layer_norm(x2, (half,), sd[pre + "ffn.sg.norm.weight"], sd[pre + "ffn.sg.norm.bias"], 1e-5))
    x2 = F.conv2d(x2.permute(0, 3, 1, 2), sd[pre + "ffn.sg.conv.weight"], sd[pre + "ffn.sg.conv.bias"], padding=1, groups=half).permute(0, 2, 3, 1)
    return F.linear(q(x1 * x2), sd[pre + "ffn.fc2.weight"], sd[pre + "ffn.fc2.bias"])


def block(sd, pre, x, heads, split, spatial, shifted, q=ident):
    """One block on [B, H, W, C]; pre = "layers.i.blocks.j."."""
    b, h, w, c = x.shape
    y = q(F.layer_norm(x, (c,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    qkv = q(F.linear(y, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]))
    v_img = qkv[..., 2 * c:].permute(0, 3, 1, 2)
    if spatial:
        tables = (position_bias(sd, pre + "attn.attns.0.pos.", split[0], split[1]), position_bias(sd, pre + "attn.attns.1.pos.", split[1], split[0]))
        att = spatial_attention(qkv, tables, heads, split, shifted, q)
    else:
        att = channel_attention(qkv.view(b, h * w, 3 * c), sd[pre + "attn.temperature"].reshape(-1), heads, q).view(b, h, w, c)
    mix = aim(sd, pre, att.permute(0, 3, 1, 2), aim_conv(sd, pre, v_img, q), spatial, q).permute(0, 2, 3, 1)
    x = q(x + F.linear(mix, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"]))
    y = q(F.layer_norm(x, (c,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-5))
    return q(x + sgfn(sd, pre, y, q))


def config_of(sd):
    c = sd["conv_first.weight"].shape[0]
    depths = []
    while f"layers.{len(depths)}.blocks.0.norm1.weight" in sd:
        i, j = len(depths), 0
        while f"layers.{i}.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    rows = sd["layers.0.blocks.0.attn.attns.0.rpe_biases"].shape[0]
    split = {15 * 31: (8, 16), 15 * 63: (8, 32)}[rows]
    heads = 2 * sd["layers.0.blocks.0.attn.attns.0.pos.pos3.2.weight"].shape[0]
    scale = 4 if "upsample.2.weight" in sd else (3 if sd["upsample.0.weight"].shape[0] == 576 else 2)
    return dict(embed_dim=c, depths=tuple(depths), num_heads=heads, split=split, ffn_hidden=sd["layers.0.blocks.0.ffn.fc1.weight"].shape[0],
                scale=scale)


def _conv(sd, name, x, pad=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)


def forward(sd, x, q=ident):
    """x [B, 3, H, W] in [0, 1] -> [B, 3, H s, W s], in the dtype of x and the state dict."""
    cfg = config_of(sd)
    heads, s, split = cfg["num_heads"], cfg["scale"], cfg["split"]
    mean = torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    f = q(_conv(sd, "conv_first", q(x - mean)))
    c = f.shape[1]
    t = q(F.layer_norm(f.permute(0, 2, 3, 1), (c,), sd["before_RG.1.weight"], sd["before_RG.1.bias"], 1e-5))
    for i, depth in enumerate(cfg["depths"]):
        y = t
        for j in range(depth):
            y = block(sd, f"layers.{i}.blocks.{j}.", y, heads, split, j % 2 == 0, is_shifted(i, j), q)
        t = q(_conv(sd, f"layers.{i}.conv", y.permute(0, 3, 1, 2)) + t.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    t = q(F.layer_norm(t, (c,), sd["norm.weight"], sd["norm.bias"], 1e-5))
    f = q(_conv(sd, "conv_after_body", t.permute(0, 3, 1, 2)) + f)
    return (tail(sd, f, s, q) + mean).contiguous()


def tail(sd, f, s, q=ident):
    """The pixelshuffle upsampler: conv_before_upsample.0 + LeakyReLU(0.01), per step a conv 64 -> 4 * 64 (9 * 64 for x3) + PixelShuffle, conv_last."""
    y = q(F.leaky_relu(q(_conv(sd, "conv_before_upsample.0", f)), 0.01))
    for k in ((0, 2) if s == 4 else (0,)):
        y = F.pixel_shuffle(q(_conv(sd, f"upsample.{k}", y)), 3 if s == 3 else 2)
    return _conv(sd, "conv_last", y)


GEMM_LAYERS = ("conv_first", "attn.qkv", "attn.proj", "ffn.fc1", "ffn.fc2", "conv_after_body", "conv_before_upsample.0", "upsample.0", "upsample.2",
               "conv_last")


def round_weights(sd):
    """The weights of the layers that run as GEMMs rounded to fp16: the convs, qkv, proj, fc1, fc2, the groups' convs."""
    from fp16_emu import r16

    def gemm(k):
        stem = k[:-len(".weight")]
        return k.endswith(".weight") and (stem in GEMM_LAYERS or any(stem.endswith("." + n) for n in GEMM_LAYERS) or
                                          (stem.startswith("layers.") and stem.endswith(".conv") and ".sg." not in stem))
    return {k: (r16(v) if gemm(k) else v) for k, v in sd.items()}


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward(round_weights(sd), x, r16)


def make_state_dict(embed_dim=60, depths=(4, 2), heads=6, split=(8, 16), expansion=2, scale=4, seed=0):
    g = torch.Generator().manual_seed(0x53 + 977 * seed + 31 * embed_dim + 7 * sum(depths) + 3 * heads + scale + 11 * split[1] + 1000 * expansion)
    c, hid, sd = embed_dim, int(expansion * embed_dim), {}
    half, pos_dim = hid // 2, (c // 2 // 4) // 4

    def lin(name, o, i, k=0, gain=1.0, bias=0.05, groups=1):    # k = 0: a Linear [o, i]; k = 1 | 3: a conv [o, i / groups, k, k]
        fan = (i // groups) * max(k, 1) ** 2
        sd[name + ".weight"] = torch.randn((o, i) if k == 0 else (o, i // groups, k, k), generator=g) * gain / math.sqrt(fan)
        sd[name + ".bias"] = torch.randn((o,), generator=g) * bias

    def norm(name, n=c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn((n,), generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn((n,), generator=g)

    def bn(name, n):
        norm(name, n)
        sd[name + ".running_mean"] = 0.1 * torch.randn((n,), generator=g)
        sd[name + ".running_var"] = 0.5 + torch.rand((n,), generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(1000)

    lin("conv_first", c, 3, 3, 4.0)
    norm("before_RG.1")
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.blocks.{j}."
            norm(b + "norm1")
            lin(b + "attn.qkv", 3 * c, c, gain=1.5)
            lin(b + "attn.proj", c, c, gain=0.7)
            lin(b + "attn.dwconv.0", c, c, 3, 1.5, groups=c)
            bn(b + "attn.dwconv.1", c)
            p = b + "attn.channel_interaction."
            lin(p + "1", c // 8, c, 1, 3.0)
            bn(p + "2", c // 8)
            lin(p + "4", c, c // 8, 1, 2.0)
            p = b + "attn.spatial_interaction."
            lin(p + "0", c // 16, c, 1, 1.5)
            bn(p + "1", c // 16)
            lin(p + "3", 1, c // 16, 1, 2.0)
            if j % 2 == 0:
                for k, (hs, ws) in enumerate((split, split[::-1])):
                    p = b + f"attn.attns.{k}.pos."
                    lin(p + "pos_proj", pos_dim, 2, gain=0.5)
                    for n, out in (("pos1", pos_dim), ("pos2", pos_dim), ("pos3", heads // 2)):
                        norm(p + n + ".0", pos_dim)
                        lin(p + n + ".2", out, pos_dim, gain=2.0, bias=0.3)
                    sd[b + f"attn.attns.{k}.rpe_biases"] = offsets(hs, ws)
                    sd[b + f"attn.attns.{k}.relative_position_index"] = relative_position_index(hs, ws)
                if is_shifted(i, j):
                    sd[b + "attn.attn_mask_0"] = shift_mask(64, 64, split[0], split[1])
                    sd[b + "attn.attn_mask_1"] = shift_mask(64, 64, split[1], split[0])
            else:
                sd[b + "attn.temperature"] = torch.exp(math.log(0.5) + (math.log(5.0) - math.log(0.5)) * torch.rand((heads, 1, 1), generator=g))
            norm(b + "norm2")
            lin(b + "ffn.fc1", hid, c, gain=1.4)
            norm(b + "ffn.sg.norm", half)
            lin(b + "ffn.sg.conv", half, half, 3, 1.5, groups=half)
            lin(b + "ffn.fc2", c, half, gain=0.7)
        lin(f"layers.{i}.conv", c, c, 3, 0.5)
    norm("norm")
    lin("conv_after_body", c, c, 3, 1.0)
    lin("conv_before_upsample.0", 64, c, 3, 1.0)
    f2 = 9 if scale == 3 else 4
    for k in ((0, 2) if scale == 4 else (0,)):
        lin(f"upsample.{k}", f2 * 64, 64, 3, 1.0)
    lin("conv_last", 3, 64, 3, 0.15, bias=0.02)
    return sd
