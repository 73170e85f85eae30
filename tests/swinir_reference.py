"""Plain torch restatement of SwinIR (Liang et al. 2021; the webui's extensions-builtin/SwinIR/swinir_model_arch.py) with the
`nearest+conv` upsampler — the reference of the SwinIR tests (test infrastructure; fp32 on the CPU).

    x    = reflect-pad right / bottom to multiples of 8;  x = x - mean
    f    = conv_first(x);  t = patch_embed.norm(tokens(f))
    t    = t + conv_i(blocks_i(t))            for every RSTB i (conv_i: `1conv` or `3conv`)
    f    = conv_after_body(norm(t)) + f
    y    = LeakyReLU(0.01)(conv_before_upsample.0(f))
    y    = lrelu(conv_up1(nearest x2(y)));  x4: y = lrelu(conv_up2(nearest x2(y)))
    y    = conv_last(lrelu(conv_hr(y))) + mean, cropped                    (lrelu = LeakyReLU(0.2))
    block j of an RSTB (shift 4 for odd j):  x = x + unshift(merge(attn(partition(shift(norm1(x))))));  x = x + fc2(gelu(fc1(norm2(x))))

Everything is read from the state dict (`config_of`).  The shift mask is built the way the original builds it (an id image cut by the
slices (0, -8), (-8, -4), (-4, None), window-partitioned, -100 where two ids differ) and is applied whenever shift > 0, for every input
size: the models are built with img_size 64, so the original never drops the shift for a small input.

`forward(sd, x, q)` takes an optional rounding `q` applied wherever the engine stores fp16 or feeds an MFMA: the mean-subtracted input,
every conv / linear output (with its residual sum, after its fused activation), a separate LeakyReLU pass's output, the LayerNorm outputs,
q / k / v, the softmax probabilities and the attention output.  conv_last's output stays fp32.  q = identity is the fp32 reference;
`fp16_twin` is q = fp16_emu.r16 with the conv / linear weights rounded to fp16.

Test weights (`make_state_dict`): seeded.  Linear / conv weights N(0, g^2 / fan_in) with gains that keep the token stream O(1) through
the depth (0.5 on the two residual branches of a block and on the conv that closes an RSTB), conv_first x 4 on its ~0.1-sized input,
the tail Kaiming for LeakyReLU(0.2), conv_last so that the output is 0.43 +- ~0.15: inside [0, 1].  Bias tables N(0, 0.5^2) (spread ~ 1
between entries), norm weights 1 + N(0, 0.1^2), biases N(0, 0.05^2)."""
import math

import torch
import torch.nn.functional as F

MEAN = (0.4488, 0.4371, 0.4040)
WS = 8


def ident(t):
    return t


def relative_position_index():
    """[64, 64]: index[a][b] = (ya - yb + 7) * 15 + (xa - xb + 7) for window-local tokens a, b (row-major in the 8 x 8 window)."""
    coords = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)      # [2, 64]
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (WS - 1)
    return rel[..., 0] * (2 * WS - 1) + rel[..., 1]


def window_partition(x):
    """[B, H, W, C] -> [B * nW, 64, C], windows row-major."""
    b, h, w, c = x.shape
    return x.view(b, h // WS, WS, w // WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, WS * WS, c)


def window_reverse(win, b, h, w):
    c = win.shape[-1]
    return win.view(b, h // WS, w // WS, WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def region_ids(h, w, shift=4):
    """[h, w] id image of the SHIFTED grid: 3 * r(y) + r(x) with the slices (0, -8), (-8, -shift), (-shift, None)."""
    img = torch.zeros((h, w))
    cnt = 0
    for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
        for ws_ in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            img[hs, ws_] = cnt
            cnt += 1
    return img


def shift_mask(h, w, shift=4):
    """[nW, 64, 64]: -100.0 where the region ids of two tokens of a window differ, else 0."""
    ids = window_partition(region_ids(h, w, shift)[None, :, :, None]).squeeze(-1)
    diff = ids[:, None, :] - ids[:, :, None]
    return torch.where(diff != 0, torch.tensor(-100.0), torch.tensor(0.0))


_MASKS = {}


def _cached_mask(h, w, shift, device, dtype):
    """shift_mask on the device of the run, built once per size (the original keeps it as a buffer)."""
    key = (h, w, shift, str(device), dtype)
    if key not in _MASKS:
        _MASKS[key] = shift_mask(h, w, shift).to(device, dtype)
    return _MASKS[key]


def window_attention(qkv, table, heads, mask=None, q=ident, use_bias=True):
    """qkv [nWB, 64, 3C] (already rounded by the caller) -> [nWB, 64, C]: softmax(q k^T d^-1/2 + bias + mask) v, the probabilities and the
    result through q."""
    n, t, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    qq, kk, vv = qkv.view(n, t, 3, heads, d).permute(2, 0, 3, 1, 4)
    s = (qq @ kk.transpose(-2, -1)) * d ** -0.5
    if use_bias:
        s = s + table[relative_position_index().view(-1).to(table.device)].view(t, t, heads).permute(2, 0, 1)[None]
    if mask is not None:
        nw = mask.shape[0]
        s = (s.view(n // nw, nw, heads, t, t) + mask[None, :, None]).view(n, heads, t, t)
    p = q(torch.softmax(s, dim=-1))
    return q((p @ vv).transpose(1, 2).reshape(n, t, c))


def block(sd, pre, x, heads, shift, q=ident):
    """One SwinTransformerBlock on [B, H, W, C]; pre = "layers.i.residual_group.blocks.j."."""
    b, h, w, c = x.shape
    y = q(F.layer_norm(x, (c,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    if shift:
        y = torch.roll(y, (-shift, -shift), (1, 2))
    qkv = q(F.linear(window_partition(y), sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]))
    mask = _cached_mask(h, w, shift, x.device, x.dtype) if shift else None
    a = window_attention(qkv, sd[pre + "attn.relative_position_bias_table"], heads, mask, q)
    a = window_reverse(a, b, h, w)
    if shift:
        a = torch.roll(a, (shift, shift), (1, 2))
    x = q(x + F.linear(a, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"]))
    y = q(F.layer_norm(x, (c,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-5))
    y = q(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])))
    return q(x + F.linear(y, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"]))


def config_of(sd):
    c = sd["conv_first.weight"].shape[0]
    depths = []
    while f"layers.{len(depths)}.residual_group.blocks.0.norm1.weight" in sd:
        i, j = len(depths), 0
        while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    heads = sd["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"].shape[1]
    return dict(embed_dim=c, depths=tuple(depths), num_heads=heads, mlp_hidden=sd["layers.0.residual_group.blocks.0.mlp.fc1.weight"].shape[0],
                resi_3conv=int("layers.0.conv.0.weight" in sd), scale=4 if "conv_up2.weight" in sd else 2)


def _conv(sd, name, x, pad=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)


def _resi(sd, stem, x, resid, q):
    """conv(x) + resid with the conv that closes an RSTB / the trunk; x, resid NCHW."""
    if stem + ".weight" in sd:
        return q(_conv(sd, stem, x) + resid)
    y = q(F.leaky_relu(q(_conv(sd, stem + ".0", x)), 0.2))
    y = q(F.leaky_relu(q(_conv(sd, stem + ".2", y, 0)), 0.2))
    return q(_conv(sd, stem + ".4", y) + resid)


def forward(sd, x, q=ident):
    """x [B, 3, H, W] in [0, 1], H, W >= 8 -> [B, 3, H s, W s], on the device and in the dtype of x and the state dict (fp32 on the CPU
    for the tests)."""
    cfg = config_of(sd)
    heads, s = cfg["num_heads"], cfg["scale"]
    b, _, h0, w0 = x.shape
    x = F.pad(x, (0, -w0 % WS, 0, -h0 % WS), "reflect")
    mean = torch.tensor(MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    f = q(_conv(sd, "conv_first", q(x - mean)))
    c = f.shape[1]
    t = f.permute(0, 2, 3, 1)                                                   # [B, H, W, C]: tokens
    t = q(F.layer_norm(t, (c,), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], 1e-5))
    for i, depth in enumerate(cfg["depths"]):
        y = t
        for j in range(depth):
            y = block(sd, f"layers.{i}.residual_group.blocks.{j}.", y, heads, 4 if j % 2 else 0, q)
        t = _resi(sd, f"layers.{i}.conv", y.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), q).permute(0, 2, 3, 1)
    t = q(F.layer_norm(t, (c,), sd["norm.weight"], sd["norm.bias"], 1e-5))
    f = _resi(sd, "conv_after_body", t.permute(0, 3, 1, 2), f, q)
    y = q(F.leaky_relu(q(_conv(sd, "conv_before_upsample.0", f)), 0.01))
    y = q(F.leaky_relu(_conv(sd, "conv_up1", F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
    if s == 4:
        y = q(F.leaky_relu(_conv(sd, "conv_up2", F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
    y = _conv(sd, "conv_last", q(F.leaky_relu(_conv(sd, "conv_hr", y), 0.2))) + mean
    return y[:, :, :h0 * s, :w0 * s].contiguous()


def round_weights(sd):
    """The state dict with every conv / linear weight rounded to fp16 (biases, norms and bias tables stay fp32, as in the engine)."""
    from fp16_emu import r16
    return {k: (r16(v) if k.endswith(".weight") and v.dim() >= 2 else v) for k, v in sd.items()}


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward(round_weights(sd), x, r16)


def make_state_dict(embed_dim=60, depths=(2, 2), heads=2, resi="1conv", scale=4, seed=0, mlp_ratio=2):
    g = torch.Generator().manual_seed(0x51 + 977 * seed + 31 * embed_dim + 7 * sum(depths) + 3 * heads + scale + (100 if resi == "3conv" else 0))
    c, hid, sd = embed_dim, int(mlp_ratio * embed_dim), {}

    def lin(name, o, i, k=0, gain=1.0, bias=0.05):              # k = 0: a Linear [o, i]; k = 1 | 3: a conv [o, i, k, k]
        fan = i * max(k, 1) ** 2
        sd[name + ".weight"] = torch.randn((o, i) if k == 0 else (o, i, k, k), generator=g) * gain / math.sqrt(fan)
        sd[name + ".bias"] = torch.randn((o,), generator=g) * bias

    def norm(name):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn((c,), generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn((c,), generator=g)

    def resi_conv(stem, gain):
        if resi == "1conv":
            lin(stem, c, c, 3, gain)
        else:
            lin(stem + ".0", c // 4, c, 3, 1.4)
            lin(stem + ".2", c // 4, c // 4, 1, 1.4)
            lin(stem + ".4", c, c // 4, 3, gain * 1.4)

    lin("conv_first", c, 3, 3, 4.0)
    norm("patch_embed.norm")
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            norm(b + "norm1")
            sd[b + "attn.relative_position_bias_table"] = 0.5 * torch.randn(((2 * WS - 1) ** 2, heads), generator=g)
            sd[b + "attn.relative_position_index"] = relative_position_index()
            lin(b + "attn.qkv", 3 * c, c, gain=1.5)
            lin(b + "attn.proj", c, c, gain=0.7)
            if j % 2:
                sd[b + "attn_mask"] = shift_mask(64, 64)
            norm(b + "norm2")
            lin(b + "mlp.fc1", hid, c)
            lin(b + "mlp.fc2", c, hid, gain=0.7)
        resi_conv(f"layers.{i}.conv", 0.5)
    norm("norm")
    resi_conv("conv_after_body", 1.0)
    lin("conv_before_upsample.0", 64, c, 3, 1.0)
    lin("conv_up1", 64, 64, 3, 1.4)
    if scale == 4:
        lin("conv_up2", 64, 64, 3, 1.4)
    lin("conv_hr", 64, 64, 3, 1.4)
    lin("conv_last", 3, 64, 3, 0.15, bias=0.02)
    return sd


def image(b, h, w, seed):
    """[b, 3, h, w] fp32: U(0.35, 0.65) rounded to n / 255 (so the uint8 and the fp32 form of an input are the same image)."""
    g = torch.Generator().manual_seed(seed)
    return torch.round((torch.rand((b, 3, h, w), generator=g) * 0.3 + 0.35) * 255.0) / 255.0


class SwinIRModule(torch.nn.Module):
    """The reference as a module with real parameters (what a webui scaler holds): .half() / .to(device) work, for the job-level
    comparison and the timing yardstick (tools/gpu/swinir_time.py).  The tensors are buffers, so the state dict moves with the module."""

    def __init__(self, sd):
        super().__init__()
        self.names = list(sd)
        for i, k in enumerate(self.names):
            self.register_buffer(f"t{i}", sd[k].clone())

    def forward(self, x):
        sd = {k: getattr(self, f"t{i}") for i, k in enumerate(self.names)}
        return forward(sd, x)
