"""Plain torch restatement of Swin2SR (Conde et al. 2022, network_swin2sr.py; the webui's extensions-builtin/SwinIR/swinir_model_arch_v2.py)
— the reference of the Swin2SR tests (test infrastructure; fp32 on the CPU).  SwinIR's skeleton (tests/swinir_reference.py, whose window
helpers are used here) with Swin-V2 blocks:

    x    = reflect-pad right / bottom to multiples of 8;  x = x - mean
    f    = conv_first(x);  t = patch_embed.norm(patch_embed.proj(tokens(f)))       (proj: a 1x1 conv; absent = identity)
    t    = t + layers.i.patch_embed.proj(conv_i(blocks_i(t)))                      for every RSTB i
    f    = conv_after_body(norm(t)) + f
    block j (shift 4 for odd j):  x = x + norm1(unshift(merge(attn(partition(shift(x))))));  x = x + norm2(fc2(gelu(fc1(x))))
    attn: softmax(normalize(q) normalize(k)^T * exp(min(logit_scale, ln 100)) + 16 sigmoid(cpb_mlp(coords))[index] + mask) v,
          qkv = Linear(x; qkv.weight, (q_bias | 0 | v_bias))
    tails: nearest+conv (x4) as SwinIR's;
           pixelshuffle: y = LeakyReLU(0.01)(conv_before_upsample.0(f)); per step y = PixelShuffle(upsample.{0,2}(y)); conv_last(y) + mean
           pixelshuffledirect: PixelShuffle(upsample.0(f)) + mean

The shift mask is -100 where the region ids differ and is applied ONCE (the `transformers` port adds it twice; see
tests/test_cpu_swin2sr.py).

`forward(sd, x, q)` takes the rounding hook of swinir_reference: q is applied wherever the engine stores fp16 or feeds an MFMA — the
mean-subtracted input, every conv / linear output (after its fused activation), a separate LeakyReLU pass's output, the LayerNorm
outputs of the trunk, each `x + norm(branch)` sum (one rounding of the sum: swin2_layernorm_add), q / k / v, the softmax probabilities,
the attention output, the pixelshuffledirect conv's output.  q and k are NOT rounded again after normalisation; norms, logits and softmax
stay in the working precision.  conv_last's output stays fp32.  `fp16_twin` is q = fp16_emu.r16 with the conv / linear weights rounded to
fp16 — the layer-closing conv and its patch_embed.proj as the ONE conv the loader makes of them (P W, rounded once).

Test weights (`make_state_dict`): swinir_reference.make_state_dict's gains; the two norms of a block get gamma 0.5 (1 + N(0, 0.1^2)) (the
residual branches of a res-post-norm block have the size of their norm's gamma); logit_scale uniform over ln 3 .. ln 250 (some heads
above the clamp ln 100); cpb_mlp (hidden 512, as the architecture fixes it) with a spread that puts 16 sigmoid(.) across (0, 16); q_bias / v_bias N(0, 0.05^2);
patch_embed.proj near the identity."""
import math

import torch
import torch.nn.functional as F

import swinir_reference as S
from swinir_reference import MEAN, WS, ident, image, region_ids, relative_position_index, shift_mask, window_partition, window_reverse  # noqa: F401

UPSAMPLERS = ("nearest+conv", "pixelshuffle", "pixelshuffledirect")
LOGIT_MAX = math.log(100.0)


def coords_table(dtype=torch.float32):
    """[225, 2]: row (dy + 7) * 15 + (dx + 7) = (y, x) of the log-spaced relative coordinates."""
    d = torch.arange(-(WS - 1), WS, dtype=torch.float32) / (WS - 1) * 8
    t = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).reshape(-1, 2)
    return (torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)).to(dtype)


def bias_table(sd, pre):
    """16 sigmoid(cpb_mlp(coords)) -> [225, heads], in the dtype of the weights."""
    w0, b0, w2 = sd[pre + "attn.cpb_mlp.0.weight"], sd[pre + "attn.cpb_mlp.0.bias"], sd[pre + "attn.cpb_mlp.2.weight"]
    return 16 * torch.sigmoid(F.linear(F.relu(F.linear(coords_table(w0.dtype), w0, b0)), w2))


def head_scale(sd, pre):
    return torch.clamp(sd[pre + "attn.logit_scale"].reshape(-1), max=LOGIT_MAX).exp()


def cosine_window_attention(qkv, table, scale, heads, mask=None, q=ident, use_bias=True, use_scale=True):
    """qkv [nWB, 64, 3C] (already rounded by the caller) -> [nWB, 64, C]; table [225, heads] = 16 sigmoid(.), scale [heads]; the
    probabilities and the result through q."""
    n, t, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    qq, kk, vv = qkv.view(n, t, 3, heads, d).permute(2, 0, 3, 1, 4)
    s = F.normalize(qq, dim=-1) @ F.normalize(kk, dim=-1).transpose(-2, -1)
    if use_scale:
        s = s * scale.to(s.dtype).view(1, heads, 1, 1)
    if use_bias:
        s = s + table.to(s.dtype)[relative_position_index().view(-1).to(table.device)].view(t, t, heads).permute(2, 0, 1)[None]
    if mask is not None:
        nw = mask.shape[0]
        s = (s.view(n // nw, nw, heads, t, t) + mask[None, :, None]).view(n, heads, t, t)
    p = q(torch.softmax(s, dim=-1))
    return q((p @ vv).transpose(1, 2).reshape(n, t, c))


def qkv_bias(sd, pre, c):
    z = torch.zeros(c, dtype=sd[pre + "attn.qkv.weight"].dtype)
    return torch.cat([sd.get(pre + "attn.q_bias", z), z, sd.get(pre + "attn.v_bias", z)])


def block(sd, pre, x, heads, shift, q=ident):
    """One Swin-V2 block on [B, H, W, C]; pre = "layers.i.residual_group.blocks.j."."""
    b, h, w, c = x.shape
    y = torch.roll(x, (-shift, -shift), (1, 2)) if shift else x
    qkv = q(F.linear(window_partition(y), sd[pre + "attn.qkv.weight"], qkv_bias(sd, pre, c)))
    mask = S._cached_mask(h, w, shift, x.device, x.dtype) if shift else None
    a = cosine_window_attention(qkv, bias_table(sd, pre), head_scale(sd, pre), heads, mask, q)
    a = window_reverse(a, b, h, w)
    if shift:
        a = torch.roll(a, (shift, shift), (1, 2))
    t = q(F.linear(a, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"]))
    x = q(x + F.layer_norm(t, (c,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    y = q(F.gelu(F.linear(x, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])))
    t = q(F.linear(y, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"]))
    return q(x + F.layer_norm(t, (c,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-5))


def config_of(sd):
    c = sd["conv_first.weight"].shape[0]
    depths = []
    while f"layers.{len(depths)}.residual_group.blocks.0.norm1.weight" in sd:
        i, j = len(depths), 0
        while f"layers.{i}.residual_group.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    if "conv_up1.weight" in sd:
        upsampler, scale = "nearest+conv", 4
    elif "conv_before_upsample.0.weight" in sd:
        upsampler = "pixelshuffle"
        scale = 4 if "upsample.2.weight" in sd else (3 if sd["upsample.0.weight"].shape[0] == 576 else 2)
    else:
        upsampler, scale = "pixelshuffledirect", int(round(math.sqrt(sd["upsample.0.weight"].shape[0] / 3)))
    return dict(embed_dim=c, depths=tuple(depths), num_heads=sd["layers.0.residual_group.blocks.0.attn.logit_scale"].shape[0],
                mlp_hidden=sd["layers.0.residual_group.blocks.0.mlp.fc1.weight"].shape[0], resi_3conv=int("layers.0.conv.0.weight" in sd),
                upsampler=upsampler, scale=scale)


def _conv(sd, name, x, pad=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)


def _proj(sd, stem, x):
    """PatchEmbed.proj (1x1) on NCHW; the identity where the state dict has none."""
    return _conv(sd, stem, x, 0) if stem + ".weight" in sd else x


def _resi(sd, stem, proj, x, resid, q):
    """proj(conv(x)) + resid with the conv that closes an RSTB / the trunk (proj: the RSTB's patch_embed.proj, None for the trunk); x,
    resid NCHW.  The closing conv and proj are stored as one conv: one rounding."""
    def last(name, y):
        y = _conv(sd, name, y)
        return _proj(sd, proj, y) if proj else y
    if stem + ".weight" in sd:
        return q(last(stem, x) + resid)
    y = q(F.leaky_relu(q(_conv(sd, stem + ".0", x)), 0.2))
    y = q(F.leaky_relu(q(_conv(sd, stem + ".2", y, 0)), 0.2))
    return q(last(stem + ".4", y) + resid)


def forward(sd, x, q=ident):
    """x [B, 3, H, W] in [0, 1], H, W >= 8 -> [B, 3, H s, W s], on the device and in the dtype of x and the state dict."""
    cfg = config_of(sd)
    heads, s = cfg["num_heads"], cfg["scale"]
    b, _, h0, w0 = x.shape
    x = F.pad(x, (0, -w0 % WS, 0, -h0 % WS), "reflect")
    mean = torch.tensor(MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    f = q(_conv(sd, "conv_first", q(x - mean)))
    c = f.shape[1]
    t = q(_proj(sd, "patch_embed.proj", f)).permute(0, 2, 3, 1)                  # [B, H, W, C]: tokens
    t = q(F.layer_norm(t, (c,), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], 1e-5))
    for i, depth in enumerate(cfg["depths"]):
        y = t
        for j in range(depth):
            y = block(sd, f"layers.{i}.residual_group.blocks.{j}.", y, heads, 4 if j % 2 else 0, q)
        t = _resi(sd, f"layers.{i}.conv", f"layers.{i}.patch_embed.proj", y.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), q).permute(0, 2, 3, 1)
    t = q(F.layer_norm(t, (c,), sd["norm.weight"], sd["norm.bias"], 1e-5))
    f = _resi(sd, "conv_after_body", None, t.permute(0, 3, 1, 2), f, q)
    if cfg["upsampler"] == "pixelshuffledirect":
        y = F.pixel_shuffle(q(_conv(sd, "upsample.0", f)), s) + mean
        return y[:, :, :h0 * s, :w0 * s].contiguous()
    y = q(F.leaky_relu(q(_conv(sd, "conv_before_upsample.0", f)), 0.01))
    if cfg["upsampler"] == "nearest+conv":
        y = q(F.leaky_relu(_conv(sd, "conv_up1", F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
        y = q(F.leaky_relu(_conv(sd, "conv_up2", F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
        y = q(F.leaky_relu(_conv(sd, "conv_hr", y), 0.2))
    else:
        for k in ((0, 2) if s == 4 else (0,)):
            y = F.pixel_shuffle(q(_conv(sd, f"upsample.{k}", y)), 3 if s == 3 else 2)
    y = _conv(sd, "conv_last", y) + mean
    return y[:, :, :h0 * s, :w0 * s].contiguous()


def fold_projections(sd):
    """The state dict with every layers.i.patch_embed.proj multiplied into the conv in front of it (float64), as the loader stores them:
    the same function, the proj keys gone."""
    out = dict(sd)
    i = 0
    while f"layers.{i}.residual_group.blocks.0.norm1.weight" in sd:
        stem = f"layers.{i}.patch_embed.proj"
        if stem + ".weight" in sd:
            name = f"layers.{i}.conv" if f"layers.{i}.conv.weight" in sd else f"layers.{i}.conv.4"
            w, bias = sd[name + ".weight"].double(), sd[name + ".bias"].double()
            pw, pb = sd[stem + ".weight"].double().flatten(1), sd[stem + ".bias"].double()
            out[name + ".weight"] = (pw @ w.flatten(1)).view_as(w).to(sd[name + ".weight"].dtype)
            out[name + ".bias"] = (pw @ bias + pb).to(sd[name + ".bias"].dtype)
            del out[stem + ".weight"], out[stem + ".bias"]
        i += 1
    return out


def round_weights(sd):
    """Every conv / linear weight rounded to fp16, the closing convs with their projection folded in first (biases, norms, the cpb MLP
    and logit_scale stay fp32: the engine gets the bias table and head_scale ready-made in fp32)."""
    from fp16_emu import r16
    keep = ("cpb_mlp", "logit_scale")
    return {k: (r16(v) if k.endswith(".weight") and v.dim() >= 2 and not any(n in k for n in keep) else v) for k, v in fold_projections(sd).items()}


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward(round_weights(sd), x, r16)


def make_state_dict(embed_dim=60, depths=(2, 2), heads=6, resi="1conv", scale=4, upsampler="nearest+conv", seed=0, mlp_ratio=2, proj=True):
    g = torch.Generator().manual_seed(0x52 + 977 * seed + 31 * embed_dim + 7 * sum(depths) + 3 * heads + scale + (100 if resi == "3conv" else 0) +
                                      1000 * UPSAMPLERS.index(upsampler))
    c, hid, sd = embed_dim, int(mlp_ratio * embed_dim), {}

    def lin(name, o, i, k=0, gain=1.0, bias=0.05):              # k = 0: a Linear [o, i]; k = 1 | 3: a conv [o, i, k, k]
        fan = i * max(k, 1) ** 2
        sd[name + ".weight"] = torch.randn((o, i) if k == 0 else (o, i, k, k), generator=g) * gain / math.sqrt(fan)
        sd[name + ".bias"] = torch.randn((o,), generator=g) * bias

    def norm(name, gamma=1.0):
        sd[name + ".weight"] = gamma * (1.0 + 0.1 * torch.randn((c,), generator=g))
        sd[name + ".bias"] = 0.1 * gamma * torch.randn((c,), generator=g)

    def near_identity(name):
        sd[name + ".weight"] = (torch.eye(c) + 0.3 * torch.randn((c, c), generator=g) / math.sqrt(c)).view(c, c, 1, 1)
        sd[name + ".bias"] = torch.randn((c,), generator=g) * 0.05

    def resi_conv(stem, gain):
        if resi == "1conv":
            lin(stem, c, c, 3, gain)
        else:
            lin(stem + ".0", c // 4, c, 3, 1.4)
            lin(stem + ".2", c // 4, c // 4, 1, 1.4)
            lin(stem + ".4", c, c // 4, 3, gain * 1.4)

    lin("conv_first", c, 3, 3, 4.0)
    if proj:
        near_identity("patch_embed.proj")
    norm("patch_embed.norm")
    lo, hi = math.log(3.0), math.log(250.0)
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            sd[b + "attn.logit_scale"] = (lo + (hi - lo) * torch.rand((heads, 1, 1), generator=g))
            sd[b + "attn.cpb_mlp.0.weight"] = torch.randn((512, 2), generator=g)
            sd[b + "attn.cpb_mlp.0.bias"] = 0.5 * torch.randn((512,), generator=g)
            sd[b + "attn.cpb_mlp.2.weight"] = 0.14 * torch.randn((heads, 512), generator=g)
            sd[b + "attn.relative_coords_table"] = coords_table().view(1, 15, 15, 2)
            sd[b + "attn.relative_position_index"] = relative_position_index()
            lin(b + "attn.qkv", 3 * c, c, gain=1.5)
            del sd[b + "attn.qkv.bias"]
            sd[b + "attn.q_bias"] = 0.05 * torch.randn((c,), generator=g)
            sd[b + "attn.v_bias"] = 0.05 * torch.randn((c,), generator=g)
            lin(b + "attn.proj", c, c, gain=0.7)
            if j % 2:
                sd[b + "attn_mask"] = shift_mask(64, 64)
            norm(b + "norm1", 0.5)
            lin(b + "mlp.fc1", hid, c)
            lin(b + "mlp.fc2", c, hid, gain=0.7)
            norm(b + "norm2", 0.5)
        resi_conv(f"layers.{i}.conv", 0.5)
        if proj:
            near_identity(f"layers.{i}.patch_embed.proj")
    norm("norm")
    resi_conv("conv_after_body", 1.0)
    if upsampler == "pixelshuffledirect":
        lin("upsample.0", 3 * scale * scale, c, 3, 0.1, bias=0.02)
        return sd
    lin("conv_before_upsample.0", 64, c, 3, 1.0)
    if upsampler == "nearest+conv":
        assert scale == 4
        for n in ("conv_up1", "conv_up2", "conv_hr"):
            lin(n, 64, 64, 3, 1.4)
    else:
        f2 = 9 if scale == 3 else 4
        for k in ((0, 2) if scale == 4 else (0,)):
            lin(f"upsample.{k}", f2 * 64, 64, 3, 1.0)                   # no activation follows: gain 1
    lin("conv_last", 3, 64, 3, 0.15, bias=0.02)
    return sd
