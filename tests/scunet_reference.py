"""Plain torch restatement of SCUNet (Zhang et al., "Practical Blind Denoising via Swin-Conv-UNet and Data Synthesis"; the official
network_scunet.py, which the webui's extensions-builtin/ScuNET loads) — the reference of the ScuNET tests (test infrastructure; fp32 on
the CPU).

    SCUNet(in_nc=3, config, dim=64), head_dim 32, window 8
    x  = ReplicationPad2d((0, padR, 0, padB))(x) to multiples of 64
    x1 = m_head(x); x2 = m_down1(x1); x3 = m_down2(x2); x4 = m_down3(x3); x = m_body(x4)
    x  = m_up3(x + x4); x = m_up2(x + x3); x = m_up1(x + x2); x = m_tail(x + x1), cropped
    m_downN = config[N-1] x CTB + Conv2d(2, 2, 0), m_upN = ConvTranspose2d(2, 2, 0) + config x CTB, no bias on any of the resampling /
    head / tail convs; block i of a stage is 'W' for even i, 'SW' for odd i
    CTB(c, t): conv_x, trans_x = split(conv1_1(x)); conv_x = conv_block(conv_x) + conv_x; trans_x = Block(trans_x);
               x = x + conv1_2(cat(conv_x, trans_x))
    Block: x = x + msa(ln1(x)); x = x + mlp(ln2(x));  msa = WMSA: roll by -4 ('SW'), 8 x 8 windows, embedding_layer, q k^T 32^-1/2 +
           relative_position_params[h][ya - yb + 7][xa - xb + 7], -inf on the masked pairs ('SW', last row / column of windows), softmax,
           @ v, heads merged as (h c), linear, roll back.

`forward(sd, x, q)` takes an optional rounding `q` applied wherever the engine stores fp16 or feeds an MFMA: the padded input, every
conv / linear output (with its residual sum, after its fused activation), the LayerNorm outputs, q / k / v, the softmax probabilities,
the attention output, the skip sums.  m_tail's output stays fp32.  q = identity is the fp32 reference; `fp16_twin` is q = fp16_emu.r16
with the conv / linear weights rounded to fp16.

Test weights (`make_state_dict`): seeded.  Linear / conv weights N(0, g^2 / fan_in) with gains that keep the stream O(1) through 14+
blocks (a ConvTransBlock's increment is linear in its input, so the stream grows by a factor per block: 0.7 on conv1_1 and 0.25 on
conv1_2 keep that at ~ 1.03; 0.7 on the two residual branches of a Block and on the second 3x3, 0.7 on the transposed convs, whose
input is a sum of two streams).  m_head and m_tail have no bias, so the output's level comes from the weights: every m_head filter carries an
offset that puts its feature at 1 on a mid-grey image, m_tail's centre taps an offset that maps that to 0.45; its random part spreads the
output by ~ 0.1: inside [0, 1]."""
import math

import torch
import torch.nn.functional as F

WS = 8
STAGES = ("m_down1", "m_down2", "m_down3", "m_body", "m_up3", "m_up2", "m_up1")


def ident(t):
    return t


def stage_dim(st):
    """conv_dim = trans_dim of stage st."""
    return 32 << (st if st < 4 else 6 - st)


def window_partition(x):
    """[B, H, W, C] -> [B, nWy, nWx, 64, C]."""
    b, h, w, c = x.shape
    return x.view(b, h // WS, WS, w // WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h // WS, w // WS, WS * WS, c)


def window_reverse(win, b, h, w):
    c = win.shape[-1]
    return win.view(b, h // WS, w // WS, WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def relative_bias(params):
    """relative_position_params [heads, 15, 15] -> [heads, 64, 64]: bias[h][a][b] = params[h][ya - yb + 7][xa - xb + 7]."""
    cord = torch.tensor([[i, j] for i in range(WS) for j in range(WS)])
    rel = cord[:, None, :] - cord[None, :, :] + WS - 1
    return params[:, rel[:, :, 0].long(), rel[:, :, 1].long()]


def wmsa_mask(nwy, nwx, shift=4):
    """[nwy, nwx, 64, 64] bool, True = forbidden, as WMSA.generate_mask builds it for an 'SW' block on nwy x nwx windows."""
    p, s = WS, WS - shift
    m = torch.zeros(nwy, nwx, p, p, p, p, dtype=torch.bool)
    m[-1, :, :s, :, s:, :] = True
    m[-1, :, s:, :, :s, :] = True
    m[:, -1, :, :s, :, s:] = True
    m[:, -1, :, s:, :, :s] = True
    return m.reshape(nwy, nwx, p * p, p * p)


def window_attention(qkv, params, mask=None, q=ident, use_bias=True):
    """qkv [B, nWy, nWx, 64, 3C] (already rounded by the caller), columns ordered (three heads, 32) -> [B, nWy, nWx, 64, C]."""
    b, ny, nx, t, c3 = qkv.shape
    heads = c3 // 96
    qq, kk, vv = qkv.view(b, ny, nx, t, 3, heads, 32).permute(4, 0, 1, 2, 5, 3, 6)       # each [B, nWy, nWx, heads, 64, 32]
    s = (qq @ kk.transpose(-2, -1)) * 32 ** -0.5
    if use_bias:
        s = s + relative_bias(params).to(s.dtype)
    if mask is not None:
        s = s.masked_fill(mask[None, :, :, None].to(s.device), float("-inf"))
    p = q(torch.softmax(s, dim=-1))
    return q((p @ vv).transpose(3, 4).reshape(b, ny, nx, t, heads * 32))


def block(sd, pre, x, shift, q=ident, mask=True, bias=True, mlp=True):
    """One transformer Block on [B, H, W, C]; pre = "m_down1.0.trans_block.".  mask / bias / mlp = False drop that term (the GPU tests
    show with them that each one is really applied)."""
    b, h, w, c = x.shape
    y = q(F.layer_norm(x, (c,), sd[pre + "ln1.weight"], sd[pre + "ln1.bias"], 1e-5))
    if shift:
        y = torch.roll(y, (-shift, -shift), (1, 2))
    qkv = q(F.linear(window_partition(y), sd[pre + "msa.embedding_layer.weight"], sd[pre + "msa.embedding_layer.bias"]))
    m = wmsa_mask(h // WS, w // WS, shift) if shift and mask else None
    a = window_reverse(window_attention(qkv, sd[pre + "msa.relative_position_params"], m, q, bias), b, h, w)
    if shift:
        a = torch.roll(a, (shift, shift), (1, 2))
    x = q(x + F.linear(a, sd[pre + "msa.linear.weight"], sd[pre + "msa.linear.bias"]))
    if not mlp:
        return x
    y = q(F.layer_norm(x, (c,), sd[pre + "ln2.weight"], sd[pre + "ln2.bias"], 1e-5))
    y = q(F.gelu(F.linear(y, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"])))
    return q(x + F.linear(y, sd[pre + "mlp.2.weight"], sd[pre + "mlp.2.bias"]))


def conv_trans_block(sd, pre, x, sw, q=ident):
    """One ConvTransBlock on NCHW; pre = "m_down1.0."."""
    c = x.shape[1] // 2
    y = q(F.conv2d(x, sd[pre + "conv1_1.weight"], sd[pre + "conv1_1.bias"]))
    conv_x, trans_x = y[:, :c], y[:, c:]
    t = q(F.relu(F.conv2d(conv_x, sd[pre + "conv_block.0.weight"], None, padding=1)))
    conv_x = q(F.conv2d(t, sd[pre + "conv_block.2.weight"], None, padding=1) + conv_x)
    trans_x = block(sd, pre + "trans_block.", trans_x.permute(0, 2, 3, 1), 4 if sw else 0, q).permute(0, 3, 1, 2)
    return q(x + F.conv2d(torch.cat((conv_x, trans_x), 1), sd[pre + "conv1_2.weight"], sd[pre + "conv1_2.bias"]))


def config_of(sd):
    depths = []
    for st, stem in enumerate(STAGES):
        first, n = (1 if st > 3 else 0), 0
        while f"{stem}.{first + n}.conv1_1.weight" in sd:
            n += 1
        depths.append(n)
    return dict(depths=tuple(depths), dim=int(sd["m_head.0.weight"].shape[0]), scale=1)


def forward(sd, x, q=ident):
    """x [B, 3, H, W] in [0, 1] -> [B, 3, H, W]."""
    depths = config_of(sd)["depths"]
    h0, w0 = x.shape[2:]
    x = q(F.pad(x, (0, -w0 % 64, 0, -h0 % 64), "replicate"))

    def blocks(st, y):
        first = 1 if st > 3 else 0
        for i in range(depths[st]):
            y = conv_trans_block(sd, f"{STAGES[st]}.{first + i}.", y, i % 2, q)
        return y
    skips = [q(F.conv2d(x, sd["m_head.0.weight"], None, padding=1))]
    for st in range(3):
        y = blocks(st, skips[-1])
        skips.append(q(F.conv2d(y, sd[f"{STAGES[st]}.{depths[st]}.weight"], None, stride=2)))
    y = blocks(3, skips[3])
    for st in (4, 5, 6):
        y = q(F.conv_transpose2d(q(y + skips[7 - st]), sd[f"{STAGES[st]}.0.weight"], None, stride=2))
        y = blocks(st, y)
    y = F.conv2d(q(y + skips[0]), sd["m_tail.0.weight"], None, padding=1)
    return y[:, :, :h0, :w0].contiguous()


def round_weights(sd):
    """The state dict with every conv / linear weight rounded to fp16 (biases, norms and relative_position_params stay fp32, as in the
    engine)."""
    from fp16_emu import r16
    return {k: (r16(v) if k.endswith(".weight") and v.dim() >= 2 else v) for k, v in sd.items()}


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward(round_weights(sd), x, r16)


def make_block(sd, pre, c, g):
    """The tensors of one transformer Block of width c under the prefix pre."""
    def lin(name, o, i, gain=1.0):
        sd[name + ".weight"] = torch.randn((o, i), generator=g) * gain / math.sqrt(i)
        sd[name + ".bias"] = torch.randn((o,), generator=g) * 0.05

    def norm(name):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn((c,), generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn((c,), generator=g)
    norm(pre + "ln1")
    sd[pre + "msa.relative_position_params"] = 0.5 * torch.randn((c // 32, 2 * WS - 1, 2 * WS - 1), generator=g)
    lin(pre + "msa.embedding_layer", 3 * c, c, 1.5)
    lin(pre + "msa.linear", c, c, 0.7)
    norm(pre + "ln2")
    lin(pre + "mlp.0", 4 * c, c)
    lin(pre + "mlp.2", c, 4 * c, 0.7)


def make_state_dict(depths=(2,) * 7, seed=0):
    g = torch.Generator().manual_seed(0x5C + 977 * seed + sum((i + 1) * d for i, d in enumerate(depths)))
    sd = {}

    def conv(name, o, i, k, gain=1.0, bias=False):
        sd[name + ".weight"] = torch.randn((o, i, k, k), generator=g) * gain / math.sqrt(i * k * k)
        if bias:
            sd[name + ".bias"] = torch.randn((o,), generator=g) * 0.05
    conv("m_head.0", 64, 3, 3, 2.0)
    sd["m_head.0.weight"] += 2.0 / 27
    for st, (stem, depth) in enumerate(zip(STAGES, depths)):
        c = stage_dim(st)
        d = 2 * c
        first = 1 if st > 3 else 0
        if st > 3:
            sd[f"{stem}.0.weight"] = torch.randn((2 * d, d, 2, 2), generator=g) * 0.7 / math.sqrt(2 * d)
        for i in range(first, first + depth):
            make_block(sd, f"{stem}.{i}.trans_block.", c, g)
            conv(f"{stem}.{i}.conv1_1", d, d, 1, 0.7, True)
            conv(f"{stem}.{i}.conv1_2", d, d, 1, 0.25, True)
            conv(f"{stem}.{i}.conv_block.0", c, c, 3, 1.4)
            conv(f"{stem}.{i}.conv_block.2", c, c, 3, 0.7)
        if st < 3:
            conv(f"{stem}.{depth}", 2 * d, d, 2, 1.0)
    conv("m_tail.0", 3, 64, 3, 0.05)
    sd["m_tail.0.weight"][:, :, 1, 1] += 0.45 / 64
    return sd


def image(b, h, w, seed):
    """[b, 3, h, w] fp32: U(0.35, 0.65) rounded to k / 255 (so the uint8 and the fp32 form of an input are the same image)."""
    g = torch.Generator().manual_seed(seed)
    return torch.round((torch.rand((b, 3, h, w), generator=g) * 0.3 + 0.35) * 255.0) / 255.0
