"""Plain torch restatement of BasicSR's RRDBNet (basicsr/archs/rrdbnet_arch.py: ResidualDenseBlock, RRDB, RRDBNet.forward) — the
reference of the ESRGAN / Real-ESRGAN tests (test infrastructure; fp32 on the CPU).

    rdb(x)   x1 = lrelu(conv1(x)); x2 = lrelu(conv2(cat(x, x1))); ... x5 = conv5(cat(x, x1, x2, x3, x4)); return x5 * 0.2 + x
    rrdb(x)  rdb3(rdb2(rdb1(x))) * 0.2 + x
    net(x)   feat = conv_first(pixel_unshuffle(x, 4 / scale));  feat = feat + conv_body(body(feat))
             feat = lrelu(conv_up1(nearest_x2(feat)));  feat = lrelu(conv_up2(nearest_x2(feat)));  conv_last(lrelu(conv_hr(feat)))

`forward(sd, x, q)` takes the checkpoint's state dict (new-arch keys) and an optional rounding `q` applied to every tensor a module
writes: q = identity is the fp32 reference, q = fp16_emu.r16 with r16 weights (`fp16_twin`) is the fp16-storage twin — what the same
network computes as `model.half()` (fp32 accumulation, every output stored as binary16).

Test weights (`make_state_dict`): seeded normals.  The dense-block convs get 0.1 x Kaiming (std = 0.1 sqrt(2 / fan_in), BasicSR's
default_init_weights(..., 0.1) — the only convs RRDBNet initialises that way); the convs outside the blocks get plain Kaiming, as the
0.1 scale on ALL thirteen layers of the trunk would shrink the output to ~1e-5 (every byte 0: a saturated image compares nothing).
conv_last is scaled so that the output has a spread of a few tenths and its bias is 0.5, which centres the image in [0, 1]; the other
biases are small seeded normals so that the bias path is exercised.  tests/test_cpu_esrgan.py checks that fewer than 5 % of the
reference's output bytes are 0 or 255.
"""
import torch
import torch.nn.functional as F


def conv_names(num_block):
    names = ["conv_first"] + [f"body.{i}.rdb{j}.conv{k}" for i in range(num_block) for j in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
    return names + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"]


def conv_shape(name, in_ch=3):
    if name == "conv_first":
        return 64, in_ch
    if name == "conv_last":
        return 3, 64
    if ".conv" in name:
        k = int(name[-1])
        return (32 if k < 5 else 64), 64 + 32 * (k - 1)
    return 64, 64


def make_state_dict(num_block=2, scale=4, seed=0):
    g = torch.Generator().manual_seed(0xE5 + seed)
    in_ch = {4: 3, 2: 12, 1: 48}[scale]
    sd = {}
    for n in conv_names(num_block):
        o, i = conv_shape(n, in_ch)
        std = (2.0 / (i * 9)) ** 0.5 * (0.1 if ".rdb" in n else 1.0)
        if n == "conv_last":
            std *= 0.08
        sd[n + ".weight"] = torch.randn((o, i, 3, 3), generator=g) * std
        sd[n + ".bias"] = torch.randn((o,), generator=g) * 0.02 + (0.5 if n == "conv_last" else 0.0)
    return sd


def to_old_arch(sd, num_block):
    """The same weights under the original ESRGAN x4 key layout."""
    top = {"conv_first": "model.0", "conv_body": f"model.1.sub.{num_block}", "conv_up1": "model.3", "conv_up2": "model.6",
           "conv_hr": "model.8", "conv_last": "model.10"}
    out = {}
    for k, v in sd.items():
        stem, leaf = k.rsplit(".", 1)
        if stem in top:
            out[f"{top[stem]}.{leaf}"] = v
        else:
            _, i, rdb, conv = stem.split(".")
            out[f"model.1.sub.{i}.RDB{rdb[3:]}.{conv}.0.{leaf}"] = v
    return out


def rdb(sd, prefix, x, q):
    feats = [x]
    for k in (1, 2, 3, 4, 5):
        y = q(F.conv2d(torch.cat(feats, 1), sd[f"{prefix}.conv{k}.weight"], sd[f"{prefix}.conv{k}.bias"], padding=1))
        if k < 5:
            feats.append(q(F.leaky_relu(y, 0.2)))
    return q(y * 0.2 + x)


def forward(sd, x, q=lambda t: t):
    """x [B, 3, H, W] fp32 in [0, 1] -> [B, 3, H s, W s] fp32 (s from conv_first's input channels)."""
    num_block = len({k.split(".")[1] for k in sd if k.startswith("body.")})
    unshuffle = {3: 1, 12: 2, 48: 4}[sd["conv_first.weight"].shape[1]]
    conv = lambda n, t: q(F.conv2d(t, sd[n + ".weight"], sd[n + ".bias"], padding=1))
    lrelu = lambda t: q(F.leaky_relu(t, 0.2))
    feat = q(F.pixel_unshuffle(x, unshuffle) if unshuffle > 1 else x)
    feat = conv("conv_first", feat)
    body = feat
    for i in range(num_block):
        y = body
        for j in (1, 2, 3):
            y = rdb(sd, f"body.{i}.rdb{j}", y, q)
        body = q(y * 0.2 + body)
    feat = q(feat + conv("conv_body", body))
    feat = lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    feat = lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    return conv("conv_last", lrelu(conv("conv_hr", feat)))


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward({k: (r16(v) if k.endswith(".weight") else v) for k, v in sd.items()}, x, r16)


class RRDBNetModule(torch.nn.Module):
    """The reference as a module (what a webui scaler holds), for the job-level comparison."""

    def __init__(self, sd):
        super().__init__()
        self.sd = {k: v.clone() for k, v in sd.items()}

    def forward(self, x):
        return forward(self.sd, x)
