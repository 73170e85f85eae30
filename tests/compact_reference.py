"""Plain torch restatement of Real-ESRGAN's SRVGGNetCompact (realesrgan/archs/srvgg_arch.py) — the reference of the compact-upscaler
tests (test infrastructure; fp32 on the CPU).

    body = [conv3x3(3 -> F), PReLU(F)] + num_conv x [conv3x3(F -> F), PReLU(F)] + [conv3x3(F -> 3 r^2)]
    out  = pixel_shuffle(body(x), r) + nearest_upsample(x, r)

State-dict keys: body.{2i}.weight / .bias for conv i (i = 0 .. num_conv + 1), body.{2i+1}.weight ([F], one slope per channel) for the
PReLU after it; none after the last conv.

`forward(sd, x, q)` takes the state dict and an optional rounding `q` applied to every tensor a module writes (each conv's output, each
PReLU's output, the pixel-shuffled tensor's sum with the base): q = identity is the fp32 reference, q = fp16_emu.r16 with r16 conv
weights (`fp16_twin`) is the fp16-storage twin — what the network computes as `model.half()`.  `residual(sd, x, q)` is the same without
the base: out - nearest_upsample(x, r) of the fp32 reference, the quantity the parity tests compare (the output itself is the input
image plus a small correction, so an error of the body barely shows in it).

Test weights (`make_state_dict`): seeded.  Conv weights N(0, 2 / ((1 + 0.25^2) fan_in)) — Kaiming for a PReLU of slope 0.25 — the
last conv's std x 0.3; biases N(0, 0.02^2); slopes U(0.05, 0.45).  With inputs U(0.35, 0.65) rounded to n / 255 (`image`) the residual
of the nets the GPU tests use (seed 0) has a spread of 0.11 - 0.19 and at most 2.9 % of the reference's output bytes are 0 or 255
(tests/test_cpu_compact.py asserts >= 0.1 and < 5 %).  The spread moves a lot with the draw: with the last conv at x 0.25 two of these
nets came out at 0.09, with x 0.35 one passed 5 % saturated bytes.
"""
import torch
import torch.nn.functional as F


def make_state_dict(num_conv=4, scale=4, seed=0, num_feat=64):
    g = torch.Generator().manual_seed(0xC0 + 131 * seed + 7 * num_conv + scale)
    sd = {}
    for i in range(num_conv + 2):
        o = 3 * scale * scale if i == num_conv + 1 else num_feat
        c = 3 if i == 0 else num_feat
        std = (2.0 / ((1 + 0.25 ** 2) * c * 9)) ** 0.5 * (0.3 if i == num_conv + 1 else 1.0)
        sd[f"body.{2 * i}.weight"] = torch.randn((o, c, 3, 3), generator=g) * std
        sd[f"body.{2 * i}.bias"] = torch.randn((o,), generator=g) * 0.02
        if i <= num_conv:
            sd[f"body.{2 * i + 1}.weight"] = torch.rand((num_feat,), generator=g) * 0.4 + 0.05
    return sd


def image(b, h, w, seed):
    """[b, 3, h, w] fp32: U(0.35, 0.65) rounded to n / 255 (so the uint8 and the fp32 form of an input are the same image)."""
    g = torch.Generator().manual_seed(seed)
    return torch.round((torch.rand((b, 3, h, w), generator=g) * 0.3 + 0.35) * 255.0) / 255.0


def num_conv_of(sd):
    return len([k for k in sd if k.endswith(".weight") and sd[k].dim() == 4]) - 2


def scale_of(sd):
    last = 2 * (num_conv_of(sd) + 1)
    return int(round((sd[f"body.{last}.weight"].shape[0] / 3) ** 0.5))


def body(sd, x, q=lambda t: t):
    n = num_conv_of(sd)
    out = x
    for i in range(n + 2):
        out = q(F.conv2d(out, sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"], padding=1))
        if i <= n:
            out = q(F.prelu(out, sd[f"body.{2 * i + 1}.weight"]))
    return out


def forward(sd, x, q=lambda t: t):
    """x [B, 3, H, W] fp32 in [0, 1] -> [B, 3, H r, W r] fp32."""
    r = scale_of(sd)
    return q(F.pixel_shuffle(body(sd, x, q), r) + F.interpolate(x, scale_factor=r, mode="nearest"))


def base(sd, x):
    return F.interpolate(x, scale_factor=scale_of(sd), mode="nearest")


def fp16_twin(sd, x):
    from fp16_emu import r16
    return forward({k: (r16(v) if v.dim() == 4 else v) for k, v in sd.items()}, x, r16)


class CompactModule(torch.nn.Module):
    """The reference as a module (what a webui scaler holds), for the job-level comparison."""

    def __init__(self, sd):
        super().__init__()
        self.sd = {k: v.clone() for k, v in sd.items()}

    def forward(self, x):
        return forward(self.sd, x)
