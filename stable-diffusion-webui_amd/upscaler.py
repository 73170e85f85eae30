"""Image-space upscaler hand-off used by the non-latent hires fix.

The engine's part is decode -> [host image resize] -> encode; the resize itself stays the reference's job.  This module is
the seam: the registry ``shared.sd_upscalers`` of ``UpscalerData(name, path, scaler)`` entries the reference's code looks names
up in (modules/images.py:276, modules/modelloader.py:136), the ``Upscaler.upscale`` driver loop (modules/upscaler.py:54-76) and
the three built-in PIL scalers (None / Lanczos / Nearest, modules/upscaler.py:107-154).  The RRDBNet family (ESRGAN, Real-ESRGAN) and the
compact Real-ESRGAN models (SRVGGNetCompact: General 4xV3, General WDN 4xV3, AnimeVideo) run on the engine (``UpscalerESRGAN`` /
``register_esrgan`` below, csrc/rrdb.hip and csrc/compact.hip), and so do the SwinIR models with the nearest+conv upsampler
(``SwinIRNet``) and the Swin2SR models (``Swin2SRNet``; both csrc/swinir.hip) and the ScuNET models (``ScuNETNet``, csrc/scunet.hip) and the DAT models (``DATNet``, csrc/dat.hip) and the HAT models (``HATNet``, csrc/hat.hip); other model upscalers register their own ``UpscalerData`` whose ``scaler.upscale(img, scale, path)``
is called as in the reference.
"""
from __future__ import annotations

import os
import re

import numpy as np
from PIL import Image

from . import shared

LANCZOS = (Image.Resampling.LANCZOS if hasattr(Image, 'Resampling') else Image.LANCZOS)
NEAREST = (Image.Resampling.NEAREST if hasattr(Image, 'Resampling') else Image.NEAREST)


class UpscalerData:
    """A selectable upscaler: what shared.sd_upscalers holds (modules/upscaler.py:87-104)."""

    def __init__(self, name, path, upscaler=None, scale=4, model=None):
        self.name, self.data_path, self.local_data_path = name, path, path
        self.scaler, self.scale, self.model = upscaler, scale, model

    def __repr__(self):
        return f"<UpscalerData name={self.name} path={self.data_path} scale={self.scale}>"


class Upscaler:
    """Base class with the reference's driver (modules/upscaler.py:54-76): a scaler may enlarge by less than asked for, so it
    is applied up to three times until the (8-aligned) destination size is covered, then the result is fitted with LANCZOS."""
    name = None

    def __init__(self):
        self.scale = 1
        self.scalers = []

    def do_upscale(self, img, selected_model=None):
        return img

    def upscale(self, img, scale, selected_model=None):
        self.scale = scale
        dest_w, dest_h = int((img.width * scale) // 8 * 8), int((img.height * scale) // 8 * 8)
        for attempt in range(3):
            covered = img.width >= dest_w and img.height >= dest_h
            if (covered and (attempt > 0 or scale != 1)) or shared.state.interrupted:
                break
            before = (img.width, img.height)
            img = self.do_upscale(img, selected_model)
            if before == (img.width, img.height):
                break
        if (img.width, img.height) != (dest_w, dest_h):
            img = img.resize((dest_w, dest_h), resample=LANCZOS)
        return img


class _PilUpscaler(Upscaler):
    """The built-in scalers that are one PIL resize (modules/upscaler.py:107-154): "None" (identity), "Lanczos", "Nearest"."""
    resample = None

    def __init__(self):
        super().__init__()
        self.scalers = [UpscalerData(self.name, None, self)]

    def do_upscale(self, img, selected_model=None):
        if self.resample is None:
            return img
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=self.resample)


class UpscalerNone(_PilUpscaler):
    name = "None"


class UpscalerLanczos(_PilUpscaler):
    name, resample = "Lanczos", LANCZOS


class UpscalerNearest(_PilUpscaler):
    name, resample = "Nearest", NEAREST


def builtin_upscalers():
    """The order modelloader.load_upscalers leaves the built-ins in (:136-141: "None" first, then by name)."""
    return [*UpscalerNone().scalers, *UpscalerLanczos().scalers, *UpscalerNearest().scalers]


# ---- RRDBNet upscalers on the engine ----------------------------------------------------------------------------------------------
_NEW_CONVS = ("conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last")
_OLD_TO_NEW = {"model.0": "conv_first", "model.3": "conv_up1", "model.6": "conv_up2", "model.8": "conv_hr", "model.10": "conv_last"}


def _old_arch_to_new(sd):
    """The original ESRGAN key layout (model.0, model.1.sub.{i}.RDB{j}.conv{k}.0, model.1.sub.{nb}, model.3 / 6 / 8 / 10) renamed to
    BasicSR's, as the webui does on load (the x4 layout only: other scales put their up-convs elsewhere)."""
    tops = {m.group(1) for k in sd for m in [re.match(r"model\.(\d+)\.(weight|bias)$", k)] if m}
    if tops != {"0", "3", "6", "8", "10"}:
        raise ValueError(f"old-arch ESRGAN checkpoint is not a x4 model (top-level convs model.{sorted(tops, key=int)})")
    subs = [int(m.group(1)) for k in sd for m in [re.match(r"model\.1\.sub\.(\d+)\.weight$", k)] if m]
    if len(subs) != 1:
        raise ValueError("old-arch ESRGAN checkpoint without its trunk conv (model.1.sub.<num_block>)")
    nb, out = subs[0], {}
    for k, v in sd.items():
        stem, leaf = k.rsplit(".", 1)
        m = re.match(r"model\.1\.sub\.(\d+)\.RDB(\d)\.conv(\d)\.0$", stem)
        if m:
            out[f"body.{m.group(1)}.rdb{m.group(2)}.conv{m.group(3)}.{leaf}"] = v
        elif stem == f"model.1.sub.{nb}":
            out[f"conv_body.{leaf}"] = v
        elif stem in _OLD_TO_NEW:
            out[f"{_OLD_TO_NEW[stem]}.{leaf}"] = v
        else:
            raise ValueError(f"unexpected key in an old-arch ESRGAN checkpoint: {k}")
    return out


def _as_f32(t):
    return np.asarray(t.detach().float().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32).ravel()


def _unwrap_state_dict(sd):
    for wrap in ("params_ema", "params"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    return {k: v for k, v in sd.items() if hasattr(v, "shape")}


def parse_esrgan_state_dict(sd):
    """Checkpoint state dict -> (blob, num_block, in_ch, scale): the engine's weight blob (fp32, every conv's OIHW weight then its bias,
    in checkpoint order — sdmi_esrgan_create), the number of RRDBs read from the keys (23, or 6 for the anime model) and the scale read
    from conv_first's input channels (3 -> x4, 12 -> x2, 48 -> x1: pixel-unshuffle in front).  Host only.  Raises ValueError on anything
    that is not a 64-feature / 32-growth RRDBNet."""
    sd = _unwrap_state_dict(sd)
    if "model.0.weight" in sd:
        sd = _old_arch_to_new(sd)
    if "conv_first.weight" not in sd:
        raise ValueError("not an RRDBNet checkpoint: neither conv_first.weight nor model.0.weight")
    blocks = sorted({int(m.group(1)) for k in sd for m in [re.match(r"body\.(\d+)\.rdb1\.conv1\.weight$", k)] if m})
    num_block = len(blocks)
    if num_block == 0 or blocks != list(range(num_block)):
        raise ValueError(f"RRDBNet body blocks are not 0..n-1: {blocks}")
    names = ["conv_first"] + [f"body.{i}.rdb{j}.conv{k}" for i in range(num_block) for j in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
    names += list(_NEW_CONVS[1:])
    missing = [n + leaf for n in names for leaf in (".weight", ".bias") if n + leaf not in sd]
    if missing:
        raise ValueError(f"RRDBNet checkpoint lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    num_feat, in_ch = int(sd["conv_first.weight"].shape[0]), int(sd["conv_first.weight"].shape[1])
    growth = int(sd["body.0.rdb1.conv1.weight"].shape[0])
    if num_feat != 64:
        raise ValueError(f"RRDBNet num_feat = {num_feat}: the engine's kernels are built for 64")
    if growth != 32:
        raise ValueError(f"RRDBNet num_grow_ch = {growth}: the engine's kernels are built for 32")
    if in_ch not in (3, 12, 48):
        raise ValueError(f"RRDBNet conv_first takes {in_ch} channels: expected 3 (x4), 12 (x2) or 48 (x1)")
    scale = {3: 4, 12: 2, 48: 1}[in_ch]
    parts = []
    for n in names:
        k = int(n[-1]) if ".conv" in n else 0
        want = {"conv_first": (64, in_ch), "conv_last": (3, 64)}.get(n, ((32 if k < 5 else 64, 64 + 32 * (k - 1)) if k else (64, 64)))
        w, b = sd[n + ".weight"], sd[n + ".bias"]
        if tuple(w.shape) != (*want, 3, 3) or tuple(b.shape) != (want[0],):
            raise ValueError(f"RRDBNet {n}: weight {tuple(w.shape)}, expected {(*want, 3, 3)}")
        parts += [_as_f32(w), _as_f32(b)]
    return np.ascontiguousarray(np.concatenate(parts)), num_block, in_ch, scale


def parse_compact_state_dict(sd):
    """Checkpoint state dict of a compact Real-ESRGAN model (SRVGGNetCompact, realesrgan/archs/srvgg_arch.py: body.{2i} = conv i,
    body.{2i+1} = the PReLU after it, none after the last conv) -> (blob, num_conv, scale): the engine's weight blob (fp32, per conv
    the OIHW weight, the bias, then — all but the last conv — the 64 PReLU slopes: sdmi_compact_create), the number of body convs read
    from the key indices (32 for General 4xV3, 16 for AnimeVideo) and the scale r = sqrt(out_ch / 3) of the last conv.  Host only.
    Raises ValueError on anything that is not a 64-feature, 3-channel, PReLU network of scale 1..4."""
    sd = _unwrap_state_dict(sd)
    convs = sorted(int(m.group(1)) for k in sd for m in [re.match(r"body\.(\d+)\.weight$", k)] if m and len(sd[k].shape) == 4)
    if "body.0.weight" not in sd or len(sd["body.0.weight"].shape) != 4:
        raise ValueError("not a compact (SRVGGNetCompact) checkpoint: no 4-d body.0.weight")
    if len(convs) < 3 or convs != list(range(0, 2 * len(convs), 2)):
        raise ValueError(f"compact network: conv indices are not body.0, body.2, ... without gaps: {convs[:6]}{' ...' if len(convs) > 6 else ''}")
    num_conv = len(convs) - 2
    feat, in_ch = int(sd["body.0.weight"].shape[0]), int(sd["body.0.weight"].shape[1])
    if feat != 64:
        raise ValueError(f"compact network num_feat = {feat}: the engine's kernel is built for 64")
    if in_ch != 3:
        raise ValueError(f"compact network takes {in_ch} input channels: expected 3")
    out_ch = int(sd[f"body.{convs[-1]}.weight"].shape[0])
    scale = int(round((out_ch / 3.0) ** 0.5))
    if out_ch != 3 * scale * scale or scale not in (1, 2, 3, 4):
        raise ValueError(f"compact network: the last conv has {out_ch} channels, expected 3 r^2 with scale r in 1..4")
    parts = []
    for n, i in enumerate(convs):
        want = (64 if n <= num_conv else out_ch, 3 if n == 0 else 64, 3, 3)
        w, b = sd[f"body.{i}.weight"], sd.get(f"body.{i}.bias")
        if tuple(w.shape) != want:
            raise ValueError(f"compact network body.{i}: weight {tuple(w.shape)}, expected {want} (3x3 convs of 64 features)")
        if b is None or tuple(b.shape) != (want[0],):
            raise ValueError(f"compact network body.{i}: bias missing or not of shape {(want[0],)}")
        parts += [_as_f32(w), _as_f32(b)]
        if n <= num_conv:
            a = sd.get(f"body.{i + 1}.weight")
            if a is None or tuple(a.shape) != (64,):
                raise ValueError(f"compact network body.{i + 1}: no PReLU weight of shape (64,) (a relu / leakyrelu build has none; "
                                 f"only act_type = 'prelu' runs on the engine)")
            parts.append(_as_f32(a))
    return np.ascontiguousarray(np.concatenate(parts)), num_conv, scale


SWINIR_MARK = "layers.0.residual_group.blocks.0.attn.qkv.weight"


# What the SwinIR and the Swin2SR parser share (`family`: the name their messages open with)
def _swin_tensor(sd, family, name, shape=None):
    """sd[name] as flat fp32, of this shape where one is given — or say what is wrong."""
    t = sd.get(name)
    if t is None or (shape is not None and tuple(t.shape) != shape):
        raise ValueError(f"{family} {name}: {None if t is None else tuple(t.shape)}, expected {shape}")
    return _as_f32(t)


def _swin_wb(sd, family, name, shape):
    """[weight, bias] of the layer `name` as flat fp32, the weight of this shape — or say what is wrong."""
    w, b = sd.get(name + ".weight"), sd.get(name + ".bias")
    if w is None or b is None:
        raise ValueError(f"{family} checkpoint lacks {name}.{'weight' if w is None else 'bias'}")
    if tuple(w.shape) != shape or tuple(b.shape) != (shape[0],):
        raise ValueError(f"{family} {name}: weight {tuple(w.shape)}, expected {shape}")
    return [_as_f32(w), _as_f32(b)]


def _swin_depths(sd, family):
    """The blocks of every layer, counted from the keys."""
    layers = sorted({int(m.group(1)) for k in sd for m in [re.match(r"layers\.(\d+)\.residual_group\.blocks\.0\.attn\.qkv\.weight$", k)] if m})
    if not layers or layers != list(range(len(layers))) or len(layers) > 16:
        raise ValueError(f"{family} layers are not 0..n-1 with 1 <= n <= 16: {layers}")
    depths = []
    for i in layers:
        blocks = sorted({int(m.group(1)) for k in sd for m in [re.match(rf"layers\.{i}\.residual_group\.blocks\.(\d+)\.attn\.qkv\.weight$", k)] if m})
        if blocks != list(range(len(blocks))):
            raise ValueError(f"{family} layers.{i}: blocks are not 0..n-1: {blocks}")
        depths.append(len(blocks))
    return depths


def _swin_trunk(sd, family, c, heads):
    """-> (mlp_hidden, resi_3conv, resi): the trunk facts read off the first block and the first layer's closing conv, refused where the
    engine's kernels are not built for them; resi(stem) lists the (name, weight shape) of a closing conv (1conv | 3conv)."""
    if c % heads or c // heads > 32:
        raise ValueError(f"{family} head_dim = {c}/{heads} = {c / heads:g}: the engine's attention kernel is built for head_dim <= 32")
    b0 = "layers.0.residual_group.blocks.0."
    if b0 + "mlp.fc1.weight" not in sd:
        raise ValueError(f"{family} checkpoint lacks {b0}mlp.fc1.weight")
    hidden = int(sd[b0 + "mlp.fc1.weight"].shape[0])
    resi3 = "layers.0.conv.0.weight" in sd
    if not resi3 and "layers.0.conv.weight" not in sd:
        raise ValueError(f"{family} checkpoint lacks layers.0.conv (.weight for 1conv, .0 / .2 / .4 for 3conv)")
    if resi3 and (c % 4 or c // 4 > 64):
        raise ValueError(f"{family} 3conv with embed_dim {c}: the engine packs embed_dim / 4 <= 64 channels")
    q = c // 4
    resi = (lambda stem: [(stem + ".0", (q, c, 3, 3)), (stem + ".2", (q, q, 1, 1)), (stem + ".4", (c, q, 3, 3))]) if resi3 \
        else (lambda stem: [(stem, (c, c, 3, 3))])
    return hidden, resi3, resi


def parse_swinir_state_dict(sd):
    """Checkpoint state dict of a SwinIR network with the nearest+conv upsampler (the real-world SR models: SwinIR-L x4 GAN, the M
    models x4 / x2) -> (blob, config): the engine's weight blob (fp32, every tensor flattened in the order include/sdmi.h documents at
    sdmi_swinir_config: conv_first; patch_embed.norm; per layer its blocks' norm1, relative_position_bias_table, qkv, proj, norm2, fc1,
    fc2, then the layer's conv(s); norm; conv_after_body; conv_before_upsample.0; conv_up1; conv_up2 (x4); conv_hr; conv_last — weight
    then bias) and config = dict(embed_dim, depths, num_heads, mlp_hidden, resi_3conv, scale), all read from the checkpoint.  The
    buffers relative_position_index / attn_mask are ignored.  Host only.  Raises ValueError on what the engine's kernels are not built
    for: another upsampler, window size, head dim > 32, ape, other channel counts."""
    sd = _unwrap_state_dict(sd)
    if SWINIR_MARK not in sd or "conv_first.weight" not in sd:
        raise ValueError(f"not a SwinIR checkpoint: no {SWINIR_MARK}")
    if "absolute_pos_embed" in sd:
        raise ValueError("SwinIR with ape (absolute_pos_embed): the engine runs the models without it")
    if "conv_before_upsample.0.weight" not in sd or "conv_up1.weight" not in sd or "conv_hr.weight" not in sd:
        kind = ("pixelshuffle" if "upsample.0.weight" in sd and "conv_before_upsample.0.weight" in sd
                else "pixelshuffledirect" if "upsample.0.weight" in sd else "none")
        raise ValueError(f"SwinIR upsampler '{kind}': the engine runs the nearest+conv upsampler only (conv_before_upsample.0, conv_up1, conv_hr)")
    c, in_ch = int(sd["conv_first.weight"].shape[0]), int(sd["conv_first.weight"].shape[1])
    if in_ch != 3 or tuple(sd["conv_first.weight"].shape[2:]) != (3, 3):
        raise ValueError(f"SwinIR conv_first takes {in_ch} input channels: expected 3")
    depths = _swin_depths(sd, "SwinIR")
    b0 = "layers.0.residual_group.blocks.0."
    table = sd.get(b0 + "attn.relative_position_bias_table")
    if table is None or len(table.shape) != 2:
        raise ValueError(f"SwinIR checkpoint lacks {b0}attn.relative_position_bias_table")
    heads = int(table.shape[1])
    if int(table.shape[0]) != 225:
        w = (int(round(int(table.shape[0]) ** 0.5)) + 1) // 2
        raise ValueError(f"SwinIR window_size {w} (a {int(table.shape[0])}-row bias table): the engine's attention kernel is built for 8 (225 rows)")
    hidden, resi3, resi = _swin_trunk(sd, "SwinIR", c, heads)
    if int(sd["conv_before_upsample.0.weight"].shape[0]) != 64:
        raise ValueError(f"SwinIR num_feat = {int(sd['conv_before_upsample.0.weight'].shape[0])}: the engine's tail kernel is built for 64")
    if int(sd["conv_last.weight"].shape[0]) != 3:
        raise ValueError(f"SwinIR conv_last writes {int(sd['conv_last.weight'].shape[0])} channels: expected 3")
    scale = 4 if "conv_up2.weight" in sd else 2
    want = [("conv_first", (c, 3, 3, 3)), ("patch_embed.norm", (c,))]
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            want += [(b + "norm1", (c,)), (b + "attn.relative_position_bias_table", (225, heads)), (b + "attn.qkv", (3 * c, c)),
                     (b + "attn.proj", (c, c)), (b + "norm2", (c,)), (b + "mlp.fc1", (hidden, c)), (b + "mlp.fc2", (c, hidden))]
        want += resi(f"layers.{i}.conv")
    want += [("norm", (c,))] + resi("conv_after_body") + [("conv_before_upsample.0", (64, c, 3, 3)), ("conv_up1", (64, 64, 3, 3))]
    want += ([("conv_up2", (64, 64, 3, 3))] if scale == 4 else []) + [("conv_hr", (64, 64, 3, 3)), ("conv_last", (3, 64, 3, 3))]
    parts = []
    for name, shape in want:
        if name.endswith("relative_position_bias_table"):
            parts.append(_swin_tensor(sd, "SwinIR", name, shape))
        else:
            parts += _swin_wb(sd, "SwinIR", name, shape)
    config = dict(embed_dim=c, depths=tuple(depths), num_heads=heads, mlp_hidden=hidden, resi_3conv=int(resi3), scale=scale)
    return np.ascontiguousarray(np.concatenate(parts)), config


SWIN2SR_MARK = "layers.0.residual_group.blocks.0.attn.logit_scale"
SWIN2SR_UPSAMPLERS = ("nearest+conv", "pixelshuffle", "pixelshuffledirect")


def swin2sr_coords_table():
    """[225, 2] fp32: the log-spaced relative coordinates of an 8 x 8 window (WindowAttention of network_swin2sr.py): offsets -7..7
    / 7 * 8, then sign(x) log2(|x| + 1) / log2(8); row (dy + 7) * 15 + (dx + 7) = (y, x)."""
    d = np.arange(-7, 8, dtype=np.float32) / np.float32(7) * np.float32(8)
    t = np.stack(np.meshgrid(d, d, indexing="ij"), axis=-1).reshape(225, 2).astype(np.float32)
    return (np.sign(t) * np.log2(np.abs(t) + np.float32(1)) / np.float32(np.log2(8.0))).astype(np.float32)


def swin2sr_bias_table(w0, b0, w2):
    """16 sigmoid(cpb_mlp(coords)) -> [225, heads] fp32, computed in fp32: cpb_mlp = Linear(2, hidden) + ReLU + Linear(hidden, heads,
    bias=False)."""
    w0, b0, w2 = (np.asarray(t, dtype=np.float32) for t in (w0, b0, w2))
    hid = np.maximum(swin2sr_coords_table() @ w0.T + b0, np.float32(0))
    z = (hid @ w2.T).astype(np.float32)
    return (np.float32(16) / (np.float32(1) + np.exp(-z))).astype(np.float32)


def swin2sr_head_scale(logit_scale):
    """exp(min(logit_scale, ln 100)) -> [heads] fp32."""
    return np.exp(np.minimum(np.asarray(logit_scale, dtype=np.float32).ravel(), np.float32(np.log(100.0)))).astype(np.float32)


def parse_swin2sr_state_dict(sd):
    """Checkpoint state dict of a Swin2SR network (network_swin2sr.py; the webui's swinir_model_arch_v2.py) -> (blob, config): the
    engine's weight blob (fp32, in the order include/sdmi.h documents at sdmi_swin2sr_config: conv_first; patch_embed.proj (the identity
    where a checkpoint has none); patch_embed.norm; per block
    attn.qkv with the bias (q_bias | 0 | v_bias), the ready bias table 16 sigmoid(cpb_mlp(coords)) [225][heads], head_scale =
    exp(min(logit_scale, ln 100)), attn.proj, norm1, mlp.fc1, mlp.fc2, norm2; the layer's conv(s), the last with the layer's patch_embed.proj folded in (P W, P b + p:
    nothing else reads that conv); norm; conv_after_body; the tail) and
    config = dict(embed_dim, depths, num_heads, mlp_hidden, resi_3conv, upsampler, scale), upsampler one of SWIN2SR_UPSAMPLERS, read
    from the tail keys.  The buffers relative_coords_table / relative_position_index / attn_mask are ignored.  Host only.  Raises
    ValueError on what the engine's kernels are not built for."""
    sd = _unwrap_state_dict(sd)
    if SWIN2SR_MARK not in sd or "conv_first.weight" not in sd:
        raise ValueError(f"not a Swin2SR checkpoint: no {SWIN2SR_MARK}")
    if "absolute_pos_embed" in sd:
        raise ValueError("Swin2SR with ape (absolute_pos_embed): the engine runs the models without it")
    if "conv_bicubic.weight" in sd or "conv_aux.weight" in sd:
        raise ValueError("Swin2SR upsampler 'pixelshuffle_aux' (conv_bicubic / conv_aux): the engine runs nearest+conv, pixelshuffle and "
                         "pixelshuffledirect")
    if "conv_up1.weight" in sd and "conv_hr.weight" in sd and "conv_before_upsample.0.weight" in sd:
        upsampler = 0
    elif "upsample.0.weight" in sd:
        upsampler = 1 if "conv_before_upsample.0.weight" in sd else 2
    else:
        raise ValueError("Swin2SR without an upsampler (no conv_up1 / conv_hr, no upsample.0: a denoising / JPEG model): the engine runs "
                         "the super-resolution models")
    c, in_ch = int(sd["conv_first.weight"].shape[0]), int(sd["conv_first.weight"].shape[1])
    if in_ch != 3 or tuple(sd["conv_first.weight"].shape[2:]) != (3, 3):
        raise ValueError(f"Swin2SR conv_first takes {in_ch} input channels: expected 3")
    depths = _swin_depths(sd, "Swin2SR")
    heads = int(sd[SWIN2SR_MARK].shape[0])
    for k, v in sd.items():                                  # the cpb grid is computed, not stored: the window shows in the buffers
        side = None
        if k.endswith("attn.relative_position_index") and tuple(v.shape) != (64, 64):
            side = int(round(int(v.shape[0]) ** 0.5))
        elif k.endswith("attn_mask") and tuple(v.shape[1:]) != (64, 64):
            side = int(round(int(v.shape[-1]) ** 0.5))
        elif k.endswith("attn.relative_coords_table") and tuple(v.shape[1:3]) != (15, 15):
            side = (int(v.shape[1]) + 1) // 2
        if side is not None:
            raise ValueError(f"Swin2SR window_size {side} ({k} {tuple(v.shape)}): the engine's attention kernel is built for 8")
    hidden, resi3, resi = _swin_trunk(sd, "Swin2SR", c, heads)
    if upsampler != 2 and int(sd["conv_before_upsample.0.weight"].shape[0]) != 64:
        raise ValueError(f"Swin2SR num_feat = {int(sd['conv_before_upsample.0.weight'].shape[0])}: the engine's tail kernels are built for 64")
    if upsampler == 0:
        if "conv_up2.weight" not in sd:
            raise ValueError("Swin2SR nearest+conv without conv_up2 (scale 2): the architecture has this upsampler at scale 4 only")
        scale = 4
        tail = [("conv_before_upsample.0", (64, c, 3, 3)), ("conv_up1", (64, 64, 3, 3)), ("conv_up2", (64, 64, 3, 3)),
                ("conv_hr", (64, 64, 3, 3)), ("conv_last", (3, 64, 3, 3))]
    elif upsampler == 1:
        n0 = int(sd["upsample.0.weight"].shape[0])
        scale = {(256, False): 2, (576, False): 3, (256, True): 4}.get((n0, "upsample.2.weight" in sd))
        if scale is None or any(f"upsample.{k}.weight" in sd for k in (4, 6)):
            raise ValueError(f"Swin2SR pixelshuffle with upsample.0 writing {n0} channels"
                             f"{' and further steps' if 'upsample.2.weight' in sd else ''}: the engine runs scales 2, 3 and 4")
        tail = [("conv_before_upsample.0", (64, c, 3, 3)), ("upsample.0", (n0, 64, 3, 3))]
        tail += ([("upsample.2", (256, 64, 3, 3))] if scale == 4 else []) + [("conv_last", (3, 64, 3, 3))]
    else:
        n0 = int(sd["upsample.0.weight"].shape[0])
        scale = {12: 2, 27: 3, 48: 4}.get(n0)
        if scale is None:
            raise ValueError(f"Swin2SR pixelshuffledirect with upsample.0 writing {n0} channels: the engine runs scales 2, 3 and 4 "
                             f"(12, 27, 48 channels)")
        tail = [("upsample.0", (n0, c, 3, 3))]
    parts = []

    def wb(name, shape):
        parts.extend(_swin_wb(sd, "Swin2SR", name, shape))

    def tensor(name, shape=None):
        return _swin_tensor(sd, "Swin2SR", name, shape)

    def proj_of(stem):
        """PatchEmbed.proj of network_swin2sr.py, a 1x1 conv C -> C, as ([C, C], [C]) float64; the identity where a checkpoint has none."""
        if stem + ".weight" not in sd:
            return np.eye(c, dtype=np.float64), np.zeros(c, dtype=np.float64)
        w, b = tensor(stem + ".weight", (c, c, 1, 1)), tensor(stem + ".bias", (c,))
        return w.reshape(c, c).astype(np.float64), b.astype(np.float64)

    def wb_then_proj(name, shape, stem):
        """A conv whose output feeds only the 1x1 conv `stem`: the two are one conv, P W and P b + p (float64 on the host)."""
        wb(name, shape)
        if stem + ".weight" in sd:
            pw, pb = proj_of(stem)
            w, b = parts[-2].astype(np.float64).reshape(shape[0], -1), parts[-1].astype(np.float64)
            parts[-2:] = [(pw @ w).astype(np.float32).ravel(), (pw @ b + pb).astype(np.float32)]

    wb("conv_first", (c, 3, 3, 3))
    pw, pb = proj_of("patch_embed.proj")
    parts.extend([pw.astype(np.float32).ravel(), pb.astype(np.float32)])
    wb("patch_embed.norm", (c,))
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            qb, vb = sd.get(b + "attn.q_bias"), sd.get(b + "attn.v_bias")
            zeros = np.zeros(c, dtype=np.float32)
            parts += [tensor(b + "attn.qkv.weight", (3 * c, c)), zeros if qb is None else tensor(b + "attn.q_bias", (c,)), zeros,
                      zeros if vb is None else tensor(b + "attn.v_bias", (c,))]
            w0 = tensor(b + "attn.cpb_mlp.0.weight")
            if w0.size % 2:
                raise ValueError(f"Swin2SR {b}attn.cpb_mlp.0.weight: {tuple(sd[b + 'attn.cpb_mlp.0.weight'].shape)}, expected (hidden, 2)")
            hid = w0.size // 2
            table = swin2sr_bias_table(w0.reshape(hid, 2), tensor(b + "attn.cpb_mlp.0.bias", (hid,)),
                                       tensor(b + "attn.cpb_mlp.2.weight", (heads, hid)).reshape(heads, hid))
            parts += [table.ravel(), swin2sr_head_scale(tensor(b + "attn.logit_scale", (heads, 1, 1)))]
            wb(b + "attn.proj", (c, c))
            wb(b + "norm1", (c,))
            wb(b + "mlp.fc1", (hidden, c))
            wb(b + "mlp.fc2", (c, hidden))
            wb(b + "norm2", (c,))
        convs = resi(f"layers.{i}.conv")
        for name, shape in convs[:-1]:
            wb(name, shape)
        wb_then_proj(*convs[-1], f"layers.{i}.patch_embed.proj")
    wb("norm", (c,))
    for name, shape in resi("conv_after_body") + tail:
        wb(name, shape)
    config = dict(embed_dim=c, depths=tuple(depths), num_heads=heads, mlp_hidden=hidden, resi_3conv=int(resi3),
                  upsampler=SWIN2SR_UPSAMPLERS[upsampler], scale=scale)
    return np.ascontiguousarray(np.concatenate(parts)), config


SCUNET_MARKS = ("m_head.0.weight", "m_down1.0.trans_block.msa.relative_position_params")
SCUNET_STAGES = ("m_down1", "m_down2", "m_down3", "m_body", "m_up3", "m_up2", "m_up1")


def parse_scunet_state_dict(sd):
    """Checkpoint state dict of a SCUNet (network_scunet.py; the webui's "ScuNET GAN" / "ScuNET PSNR": in_nc 3, dim 64, config [4] * 7) ->
    (blob, config): the engine's weight blob (fp32, every tensor flattened in the order include/sdmi.h documents at sdmi_scunet_config:
    m_head; per stage the ConvTranspose2d (m_up*), its blocks' ln1, relative_position_params, embedding_layer, linear, ln2, mlp.0,
    mlp.2, conv1_1, conv1_2, conv_block.0, conv_block.2, the stride-2 Conv2d (m_down*); m_tail) and config = dict(depths, dim, scale),
    the depths read by counting blocks.  Host only.  Raises ValueError on what the engine's kernels are not built for: dim other than
    64, a window other than 8, in_nc other than 3, and on missing or misshapen tensors."""
    sd = _unwrap_state_dict(sd)
    if any(k not in sd for k in SCUNET_MARKS):
        raise ValueError(f"not a ScuNET checkpoint: no {' / '.join(k for k in SCUNET_MARKS if k not in sd)}")
    head = sd["m_head.0.weight"]
    dim, in_nc = int(head.shape[0]), int(head.shape[1])
    if in_nc != 3:
        raise ValueError(f"ScuNET m_head takes in_nc = {in_nc} channels: the engine runs the colour models (3)")
    if dim != 64:
        raise ValueError(f"ScuNET dim = {dim}: the engine's kernels are built for 64")
    params = sd[SCUNET_MARKS[1]]
    if tuple(params.shape[1:]) != (15, 15):
        side = int(params.shape[-1])
        raise ValueError(f"ScuNET window_size {(side + 1) // 2} (relative_position_params {tuple(params.shape)}): the engine's kernels are "
                         f"built for 8 ([heads][15][15])")
    depths = []
    for st, stem in enumerate(SCUNET_STAGES):
        first = 1 if st > 3 else 0                           # m_up*: the ConvTranspose2d sits at index 0
        blocks = sorted({int(m.group(1)) for k in sd for m in [re.match(rf"{stem}\.(\d+)\.conv1_1\.weight$", k)] if m})
        if not blocks or blocks != list(range(first, first + len(blocks))):
            raise ValueError(f"ScuNET {stem}: blocks are not {first}..n: {blocks}")
        depths.append(len(blocks))
    want = [("m_head.0.weight", (64, 3, 3, 3))]
    for st, (stem, depth) in enumerate(zip(SCUNET_STAGES, depths)):
        c = 32 << (st if st < 4 else 6 - st)
        d = 2 * c
        first = 1 if st > 3 else 0
        if st > 3:
            want.append((f"{stem}.0.weight", (2 * d, d, 2, 2)))
        for i in range(first, first + depth):
            b, t = f"{stem}.{i}.", f"{stem}.{i}.trans_block."
            want += [(t + "ln1.weight", (c,)), (t + "ln1.bias", (c,)), (t + "msa.relative_position_params", (c // 32, 15, 15)),
                     (t + "msa.embedding_layer.weight", (3 * c, c)), (t + "msa.embedding_layer.bias", (3 * c,)),
                     (t + "msa.linear.weight", (c, c)), (t + "msa.linear.bias", (c,)), (t + "ln2.weight", (c,)), (t + "ln2.bias", (c,)),
                     (t + "mlp.0.weight", (4 * c, c)), (t + "mlp.0.bias", (4 * c,)), (t + "mlp.2.weight", (c, 4 * c)), (t + "mlp.2.bias", (c,)),
                     (b + "conv1_1.weight", (d, d, 1, 1)), (b + "conv1_1.bias", (d,)), (b + "conv1_2.weight", (d, d, 1, 1)),
                     (b + "conv1_2.bias", (d,)), (b + "conv_block.0.weight", (c, c, 3, 3)), (b + "conv_block.2.weight", (c, c, 3, 3))]
        if st < 3:
            want.append((f"{stem}.{depth}.weight", (2 * d, d, 2, 2)))
    want.append(("m_tail.0.weight", (3, 64, 3, 3)))
    parts = []
    for name, shape in want:
        t = sd.get(name)
        if t is None:
            raise ValueError(f"ScuNET checkpoint lacks {name}")
        if tuple(t.shape) != shape:
            raise ValueError(f"ScuNET {name}: {tuple(t.shape)}, expected {shape}")
        parts.append(_as_f32(t))
    return np.ascontiguousarray(np.concatenate(parts)), dict(depths=tuple(depths), dim=dim, scale=1)


DAT_MARKS = ("before_RG.1.weight", "layers.0.blocks.0.attn.attns.0.pos.pos_proj.weight")
DAT_SPLITS = {15 * 31: (8, 16), 15 * 63: (8, 32)}           # rows of attns.0.rpe_biases = (2 s0 - 1)(2 s1 - 1)
_BN_EPS = np.float32(1e-5)


def _ln_f32(x, g, b):
    mu = x.mean(axis=-1, keepdims=True, dtype=np.float32)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True, dtype=np.float32)
    return ((x - mu) / np.sqrt(var + np.float32(1e-5)) * g + b).astype(np.float32)


def dat_position_bias(pos, hsp, wsp):
    """The dynamic position bias of one attention branch (DynamicPosBias, residual = False) evaluated in fp32 at the (2 hsp - 1)(2 wsp - 1)
    integer offsets (dy, dx), dy in [1 - hsp, hsp - 1] outer, dx in [1 - wsp, wsp - 1] inner -> [offsets, heads / 2].  pos: name ->
    fp32 array for pos_proj, pos1.0, pos1.2, pos2.0, pos2.2, pos3.0, pos3.2 (.weight / .bias): pos3(pos2(pos1(pos_proj(r)))), every posK
    a LayerNorm, ReLU, Linear."""
    dy, dx = np.meshgrid(np.arange(1 - hsp, hsp, dtype=np.float32), np.arange(1 - wsp, wsp, dtype=np.float32), indexing="ij")
    x = np.stack([dy.ravel(), dx.ravel()], axis=1).astype(np.float32)
    x = (x @ pos["pos_proj.weight"].T + pos["pos_proj.bias"]).astype(np.float32)
    for k in ("pos1", "pos2", "pos3"):
        x = np.maximum(_ln_f32(x, pos[k + ".0.weight"], pos[k + ".0.bias"]), np.float32(0))
        x = (x @ pos[k + ".2.weight"].T + pos[k + ".2.bias"]).astype(np.float32)
    return np.ascontiguousarray(x)


def dat_bn_fold(w, b, gamma, beta, mean, var):
    """Conv (weight [O, ...], bias [O]) followed by an eval-mode BatchNorm2d (eps 1e-5) as one conv, in fp32 -> (weight, bias)."""
    w, b, gamma, beta, mean, var = (np.asarray(t, dtype=np.float32) for t in (w, b, gamma, beta, mean, var))
    s = (gamma / np.sqrt(var + _BN_EPS)).astype(np.float32)
    return (w * s.reshape((-1,) + (1,) * (w.ndim - 1))).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)


def parse_dat_state_dict(sd):
    """Checkpoint state dict of a DAT network (basicsr's dat_arch.py with upsampler 'pixelshuffle' and resi_connection '1conv': the
    webui's "DAT x2" / "DAT x3" / "DAT x4", DAT-S, DAT-2) -> (blob, config): the engine's weight blob (fp32, in the order include/sdmi.h
    documents at sdmi_dat_config, every tensor in the checkpoint's channel order; the dynamic position bias of each branch evaluated to
    its table, every BatchNorm folded into the conv in front of it, both in fp32) and config = dict(embed_dim, depths, num_heads, split,
    ffn_hidden, scale), all read off the shapes: the split from attns.0.rpe_biases (or relative_position_index), the scale from the
    upsample.* convs.  The buffers rpe_biases / relative_position_index / attn_mask_* hold nothing the engine reads.  Host only.  Raises
    ValueError, naming the reason, on what the engine's kernels are not built for."""
    sd = _unwrap_state_dict(sd)
    if any(k not in sd for k in DAT_MARKS) or "conv_first.weight" not in sd:
        raise ValueError(f"not a DAT checkpoint: no {' / '.join(k for k in DAT_MARKS + ('conv_first.weight',) if k not in sd)}")
    if "layers.0.conv.0.weight" in sd or "conv_after_body.0.weight" in sd:
        raise ValueError("DAT resi_connection '3conv' (layers.0.conv.0): the engine runs the 1conv models")
    if "upsample.0.weight" not in sd:
        raise ValueError("DAT checkpoint lacks upsample.0.weight")
    if "conv_before_upsample.0.weight" not in sd:
        raise ValueError("DAT upsampler 'pixelshuffledirect' (DAT-light: no conv_before_upsample): the engine runs the pixelshuffle models")
    c, in_ch = int(sd["conv_first.weight"].shape[0]), int(sd["conv_first.weight"].shape[1])
    if in_ch != 3 or tuple(sd["conv_first.weight"].shape[2:]) != (3, 3):
        raise ValueError(f"DAT conv_first takes {in_ch} input channels: expected 3")
    layers = sorted({int(m.group(1)) for k in sd for m in [re.match(r"layers\.(\d+)\.blocks\.0\.attn\.qkv\.weight$", k)] if m})
    if not layers or layers != list(range(len(layers))) or len(layers) > 16:
        raise ValueError(f"DAT layers are not 0..n-1 with 1 <= n <= 16: {layers}")
    depths = []
    for i in layers:
        blocks = sorted({int(m.group(1)) for k in sd for m in [re.match(rf"layers\.{i}\.blocks\.(\d+)\.attn\.qkv\.weight$", k)] if m})
        if blocks != list(range(len(blocks))):
            raise ValueError(f"DAT layers.{i}: blocks are not 0..n-1: {blocks}")
        depths.append(len(blocks))
    b0 = "layers.0.blocks.0."
    temps = [v for k, v in sd.items() if k.endswith("attn.temperature")]
    if temps:
        heads = int(temps[0].shape[0])
    elif b0 + "attn.attns.0.pos.pos3.2.weight" in sd:
        heads = 2 * int(sd[b0 + "attn.attns.0.pos.pos3.2.weight"].shape[0])
    else:
        raise ValueError(f"DAT checkpoint lacks {b0}attn.attns.0.pos.pos3.2.weight")
    if heads % 2:
        raise ValueError(f"DAT num_heads = {heads} is odd: half of the heads go to each window branch")
    if heads < 2 or c % heads or c // heads > 32:
        raise ValueError(f"DAT head_dim = {c}/{heads} = {c / max(heads, 1):g}: the engine's attention kernels are built for head_dim <= 32")
    if 32 * heads > 512 or c < 16:
        raise ValueError(f"DAT embed_dim {c} with {heads} heads: the engine runs 16 <= embed_dim and at most 16 heads")
    rpe, rpi = sd.get(b0 + "attn.attns.0.rpe_biases"), sd.get(b0 + "attn.attns.0.relative_position_index")
    if rpe is not None:
        split = DAT_SPLITS.get(int(rpe.shape[0]))
        found = f"{int(rpe.shape[0])} rows of rpe_biases"
    elif rpi is not None:
        split = {128: (8, 16), 256: (8, 32)}.get(int(rpi.shape[0]))
        found = f"{int(rpi.shape[0])} tokens per window"
    else:
        raise ValueError(f"DAT checkpoint lacks {b0}attn.attns.0.rpe_biases")
    if split is None:
        raise ValueError(f"DAT split_size with {found}: the engine's window kernel is built for (8, 16) and (8, 32)")
    if b0 + "ffn.fc1.weight" not in sd:
        raise ValueError(f"DAT checkpoint lacks {b0}ffn.fc1.weight")
    hidden = int(sd[b0 + "ffn.fc1.weight"].shape[0])
    if hidden % 2:
        raise ValueError(f"DAT ffn hidden width {hidden} is odd: the feed-forward gate splits it in two")
    if int(sd["conv_before_upsample.0.weight"].shape[0]) != 64:
        raise ValueError(f"DAT num_feat = {int(sd['conv_before_upsample.0.weight'].shape[0])}: the engine's tail kernels are built for 64")
    n0 = int(sd["upsample.0.weight"].shape[0])
    scale = {(256, False): 2, (576, False): 3, (256, True): 4}.get((n0, "upsample.2.weight" in sd))
    if scale is None or any(f"upsample.{k}.weight" in sd for k in (4, 6)):
        raise ValueError(f"DAT pixelshuffle with upsample.0 writing {n0} channels"
                         f"{' and further steps' if 'upsample.2.weight' in sd else ''}: the engine runs scales 2, 3 and 4")
    half, c8, c16, hh = hidden // 2, c // 8, c // 16, heads // 2
    pos_dim = (c // 2 // 4) // 4
    parts = []

    def wb(name, shape):
        parts.extend(_swin_wb(sd, "DAT", name, shape))

    def tensor(name, shape=None):
        if name not in sd:
            raise ValueError(f"DAT checkpoint lacks {name}")
        return _swin_tensor(sd, "DAT", name, shape).reshape(shape if shape is not None else tuple(sd[name].shape))

    def folded(conv, bn, shape):
        """conv (weight of this shape, bias) with the BatchNorm `bn` folded in."""
        o = shape[0]
        w, b = dat_bn_fold(tensor(conv + ".weight", shape), tensor(conv + ".bias", (o,)), tensor(bn + ".weight", (o,)),
                           tensor(bn + ".bias", (o,)), tensor(bn + ".running_mean", (o,)), tensor(bn + ".running_var", (o,)))
        parts.extend([w.ravel(), b])

    def bias_table(stem, hsp, wsp):
        shapes = {"pos_proj.weight": (pos_dim, 2), "pos_proj.bias": (pos_dim,)}
        for k, out in (("pos1", pos_dim), ("pos2", pos_dim), ("pos3", hh)):
            shapes.update({k + ".0.weight": (pos_dim,), k + ".0.bias": (pos_dim,), k + ".2.weight": (out, pos_dim), k + ".2.bias": (out,)})
        parts.append(dat_position_bias({k: tensor(stem + k, s) for k, s in shapes.items()}, hsp, wsp).ravel())

    wb("conv_first", (c, 3, 3, 3))
    wb("before_RG.1", (c,))
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.blocks.{j}."
            wb(b + "norm1", (c,))
            wb(b + "attn.qkv", (3 * c, c))
            if j % 2 == 0:
                bias_table(b + "attn.attns.0.pos.", split[0], split[1])
                bias_table(b + "attn.attns.1.pos.", split[1], split[0])
            else:
                parts.append(tensor(b + "attn.temperature", (heads, 1, 1)).ravel())
            folded(b + "attn.dwconv.0", b + "attn.dwconv.1", (c, 1, 3, 3))
            folded(b + "attn.channel_interaction.1", b + "attn.channel_interaction.2", (c8, c, 1, 1))
            wb(b + "attn.channel_interaction.4", (c, c8, 1, 1))
            folded(b + "attn.spatial_interaction.0", b + "attn.spatial_interaction.1", (c16, c, 1, 1))
            wb(b + "attn.spatial_interaction.3", (1, c16, 1, 1))
            wb(b + "attn.proj", (c, c))
            wb(b + "norm2", (c,))
            wb(b + "ffn.fc1", (hidden, c))
            wb(b + "ffn.sg.norm", (half,))
            wb(b + "ffn.sg.conv", (half, 1, 3, 3))
            wb(b + "ffn.fc2", (c, half))
        wb(f"layers.{i}.conv", (c, c, 3, 3))
    wb("norm", (c,))
    wb("conv_after_body", (c, c, 3, 3))
    wb("conv_before_upsample.0", (64, c, 3, 3))
    wb("upsample.0", (n0, 64, 3, 3))
    if scale == 4:
        wb("upsample.2", (256, 64, 3, 3))
    wb("conv_last", (3, 64, 3, 3))
    config = dict(embed_dim=c, depths=tuple(depths), num_heads=heads, split=split, ffn_hidden=hidden, scale=scale)
    return np.ascontiguousarray(np.concatenate(parts)), config


HAT_MARK = "layers.0.residual_group.overlap_attn.qkv.weight"
HAT_CONV_SCALE = 0.01                                        # HAT's constructor default; no checkpoint holds it


def hat_sa_index():
    """[256, 256] int64: Swin's relative_position_index of a 16 x 16 window, (ya - yb + 15) * 31 + (xa - xb + 15)."""
    y, x = np.divmod(np.arange(256), 16)
    return (y[:, None] - y[None, :] + 15) * 31 + (x[:, None] - x[None, :] + 15)


def _hat_oca_offsets():
    """[256, 576] int64: (dy + 15) * 39 + (dx + 15) for query a = (ya, xa) of the 16 x 16 window, key b = (yb, xb) of the 24 x 24 window,
    (dy, dx) = (yb - ya, xb - xa)."""
    ya, xa = np.divmod(np.arange(256), 16)
    yb, xb = np.divmod(np.arange(576), 24)
    return (yb[None, :] - ya[:, None] + 15) * 39 + (xb[None, :] - xa[:, None] + 15)


def hat_oca_rows(index=None):
    """[1521] int64, entry (dy + 15) * 39 + (dx + 15): the row of the overlapping cross-attention block's relative_position_bias_table that
    key offset (dy, dx) reads, in 0..1520.  From the checkpoint's relative_position_index_OCA [256][576] where there is one (a negative
    row counts from the end of the table, as torch indexing has it; ValueError when two pairs with one offset name different rows, or a
    row lies outside the table); index None: the architecture's formula (dy - 7) * 39 + (dx - 7), whose negative rows wrap."""
    off = _hat_oca_offsets()
    if index is None:
        dy, dx = np.divmod(np.arange(1521), 39)
        return ((dy - 22) * 39 + (dx - 22)) % 1521
    index = np.asarray(index).astype(np.int64)
    if index.shape != (256, 576):
        raise ValueError(f"HAT relative_position_index_OCA {tuple(index.shape)}: expected (256, 576) (window_size 16, overlap_ratio 0.5)")
    if int(index.min()) < -1521 or int(index.max()) >= 1521:
        raise ValueError("HAT relative_position_index_OCA names rows outside the 1521-row table")
    rows = np.empty(1521, dtype=np.int64)
    rows[off.ravel()] = index.ravel()
    if not np.array_equal(rows[off], index):
        raise ValueError("HAT relative_position_index_OCA is not a function of the key offset (dy, dx): the engine's kernel reads the bias by offset")
    return rows % 1521


def parse_hat_state_dict(sd, conv_scale=HAT_CONV_SCALE):
    """Checkpoint state dict of a HAT network (hat_arch.py with upsampler 'pixelshuffle', resi_connection '1conv', window_size 16,
    overlap_ratio 0.5: HAT, HAT-L, HAT-S and their Real-HAT GAN trainings) -> (blob, config): the engine's weight blob (fp32, in the order
    include/sdmi.h documents at sdmi_hat_config, every tensor in the checkpoint's channel order; the overlapping cross-attention block's
    bias table reordered by key offset, [39][39][heads]: the checkpoint's relative_position_index_OCA says which row an offset reads, the
    architecture's formula where a checkpoint holds no such buffer) and config = dict(embed_dim, depths, num_heads, mlp_hidden, cab_mid,
    cab_squeeze, conv_scale, scale), read off the shapes; conv_scale is a constructor argument no checkpoint holds (0.01).  Host only.
    Raises ValueError on what the engine's kernels are not built for: another window size or overlap ratio, head dim > 32, 3conv or
    identity groups, pixelshuffledirect or no upsampler, num_feat other than 64, in_chans other than 3, an OCA index that is not a function
    of the offset, an SA index other than Swin's, and on missing or misshapen tensors."""
    sd = _unwrap_state_dict(sd)
    if HAT_MARK not in sd or "conv_first.weight" not in sd:
        raise ValueError(f"not a HAT checkpoint: no {HAT_MARK if HAT_MARK not in sd else 'conv_first.weight'}")
    if "absolute_pos_embed" in sd:
        raise ValueError("HAT with ape (absolute_pos_embed): the engine runs the models without it")
    if "layers.0.conv.0.weight" in sd:
        raise ValueError("HAT resi_connection '3conv' (layers.0.conv.0): the engine runs the 1conv models")
    if "layers.0.conv.weight" not in sd:
        raise ValueError("HAT resi_connection 'identity' (no layers.0.conv): the engine runs the 1conv models")
    if "upsample.0.weight" not in sd:
        raise ValueError("HAT without an upsampler (no upsample.0): the engine runs the pixelshuffle models")
    if "conv_before_upsample.0.weight" not in sd:
        raise ValueError("HAT upsampler 'pixelshuffledirect' (no conv_before_upsample): the engine runs the pixelshuffle models")
    c, in_ch = int(sd["conv_first.weight"].shape[0]), int(sd["conv_first.weight"].shape[1])
    if in_ch != 3 or tuple(sd["conv_first.weight"].shape[2:]) != (3, 3):
        raise ValueError(f"HAT conv_first takes {in_ch} input channels: expected 3")
    depths = _swin_depths(sd, "HAT")
    b0, o0 = "layers.0.residual_group.blocks.0.", "layers.0.residual_group.overlap_attn."
    table = sd.get(b0 + "attn.relative_position_bias_table")
    if table is None or len(table.shape) != 2:
        raise ValueError(f"HAT checkpoint lacks {b0}attn.relative_position_bias_table")
    heads = int(table.shape[1])
    if int(table.shape[0]) != 961:
        w = (int(round(int(table.shape[0]) ** 0.5)) + 1) // 2
        raise ValueError(f"HAT window_size {w} (a {int(table.shape[0])}-row bias table): the engine's attention kernel is built for 16 (961 rows)")
    otable = sd.get(o0 + "relative_position_bias_table")
    if otable is None or len(otable.shape) != 2:
        raise ValueError(f"HAT checkpoint lacks {o0}relative_position_bias_table")
    if int(otable.shape[0]) != 1521:
        ext = int(round(int(otable.shape[0]) ** 0.5)) + 1 - 16
        raise ValueError(f"HAT overlap_ratio {(ext - 16) / 16:g} (a {int(otable.shape[0])}-row overlap bias table, {ext} x {ext} keys): the engine's "
                         f"attention kernel is built for 0.5 (1521 rows, 24 x 24 keys)")
    if c % heads or c // heads > 32:
        raise ValueError(f"HAT head_dim = {c}/{heads} = {c / heads:g}: the engine's attention kernel is built for head_dim <= 32")
    for name in (b0 + "mlp.fc1.weight", b0 + "conv_block.cab.0.weight", b0 + "conv_block.cab.3.attention.1.weight"):
        if name not in sd:
            raise ValueError(f"HAT checkpoint lacks {name}")
    hidden, mid, squeeze = (int(sd[b0 + n].shape[0]) for n in ("mlp.fc1.weight", "conv_block.cab.0.weight", "conv_block.cab.3.attention.1.weight"))
    if mid > 64 or squeeze > 128:
        raise ValueError(f"HAT conv branch of {mid} mid and {squeeze} squeezed channels: the engine packs at most 64 and 128")
    if int(sd["conv_before_upsample.0.weight"].shape[0]) != 64:
        raise ValueError(f"HAT num_feat = {int(sd['conv_before_upsample.0.weight'].shape[0])}: the engine's tail kernels are built for 64")
    if "conv_last.weight" in sd and int(sd["conv_last.weight"].shape[0]) != 3:
        raise ValueError(f"HAT conv_last writes {int(sd['conv_last.weight'].shape[0])} channels: expected 3")
    n0 = int(sd["upsample.0.weight"].shape[0])
    scale = {(256, False): 2, (576, False): 3, (256, True): 4}.get((n0, "upsample.2.weight" in sd))
    if scale is None or any(f"upsample.{k}.weight" in sd for k in (4, 6)):
        raise ValueError(f"HAT pixelshuffle with upsample.0 writing {n0} channels"
                         f"{' and further steps' if 'upsample.2.weight' in sd else ''}: the engine runs scales 2, 3 and 4")
    sa = sd.get("relative_position_index_SA")
    if sa is not None and (tuple(sa.shape) != (256, 256) or not np.array_equal(np.asarray(sa).astype(np.int64), hat_sa_index())):
        raise ValueError("HAT relative_position_index_SA is not the standard index of a 16 x 16 window, (ya - yb + 15) * 31 + (xa - xb + 15)")
    oca = sd.get("relative_position_index_OCA")
    rows = hat_oca_rows(None if oca is None else np.asarray(oca))
    parts = []

    def wb(name, shape):
        parts.extend(_swin_wb(sd, "HAT", name, shape))

    def mlp(stem):
        wb(stem + "norm2", (c,))
        wb(stem + "mlp.fc1", (hidden, c))
        wb(stem + "mlp.fc2", (c, hidden))

    wb("conv_first", (c, 3, 3, 3))
    wb("patch_embed.norm", (c,))
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            wb(b + "norm1", (c,))
            parts.append(_swin_tensor(sd, "HAT", b + "attn.relative_position_bias_table", (961, heads)))
            wb(b + "attn.qkv", (3 * c, c))
            wb(b + "attn.proj", (c, c))
            wb(b + "conv_block.cab.0", (mid, c, 3, 3))
            wb(b + "conv_block.cab.2", (c, mid, 3, 3))
            wb(b + "conv_block.cab.3.attention.1", (squeeze, c, 1, 1))
            wb(b + "conv_block.cab.3.attention.3", (c, squeeze, 1, 1))
            mlp(b)
        o = f"layers.{i}.residual_group.overlap_attn."
        wb(o + "norm1", (c,))
        wb(o + "qkv", (3 * c, c))
        parts.append(np.ascontiguousarray(_swin_tensor(sd, "HAT", o + "relative_position_bias_table", (1521, heads)).reshape(1521, heads)[rows]).ravel())
        wb(o + "proj", (c, c))
        mlp(o)
        wb(f"layers.{i}.conv", (c, c, 3, 3))
    wb("norm", (c,))
    wb("conv_after_body", (c, c, 3, 3))
    wb("conv_before_upsample.0", (64, c, 3, 3))
    wb("upsample.0", (n0, 64, 3, 3))
    if scale == 4:
        wb("upsample.2", (256, 64, 3, 3))
    wb("conv_last", (3, 64, 3, 3))
    config = dict(embed_dim=c, depths=tuple(depths), num_heads=heads, mlp_hidden=hidden, cab_mid=mid, cab_squeeze=squeeze,
                  conv_scale=float(conv_scale), scale=scale)
    return np.ascontiguousarray(np.concatenate(parts)), config


def upscaler_family(sd):
    """"hat" | "dat" | "scunet" | "swin2sr" | "swinir" | "rrdb" | "compact" by the key layout: the first group's overlap_attn.qkv.weight marks a
    HAT network (no other family has it; a HAT has the SwinIR mark too, so this test comes before those); before_RG.1.weight together with
    the first block's attns.0.pos.pos_proj.weight marks a DAT network (no other family has either key); m_head.0.weight together with the first block's
    relative_position_params marks a ScuNET; the first block's attn.logit_scale marks a Swin2SR network (it has an attn.qkv.weight
    too, so this test comes before the next); the first block's attn.qkv.weight marks a SwinIR network (it has a conv_first.weight
    too, so this test comes before the next); conv_first.weight / model.0.weight mark an RRDBNet, a 4-d body.0.weight without them a
    compact network.  Anything else counts as "rrdb" and gets that loader's refusal."""
    keys = _unwrap_state_dict(sd)
    if HAT_MARK in keys:
        return "hat"
    if all(k in keys for k in DAT_MARKS):
        return "dat"
    if all(k in keys for k in SCUNET_MARKS):
        return "scunet"
    if SWIN2SR_MARK in keys:
        return "swin2sr"
    if SWINIR_MARK in keys:
        return "swinir"
    if "conv_first.weight" not in keys and "model.0.weight" not in keys and len(getattr(keys.get("body.0.weight"), "shape", ())) == 4:
        return "compact"
    return "rrdb"


def parse_upscaler_state_dict(sd):
    """The dispatcher over the checkpoints the engine runs -> ("rrdb", parse_esrgan_state_dict(sd)), ("compact",
    parse_compact_state_dict(sd)), ("swinir", (blob, config, scale)), ("swin2sr", (blob, config, scale)), ("scunet", (blob, config, 1)) or
    ("dat", (blob, config, scale)) or ("hat", (blob, config, scale)); the scale is the last member of each tuple."""
    family = upscaler_family(sd)
    if family in ("swinir", "swin2sr", "scunet", "dat", "hat"):
        blob, config = {"swinir": parse_swinir_state_dict, "swin2sr": parse_swin2sr_state_dict, "scunet": parse_scunet_state_dict,
                        "dat": parse_dat_state_dict, "hat": parse_hat_state_dict}[family](sd)
        return family, (blob, config, config["scale"])
    return family, (parse_compact_state_dict if family == "compact" else parse_esrgan_state_dict)(sd)


def load_esrgan_checkpoint(path):
    """.pth (torch.load, weights_only) or .safetensors -> state dict."""
    if str(path).lower().endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    import torch
    return torch.load(path, map_location="cpu", weights_only=True)


def model_output_to_u8(y):
    """The reference's hand-off from the model's [0, 1] output to uint8 (modules/upscaler_utils.py): clamp, x255, np.round (half to
    even) — NOT the truncation of ops.image_to_u8.  y: float array."""
    return np.round(np.clip(np.asarray(y, dtype=np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def arena_limit_bytes(device=0):
    """What a run's scratch may take: the device memory that is free now."""
    import torch
    return int(torch.cuda.mem_get_info(device)[0])


class EsrganInputTooLarge(ValueError):
    """An image whose intermediates the engine's arena cannot hold (EsrganNet.check_fits)."""


class _EngineNet:
    """One upscaler network resident on an engine: the handle of the C entries <_abi>_create / _destroy / _scratch_bytes / _run and the
    size checks in front of a run.  A family supplies its _abi, how a state dict becomes the arguments of its create entry (_parse),
    and what differs in check_fits."""
    _abi = None
    _noun = None                                             # what check_fits calls the net; None: "the x{scale} upscaler"
    _zero_need_is_a_refusal = False                          # scratch_bytes 0 = the engine refuses the size: a tensor passes 2^31 elements
    unshuffle = 1                                            # H and W of an input must be multiples of this (the caller pads)

    def _fn(self, name):
        from . import _lib
        return getattr(_lib.lib, f"{self._abi}_{name}")

    def _parse(self, state_dict):
        """-> (blob, the arguments of the create entry behind the blob); sets scale and what else the family reads off the checkpoint."""
        raise NotImplementedError

    def _extra_elements(self, b, h, w):
        """A tensor's element count that has to stay below 2^31 and that the arena bytes do not bound."""
        return 0

    def __init__(self, state_dict, device=0, engine=None):
        from . import _lib
        from .engine import Engine
        blob, args = self._parse(state_dict)
        self.device = int(device)
        self.engine = engine or Engine(self.device)
        self.handle = self._fn("create")(self.engine.handle, blob.ctypes.data, blob.size, *args)
        if not self.handle:
            raise _lib.SdmiError(f"{self._abi}_create failed: " + _lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scratch_bytes(self, b, h, w):
        """Arena bytes of one run, from the engine's own layout (<_abi>_scratch_bytes; 0 for a size the engine refuses)."""
        return int(self._fn("scratch_bytes")(self.handle, b, h, w))

    def check_fits(self, b, h, w):
        """Refuse an input whose intermediates the arena cannot hold, or one of whose tensors passes 2^31 elements."""
        need = self.scratch_bytes(b, h, w)
        # the arena the engine already holds is replaced, not added to, when it has to grow: it counts as available
        limit = arena_limit_bytes(self.device) + self.engine.arena_bytes()
        what = f"image {w}x{h} (batch {b}) is too large for {self._noun or f'the x{self.scale} upscaler'}"
        if self._zero_need_is_a_refusal and need <= 0:
            raise EsrganInputTooLarge(f"{what}: a tensor passes 2^31 elements")
        if self._extra_elements(b, h, w) >= (1 << 31) - 256 or need > limit:
            raise EsrganInputTooLarge(f"{what}: its intermediates need {need / 2 ** 30:.1f} GiB of engine arena, "
                                      f"{limit / 2 ** 30:.1f} GiB are available")

    def run(self, x, out_u8=False):
        """x: uint8 [B,H,W,3] (RGB; divided by 255 on the way in) or fp32 [B,3,H,W] in [0, 1], on the engine's device ->
        fp32 [B,3,H s,W s], or with out_u8 uint8 [B,H s,W s,3] (clamp, x255, round half to even).  The sides a family takes are in its
        docstring."""
        import torch
        from . import _lib
        in_u8 = x.dtype == torch.uint8
        x = x.contiguous() if in_u8 else x.float().contiguous()
        b, h, w = (x.shape[0], x.shape[1], x.shape[2]) if in_u8 else (x.shape[0], x.shape[2], x.shape[3])
        assert x.shape[3 if in_u8 else 1] == 3
        self.check_fits(b, h, w)
        s = self.scale
        out = (torch.empty((b, h * s, w * s, 3), dtype=torch.uint8, device=x.device) if out_u8
               else torch.empty((b, 3, h * s, w * s), dtype=torch.float32, device=x.device))
        _lib.check(self._fn("run")(self.handle, _lib.ptr(x), 1 if in_u8 else 0, b, h, w, _lib.ptr(out), 1 if out_u8 else 0, _lib.stream_ptr()),
                   self._abi + "_run")
        return out


class EsrganNet(_EngineNet):
    """One RRDBNet resident on an engine (sdmi_esrgan_*).  H, W: multiples of 4 / scale (the x2 / x1 models pixel-unshuffle).  The arena
    holds the 192-wide dense buffers and the (H s) x (W s) x 64 up-conv tensors."""
    _abi = "sdmi_esrgan"
    unshuffle = property(lambda self: 4 // self.scale)

    def _parse(self, state_dict):
        blob, self.num_block, self.in_ch, self.scale = parse_esrgan_state_dict(state_dict)
        return blob, (self.num_block, self.in_ch, self.scale)

    def _extra_elements(self, b, h, w):
        return b * (h // self.unshuffle) * (w // self.unshuffle) * 16


class CompactNet(_EngineNet):
    """One compact Real-ESRGAN network (SRVGGNetCompact) resident on an engine (sdmi_compact_*).  Any H, W.  The arena holds the padded
    input and two 64-wide buffers, all at the INPUT resolution; the output must stay below 2^31 pixels."""
    _abi = "sdmi_compact"

    def _parse(self, state_dict):
        blob, self.num_conv, self.scale = parse_compact_state_dict(state_dict)
        return blob, (self.num_conv, self.scale)

    def _extra_elements(self, b, h, w):
        return b * h * w * self.scale * self.scale


def _swin_config_c(cfg, config):
    """The fields sdmi_swinir_config and sdmi_swin2sr_config share, off a parser's config dict."""
    import ctypes
    cfg.embed_dim, cfg.num_layers, cfg.num_heads = config["embed_dim"], len(config["depths"]), config["num_heads"]
    cfg.mlp_hidden, cfg.resi_3conv, cfg.scale = config["mlp_hidden"], config["resi_3conv"], config["scale"]
    for i, d in enumerate(config["depths"]):
        cfg.depths[i] = d
    return ctypes.byref(cfg)


class SwinIRNet(_EngineNet):
    """One SwinIR network (nearest+conv upsampler) resident on an engine (sdmi_swinir_*).  Any H, W >= 8: the reflect padding to
    multiples of the window and the crop happen on the device.  The arena holds the token tensors of the padded grid, the qkv and MLP
    rows and the (H s) x (W s) x 64 tail."""
    _abi = "sdmi_swinir"
    _zero_need_is_a_refusal = True

    def _parse(self, state_dict):
        from . import _lib
        blob, self.config = parse_swinir_state_dict(state_dict)
        self.scale = self.config["scale"]
        return blob, (_swin_config_c(_lib.SwinIRConfigC(), self.config),)

    def check_fits(self, b, h, w):
        if min(h, w) < 8:
            raise ValueError(f"image {w}x{h}: SwinIR needs sides of at least 8 (one window)")
        super().check_fits(b, h, w)


class Swin2SRNet(SwinIRNet):
    """One Swin2SR network (nearest+conv, pixelshuffle or pixelshuffledirect upsampler) resident on an engine (sdmi_swin2sr_*): the
    twin of SwinIRNet, whose size checks it shares."""
    _abi = "sdmi_swin2sr"

    def _parse(self, state_dict):
        from . import _lib
        blob, self.config = parse_swin2sr_state_dict(state_dict)
        self.scale = self.config["scale"]
        cfg = _lib.Swin2SRConfigC()
        cfg.upsampler = SWIN2SR_UPSAMPLERS.index(self.config["upsampler"])
        return blob, (_swin_config_c(cfg, self.config),)


class ScuNETNet(_EngineNet):
    """One SCUNet (dim 64) resident on an engine (sdmi_scunet_*), scale 1.  Any H, W >= 1: the replicate padding to multiples of 64 and
    the crop happen on the device.  The arena holds the skip tensors and the level-1 work buffers of the padded grid."""
    _abi = "sdmi_scunet"
    _noun = "ScuNET"
    _zero_need_is_a_refusal = True

    def _parse(self, state_dict):
        import ctypes
        from . import _lib
        blob, self.config = parse_scunet_state_dict(state_dict)
        self.scale = 1
        cfg = _lib.ScuNETConfigC()
        for i, d in enumerate(self.config["depths"]):
            cfg.depths[i] = d
        return blob, (ctypes.byref(cfg),)


class DATNet(_EngineNet):
    """One DAT network (pixelshuffle upsampler, 1conv groups) resident on an engine (sdmi_dat_*).  Any H, W >= 1: the network has no
    padding of its own, the attention windows pad by index on the device.  The arena holds the token tensors, the slot-layout q | k | v,
    attention, conv and mix rows, the feed-forward rows and the (H s) x (W s) x 64 tail."""
    _abi = "sdmi_dat"
    _noun = "DAT"
    _zero_need_is_a_refusal = True

    def _parse(self, state_dict):
        import ctypes
        from . import _lib
        blob, self.config = parse_dat_state_dict(state_dict)
        self.scale = self.config["scale"]
        cfg = _lib.DATConfigC()
        cfg.embed_dim, cfg.num_layers, cfg.num_heads = self.config["embed_dim"], len(self.config["depths"]), self.config["num_heads"]
        cfg.split0, cfg.split1 = self.config["split"]
        cfg.ffn_hidden, cfg.scale = self.config["ffn_hidden"], self.scale
        for i, d in enumerate(self.config["depths"]):
            cfg.depths[i] = d
        return blob, (ctypes.byref(cfg),)


class HATNet(_EngineNet):
    """One HAT network (pixelshuffle upsampler, 1conv groups, window 16, overlap ratio 0.5) resident on an engine (sdmi_hat_*).  Any H,
    W >= 9: the reflect padding to multiples of 16 and the crop happen on the device.  The arena holds the token tensors of the padded
    grid, the slot-layout q | k | v and attention rows, the MLP rows, the conv branch's two tensors and the (H s) x (W s) x 64 tail."""
    _abi = "sdmi_hat"
    _noun = "HAT"
    _zero_need_is_a_refusal = True

    def _parse(self, state_dict):
        import ctypes
        from . import _lib
        blob, self.config = parse_hat_state_dict(state_dict)
        self.scale = self.config["scale"]
        cfg = _lib.HATConfigC()
        cfg.embed_dim, cfg.num_layers, cfg.num_heads = self.config["embed_dim"], len(self.config["depths"]), self.config["num_heads"]
        cfg.mlp_hidden, cfg.cab_mid, cfg.cab_squeeze = self.config["mlp_hidden"], self.config["cab_mid"], self.config["cab_squeeze"]
        cfg.conv_scale, cfg.scale = self.config["conv_scale"], self.scale
        for i, d in enumerate(self.config["depths"]):
            cfg.depths[i] = d
        return blob, (ctypes.byref(cfg),)

    def check_fits(self, b, h, w):
        if min(h, w) < 9:
            raise ValueError(f"image {w}x{h}: HAT needs sides of at least 9 (the reflect padding to a window of 16)")
        super().check_fits(b, h, w)


def make_upscaler_net(state_dict, device=0, engine=None):
    """EsrganNet, CompactNet, SwinIRNet, Swin2SRNet, ScuNETNet, DATNet or HATNet, by the checkpoint's key layout (upscaler_family)."""
    cls = {"compact": CompactNet, "swinir": SwinIRNet, "swin2sr": Swin2SRNet, "scunet": ScuNETNet, "dat": DATNet,
           "hat": HATNet}.get(upscaler_family(state_dict), EsrganNet)
    return cls(state_dict, device=device, engine=engine)


class UpscalerESRGAN(Upscaler):
    """ESRGAN / Real-ESRGAN on the engine: what modules/esrgan_model.py:UpscalerESRGAN.do_upscale and
    modules/realesrgan_model.py:UpscalerRealESRGAN.do_upscale compute with ESRGAN_tile = 0 (the image whole; tiling exists there for
    VRAM this card does not lack), with the uint8 hand-off of modules/upscaler_utils.py.  RRDBNet checkpoints run as EsrganNet, the
    compact Real-ESRGAN models (General 4xV3, General WDN 4xV3, AnimeVideo) as CompactNet.  SwinIR checkpoints (nearest+conv upsampler)
    run as SwinIRNet: what extensions-builtin/SwinIR's UpscalerSwinIR.do_upscale computes with the image in one tile (SWIN_tile exists
    for the same VRAM reason as ESRGAN_tile), the padding to the window size done on the device; Swin2SR checkpoints (what the extension
    builds from swinir_model_arch_v2.py) run as Swin2SRNet the same way.  ScuNET checkpoints run as ScuNETNet:
    extensions-builtin/ScuNET's UpscalerScuNET.do_upscale with the image in one tile; the result has the input's size and the driver
    loop of Upscaler.upscale fits it with Lanczos.  DAT checkpoints (pixelshuffle, 1conv) run as DATNet: modules/dat_model.py's
    UpscalerDAT.do_upscale with the image in one tile (DAT_tile exists for the same VRAM reason).  HAT checkpoints (pixelshuffle, 1conv,
    window 16) run as HATNet: modules/hat_model.py's UpscalerHAT.do_upscale with the image in one tile (HAT_tile likewise)."""
    name = "ESRGAN"

    def __init__(self, device=0, engine=None):
        """engine: the engine.Engine whose arena the runs use — e.g. the one that holds the UNet and VAE (SdModel.engine); without one
        the scaler makes a single engine of its own on first use.  Every checkpoint of this scaler shares it: one arena, however many
        models are registered."""
        super().__init__()
        self.device = int(device)
        self.engine = engine
        self._nets = {}

    def load_model(self, path):
        net = self._nets.get(path)
        if net is None:
            if self.engine is None:
                from .engine import Engine
                self.engine = Engine(self.device)
            net = self._nets[path] = make_upscaler_net(load_esrgan_checkpoint(path), device=self.device, engine=self.engine)
        return net

    def do_upscale(self, img, selected_model=None):
        import torch
        net = self.load_model(selected_model)
        rgb = np.array(img.convert("RGB"))
        h, w = rgb.shape[:2]
        f = net.unshuffle                                    # the x2 / x1 RRDBNets pixel-unshuffle: sides padded up to a multiple, cropped after
        ph, pw = -h % f, -w % f
        if ph or pw:
            rgb = np.pad(rgb, ((0, ph), (0, pw), (0, 0)), mode="reflect" if min(h, w) > max(ph, pw) else "edge")
        x = torch.from_numpy(np.ascontiguousarray(rgb)[None]).to(f"cuda:{self.device}")
        out = net.run(x, out_u8=True)[0].cpu().numpy()
        return Image.fromarray(out[:h * net.scale, :w * net.scale])


def register_esrgan(paths, device=0, engine=None):
    """Append one ``UpscalerData(name, path, scaler, scale)`` per checkpoint to shared.sd_upscalers (after the built-ins, which are
    installed first if the list is empty): `paths` is a {name: path} mapping or a list of paths (name = the file's stem), so
    hr_upscaler="R-ESRGAN 4x+" and opts.upscaler_for_img2img resolve through _resize_to.  RRDBNet, compact (SRVGGNetCompact), SwinIR,
    Swin2SR, ScuNET, DAT and HAT checkpoints may be mixed; the scale is read from the checkpoint.
    engine: see UpscalerESRGAN (all entries of one call share one scaler object and so one engine)."""
    if not shared.sd_upscalers:
        shared.sd_upscalers = builtin_upscalers()
    items = paths.items() if isinstance(paths, dict) else [(os.path.splitext(os.path.basename(p))[0], p) for p in paths]
    scaler = UpscalerESRGAN(device, engine)
    added = []
    for name, path in items:
        scale = parse_upscaler_state_dict(load_esrgan_checkpoint(path))[1][-1]
        data = UpscalerData(name, path, scaler, scale)
        scaler.scalers.append(data)
        shared.sd_upscalers.append(data)
        added.append(data)
    return added


def _resize_to(im, w, h, upscaler_name):
    """The inner `resize` of modules/images.py:269-288: Lanczos for masks / no upscaler, else the named upscaler for enlargements."""
    if upscaler_name is None or upscaler_name == "None" or im.mode == 'L':
        return im.resize((w, h), resample=LANCZOS)
    if max(w / im.width, h / im.height) > 1.0:
        named = [x for x in shared.sd_upscalers if x.name == upscaler_name]
        chosen = named[0] if named else shared.sd_upscalers[0]
        im = chosen.scaler.upscale(im, max(w / im.width, h / im.height), chosen.data_path)
    return im if (im.width, im.height) == (w, h) else im.resize((w, h), resample=LANCZOS)


def resize_image(resize_mode, im, width, height, upscaler_name=None):
    """modules/images.py:252-326.  0: stretch to width x height (the hires fix); 1: cover the target keeping the aspect ratio, centred,
    the excess cropped; 2: fit inside the target keeping the aspect ratio, centred, the empty bands filled by stretching the image's
    own border row / column over them."""
    from PIL import Image
    upscaler_name = upscaler_name or getattr(shared.opts, "upscaler_for_img2img", None)
    if resize_mode == 0:
        return _resize_to(im, width, height, upscaler_name)
    ratio, src_ratio = width / height, im.width / im.height
    by_w, by_h = im.width * height // im.height, im.height * width // im.width      # the other side when one side is matched exactly
    if resize_mode == 1:                                     # cover: match the side on which the scaled source would fall short
        src_w, src_h = (width, by_h) if ratio > src_ratio else (by_w, height)
    else:                                                    # fit: match the side on which the scaled source would overflow
        src_w, src_h = (width, by_h) if ratio < src_ratio else (by_w, height)
    resized = _resize_to(im, src_w, src_h, upscaler_name)
    canvas = Image.new("RGB", (width, height))
    x0, y0 = width // 2 - src_w // 2, height // 2 - src_h // 2
    canvas.paste(resized, box=(x0, y0))
    if resize_mode == 2:
        if ratio < src_ratio and y0 > 0:                     # bands above / below: the first / last row stretched over them
            canvas.paste(resized.resize((width, y0), box=(0, 0, width, 0)), box=(0, 0))
            canvas.paste(resized.resize((width, y0), box=(0, resized.height, width, resized.height)), box=(0, y0 + src_h))
        elif ratio > src_ratio and x0 > 0:                   # bands left / right: the first / last column
            canvas.paste(resized.resize((x0, height), box=(0, 0, 0, height)), box=(0, 0))
            canvas.paste(resized.resize((x0, height), box=(resized.width, 0, resized.width, height)), box=(x0 + src_w, 0))
    return canvas
