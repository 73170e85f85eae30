"""Emulation of the reference's *own* default GPU numerics on the CPU oracle (test infrastructure).

The webui's default GPU configuration is ``model.half()`` under ``torch.autocast("cuda")`` (SURVEY.md section 3.5;
/root/reference/modules/sd_models.py:482-491, modules/devices.py:210-231): every conv / linear / einsum accumulates in fp32 and
*stores an fp16 result*; GroupNorm32 computes in fp32 and casts back to fp16 (modules/devices.py:284-295 +
``.type(x.dtype)``); residual adds, SiLU, GELU and the GEGLU product run on fp16 tensors; the split-attention forward keeps the
score matrix and the softmax output in ``q.dtype`` (modules/sd_hijack_optimizations.py:262-268: ``s2 = s1.softmax(dim=-1,
dtype=q.dtype)``).  ``fp16_storage(net)`` reproduces exactly that rounding pattern on the fp32 oracle modules: arithmetic stays
fp32 (= fp32 accumulation), every tensor a GPU kernel would *write* is rounded to binary16.  Loaded hypernetworks
(``oracle.unet.LOADED_HYPERNETWORKS``) are modules inside the same autocast region, applied to the fp16 attention context
(modules/hypernetworks/hypernetwork.py:358-379), and round the same way.

The VAE encoder (``oracle.vae.Encoder``) rounds as the decoder does: the GroupNorm output, the SiLU in front of ``conv_out`` and every
convolution's result are stored tensors.

The CLIP text towers (``oracle.clip``) follow the same rule — every tensor a kernel of the half-precision path writes is rounded, the
arithmetic stays fp32 — read off transformers' CLIPTextModel (modeling_clip.py, CLIPAttention / CLIPMLP / CLIPEncoderLayer /
CLIPTextEmbeddings; the reference runs it as ``model.half()``, modules/sd_hijack_clip.py:351-360): ``q_proj(x) * scale`` is a tensor
of its own, the scores come out of one ``bmm`` and get the causal mask added, ``softmax`` and the product with V each write their
result, the activation writes its result behind ``fc1``, both residual sums and the sum of token and position embeddings are tensor
additions.  Linear and LayerNorm outputs are rounded by the leaf hooks.

Used by the C1 parity tests to measure how far the reference's fp16 path itself sits from its fp32 CPU path — the yardstick the
engine's own distance is compared with (profiles/r02_parity.json).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import clip as oc
from oracle import hypernetwork as ohn
from oracle import unet as ou
from oracle import vae as ov


def r16(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def _res_forward(self, x, emb):
    h = self.in_layers(x)                                       # GroupNorm / SiLU / Conv outputs rounded by the leaf hooks
    h = r16(h + self.emb_layers(emb)[:, :, None, None])
    h = self.out_layers(h)
    return r16(self.skip_connection(x) + h)


def _attn_forward(self, x, context=None):
    h = self.heads
    context = x if context is None else context
    context_k = context_v = context
    if ou.LOADED_HYPERNETWORKS:                                 # (their modules round like the network's own: _hn_forward + the leaf hooks)
        context_k, context_v = ohn.apply_hypernetworks(ou.LOADED_HYPERNETWORKS, context)
    q, k, v = self.to_q(x), self.to_k(context_k), self.to_v(context_v)
    b, n, _ = q.shape
    split = lambda t: t.reshape(b, t.shape[1], h, -1).permute(0, 2, 1, 3).reshape(b * h, t.shape[1], -1)
    q, k, v = split(q), split(k), split(v)
    sim = r16(r16(torch.einsum('bid,bjd->bij', q, k)) * self.scale)
    attn = r16(sim.softmax(dim=-1))
    out = r16(torch.einsum('bij,bjd->bid', attn, v))
    out = out.reshape(b, h, n, -1).permute(0, 2, 1, 3).reshape(b, n, -1)
    return self.to_out(out)


def _hn_forward(self, x):
    # the hypernetwork modules run on the fp16 context inside the same autocast region: every Linear stores an fp16 result (leaf hooks),
    # the activations, the product with the multiplier and the sum with x are fp16 tensor arithmetic
    return r16(x + r16(self.linear(x) * self.multiplier))


def _geglu_forward(self, x):
    x, gate = self.proj(x).chunk(2, dim=-1)
    return r16(x * r16(F.gelu(gate)))


def _tblock_forward(self, x, context=None):
    x = r16(self.attn1(self.norm1(x)) + x)
    x = r16(self.attn2(self.norm2(x), context=context) + x)
    x = r16(self.ff(self.norm3(x)) + x)
    return x


def _st_forward(self, x, context=None):
    b, c, h, w = x.shape
    x_in = x
    x = self.norm(x)
    if not self.use_linear:
        x = self.proj_in(x)
    x = x.permute(0, 2, 3, 1).reshape(b, h * w, -1)
    if self.use_linear:
        x = self.proj_in(x)
    for block in self.transformer_blocks:
        x = block(x, context=context)
    if self.use_linear:
        x = self.proj_out(x)
    x = x.view(b, h, w, -1).permute(0, 3, 1, 2)
    if not self.use_linear:
        x = self.proj_out(x)
    return r16(x + x_in)


def _vae_res_forward(self, x):
    h = self.conv1(r16(F.silu(self.norm1(x))))
    h = self.conv2(r16(F.silu(self.norm2(h))))
    if self.cin != self.cout:
        x = self.nin_shortcut(x)
    return r16(x + h)


def _vae_attn_forward(self, x):
    h = self.norm(x)
    q, k, v = self.q(h), self.k(h), self.v(h)
    b, c, hh, ww = q.shape
    q, k, v = [t.reshape(b, c, hh * ww).permute(0, 2, 1) for t in (q, k, v)]
    w = r16(torch.softmax(r16(r16(torch.bmm(q, k.transpose(1, 2))) * (int(c) ** -0.5)), dim=-1))
    o = r16(torch.bmm(w, v)).permute(0, 2, 1).reshape(b, c, hh, ww)
    return r16(x + self.proj_out(o))


def _vae_decoder_forward(self, z):
    h = self.conv_in(z)
    h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
    for i in reversed(range(self.nres)):
        for j in range(self.nrb + 1):
            h = self.up[i].block[j](h)
        if i != 0:
            h = self.up[i].upsample(h)
    return self.conv_out(r16(F.silu(self.norm_out(h))))


def _vae_encoder_forward(self, x):
    h = self.conv_in(x)
    for i in range(self.nres):
        for j in range(self.nrb):
            h = self.down[i].block[j](h)
        if i != self.nres - 1:
            h = self.down[i].downsample(h)
    h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
    return self.conv_out(r16(F.silu(self.norm_out(h))))


def _clip_attn_forward(self, x, mask):
    b, l, c = x.shape
    d = c // self.heads
    q = r16(self.q_proj(x) * d ** -0.5)
    k, v = self.k_proj(x), self.v_proj(x)
    sp = lambda t: t.view(b, l, self.heads, d).transpose(1, 2)
    w = r16(sp(q) @ sp(k).transpose(-1, -2) + mask)
    o = r16(r16(w.softmax(dim=-1)) @ sp(v))
    return self.out_proj(o.transpose(1, 2).reshape(b, l, c))


def _clip_mlp_forward(self, x):
    return self.fc2(r16(self.act(self.fc1(x))))


def _clip_layer_forward(self, x, mask):
    x = r16(x + self.self_attn(self.layer_norm1(x), mask))
    return r16(x + self.mlp(self.layer_norm2(x)))


def _clip_emb_forward(self, tokens, inputs_embeds=None):
    e = self.token_embedding(tokens) if inputs_embeds is None else inputs_embeds
    return r16(e + self.position_embedding.weight[: e.shape[1]])


_PATCHES = [(ou.ResBlock, _res_forward), (ou.CrossAttention, _attn_forward), (ou.GEGLU, _geglu_forward),
            (ou.BasicTransformerBlock, _tblock_forward), (ou.SpatialTransformer, _st_forward),
            (ohn.HypernetworkModule, _hn_forward), (ov.ResnetBlock, _vae_res_forward), (ov.AttnBlock, _vae_attn_forward), (ov.Decoder, _vae_decoder_forward),
            (ov.Encoder, _vae_encoder_forward), (oc.ClipAttention, _clip_attn_forward), (oc.ClipMLP, _clip_mlp_forward),
            (oc.ClipLayer, _clip_layer_forward), (oc.ClipEmbeddings, _clip_emb_forward)]
_LEAVES = (nn.Conv2d, nn.Linear, nn.GroupNorm, nn.LayerNorm, nn.SiLU)


@contextlib.contextmanager
def fp16_storage(net: nn.Module):
    """Inside the block ``net`` (an oracle UNetModel / AutoencoderKL / Decoder / Encoder / ClipTextModel) computes with fp32 arithmetic and fp16-rounded
    stores at every point where the reference's half-precision autocast path materialises a tensor."""
    saved = [(cls, cls.forward) for cls, _ in _PATCHES]
    handles = []
    try:
        for cls, fn in _PATCHES:
            cls.forward = fn
        for m in net.modules():
            if isinstance(m, _LEAVES):
                handles.append(m.register_forward_hook(lambda mod, inp, out: r16(out)))
        for hn in ou.LOADED_HYPERNETWORKS:                      # Linear, activation (any of hypernetwork.ACT), LayerNorm: every leaf stores fp16
            for pair in hn.layers.values():
                for m in (leaf for mod in pair for leaf in mod.modules() if not list(leaf.children())):
                    handles.append(m.register_forward_hook(lambda mod, inp, out: r16(out)))
        yield net
    finally:
        for h in handles:
            h.remove()
        for cls, fn in saved:
            cls.forward = fn


def capture_outputs(net: nn.Module, names) -> tuple:
    """Forward hooks that record the output of the named sub-modules (error budget).  Returns (dict, handles)."""
    got, handles = {}, []
    mods = dict(net.named_modules())
    for n in names:
        if n in mods:
            handles.append(mods[n].register_forward_hook(lambda mod, inp, out, n=n: got.__setitem__(n, out.detach().clone())))
    return got, handles
