"""Teacher-forced per-block parity of the engine's activation taps against the fp32 oracle (test infrastructure).

A free-running comparison of block N carries the error of every block in front of it, so it cannot be held near one block's rounding
floor.  Here the oracle's module N is fed the ENGINE's own output of block N - 1 (engine option "trace" -> Engine.taps()), and its
output is compared with the engine's output of block N: every figure is the error of one segment alone — the launches between two taps.

    forced_outputs(net, call, taps)   one forced oracle pass -> {tap name: the oracle's own output of that segment, NCHW}
    segment_errors(net, call, taps)   the forced pass twice on identical forced inputs, plain fp32 and under the reference's fp16 rounding
                                      pattern (fp16_emu.fp16_storage) -> per tap the engine's error, the yardstick, the worst slices
    assert_segments(rows, label)      the caps; returns the figures of the case for a report
    recorded_outputs(net, call, names) the same recording points on a free-running pass (the CPU self-test's stand-in for the engine)

The yardstick of a segment is `rel_l2(o16, o32)`: how far the reference's own half-precision path lands from fp32 on that segment, from
the same inputs.  It is computed from the oracle alone; nothing the engine produces enters a cap.

A tap is matched either by the oracle module of the same `named_modules()` name (a forward hook records the module's output and returns
the engine's tap in its place, so the next module — and every skip connection that keeps the tensor — goes on with the engine's
activation), or, for `<block>.attn1+x`, `<block>.attn2+x` and `<block>` of a BasicTransformerBlock, by the three `+ x` points of a
forcing-aware block forward.  A tap that nothing matches, or that the pass never reaches, is an error: no tap is left out.

The CLIP text towers (oracle.clip) go the same way: `embeddings` and `final_layer_norm` by module hook, `encoder.layers.<i>.self_attn+x`
and `encoder.layers.<i>` by the two `+ x` points of a forcing-aware ClipLayer forward.  A token tensor [B, L, C] is an NCHW tensor of
height L and width 1, so the two slicings mean per token (b, l, 0) and per channel.  The forced call must not ask for the pooled row:
that path runs `final_layer_norm` a second time, on another tensor.  The VAE encoder's result — the fp32 moments, `quant_conv` folded
into `conv_out` by the engine's host code — is filed as the tap of the AutoencoderKL module `quant_conv` with the call
`n.encode_moments(x)`: its segment is norm_out -> SiLU -> conv_out -> quant_conv from the `encoder.mid.block_2` tap.
"""
from __future__ import annotations

import contextlib

import torch

import fp16_emu
from fp16_emu import fp16_storage, r16
from helpers import rel_l2, worst_slice_rel_l2
from oracle import clip as oc
from oracle import unet as ou

MARGIN = 1.25            # the project's standing margin over a measured floor
SLICE_FACTOR = 2.0       # worst slice within 2 x the cap of the whole tensor (tests/test_gpu_ops.py: assert_slices)
YARD_FLOOR = 1e-4        # the fp16 rounding of one stored output alone is 2.06e-4: a smaller yardstick means the segment compares nothing
SLICINGS = (("pixel (b, y, x)", (0, 2, 3)), ("channel", (1,)))      # of an NCHW tensor
SUB_TAPS = (".attn1+x", ".attn2+x", "")                              # the three `+ x` points of a BasicTransformerBlock, in order
CLIP_SUB_TAPS = (".self_attn+x", "")                                 # the two `+ x` points of a ClipLayer, in order


class UnmatchedTap(AssertionError):
    pass


def as_nchw(t, h):
    """A token tensor [b, hw, C] as NCHW of height `h` (tests/test_gpu_c1_parity.py: _as_nchw)."""
    if t.dim() == 3:
        b, hw, c = t.shape
        return t.reshape(b, h, hw // h, c).permute(0, 3, 1, 2)
    return t


def _like(tap, out):
    """The NCHW tap in the layout of the oracle tensor `out`."""
    if out.dim() == 3:
        b, c, h, w = tap.shape
        return tap.permute(0, 2, 3, 1).reshape(b, h * w, c)
    return tap


class _Forcing:
    """`names`: where to record.  `taps`: what to put in place of the recorded tensor (none: a free-running pass that only records)."""

    def __init__(self, net, names, taps=None):
        self.names = list(names)
        self.taps = {k: v.float() for k, v in (taps or {}).items()}
        self.seen = {}
        self.h = None                                          # height of the feature map the current SpatialTransformer works on
        mods = dict(net.named_modules())
        self.transformers = [m for m in mods.values() if isinstance(m, ou.SpatialTransformer)]
        self.block_names = {id(m): n for n, m in mods.items() if isinstance(m, ou.BasicTransformerBlock)}
        self.block_names.update({id(m): n for n, m in mods.items() if isinstance(m, oc.ClipLayer)})
        points = {n + s for n, m in mods.items() for s in (SUB_TAPS if isinstance(m, ou.BasicTransformerBlock) else CLIP_SUB_TAPS)
                  if id(m) in self.block_names}
        self.hooked = {n: mods[n] for n in self.names if n in mods and n not in points}
        unmatched = sorted(n for n in self.names if n not in self.hooked and n not in points)
        if unmatched:
            raise UnmatchedTap(f"{len(unmatched)} of {len(self.names)} taps match no oracle module or sub-tap point: {unmatched}")
        self.recorded = set(self.names)

    def visit(self, name, out):
        """Record the oracle's `out` at tap `name` (as NCHW) and hand back the engine's tensor, if there is one, in its place."""
        if name not in self.recorded:
            return out
        tap = self.taps.get(name)
        # (height of a token tensor: the tap's; on a free-running pass the feature map's — or, outside a SpatialTransformer, all L tokens)
        got = as_nchw(out, tap.shape[2] if tap is not None else (self.h or out.shape[1]))
        self.seen[name] = got.detach().clone()
        if tap is None:
            return out
        assert got.shape == tap.shape, (name, tuple(got.shape), tuple(tap.shape))
        return _like(tap, out).to(out.dtype).contiguous()


@contextlib.contextmanager
def forced_transformer_blocks(state):
    """BasicTransformerBlock.forward records and replaces at its three `+ x` points.  Enter it INSIDE fp16_storage when both are wanted
    (as forced_outputs does): the forward it finds patched in tells it that the fp16 pattern is active, and it then rounds the three sums
    as fp16_emu._tblock_forward does."""
    cls = ou.BasicTransformerBlock
    prev = cls.forward
    rnd = r16 if prev is fp16_emu._tblock_forward else (lambda t: t)

    def forward(self, x, context=None):
        name = state.block_names[id(self)]
        x = state.visit(name + SUB_TAPS[0], rnd(self.attn1(self.norm1(x)) + x))
        x = state.visit(name + SUB_TAPS[1], rnd(self.attn2(self.norm2(x), context=context) + x))
        x = state.visit(name + SUB_TAPS[2], rnd(self.ff(self.norm3(x)) + x))
        return x
    cls.forward = forward
    try:
        yield
    finally:
        cls.forward = prev


@contextlib.contextmanager
def forced_clip_layers(state):
    """The same for ClipLayer.forward and its two `+ x` points (fp16_emu._clip_layer_forward tells that the fp16 pattern is active)."""
    cls = oc.ClipLayer
    prev = cls.forward
    rnd = r16 if prev is fp16_emu._clip_layer_forward else (lambda t: t)

    def forward(self, x, mask):
        name = state.block_names[id(self)]
        x = state.visit(name + CLIP_SUB_TAPS[0], rnd(x + self.self_attn(self.layer_norm1(x), mask)))
        return state.visit(name + CLIP_SUB_TAPS[1], rnd(x + self.mlp(self.layer_norm2(x))))
    cls.forward = forward
    try:
        yield
    finally:
        cls.forward = prev


def _run(net, call, names, taps, fp16):
    state = _Forcing(net, names, taps)
    handles = []
    with torch.no_grad(), (fp16_storage(net) if fp16 else contextlib.nullcontext()), forced_transformer_blocks(state), forced_clip_layers(state):
        try:
            for m in state.transformers:
                handles.append(m.register_forward_pre_hook(lambda mod, inp: setattr(state, "h", inp[0].shape[2])))
            for n, m in state.hooked.items():
                handles.append(m.register_forward_hook(lambda mod, inp, out, n=n: state.visit(n, out)))
            call(net)
        finally:
            for h in handles:
                h.remove()
    missed = sorted(n for n in state.names if n not in state.seen)
    if missed:
        raise UnmatchedTap(f"{len(missed)} of {len(state.names)} taps were never reached by the oracle pass: {missed}")
    return state.seen


def forced_outputs(net, call, taps, fp16=False):
    """One teacher-forced pass `call(net)` of the oracle -> {tap name: the oracle's own output there, NCHW fp32}.  `taps`: {name: NCHW
    tensor} of the engine.  `fp16`: under the reference's fp16 rounding pattern (the forcing hooks are registered behind the pattern's
    rounding hooks, so a leaf module's recorded output is the rounded one)."""
    return _run(net, call, list(taps), taps, fp16)


def recorded_outputs(net, call, names, fp16=False):
    """The same recording points on a FREE-RUNNING oracle pass (nothing replaced): {name: NCHW fp32}."""
    return _run(net, call, names, None, fp16)


def unet_tap_names(net):
    """What a traced UNet forward must hand back: every layer of every block, the three `+ x` points of every transformer block — and
    `out`, under which the tests file the network's output."""
    import re
    names = ["out"]
    for n, m in net.named_modules():
        if isinstance(m, ou.BasicTransformerBlock):
            names += [n + s for s in SUB_TAPS]
        elif re.fullmatch(r"(input_blocks\.\d+|middle_block|output_blocks\.\d+)\.\d+", n):
            names.append(n)
    return names


def vae_tap_names(vae):
    """The same for a traced VAE decode (`vae`: the AutoencoderKL): conv_in, the mid blocks, every up block and upsample — and
    `decoder.conv_out` for the image."""
    import re
    return ["decoder." + n for n, _ in vae.decoder.named_modules()
            if re.fullmatch(r"conv_in|conv_out|mid\.(block_1|attn_1|block_2)|up\.\d+\.(block\.\d+|upsample)", n)]


def clip_tap_names(model, layers_run, final_ln):
    """What a traced CLIP forward without the pooled row must hand back (`model`: the ClipTextModel): the embeddings, the two `+ x`
    points of each of the first `layers_run` layers, and `final_layer_norm` when it is applied to the returned state."""
    assert 1 <= layers_run <= len(model.encoder.layers)
    names = ["embeddings"]
    for i in range(layers_run):
        names += [f"encoder.layers.{i}{s}" for s in CLIP_SUB_TAPS]
    return names + (["final_layer_norm"] if final_ln else [])


def vae_encoder_tap_names(vae):
    """The same for a traced VAE encode (`vae`: the AutoencoderKL): conv_in, every down block and downsample, the mid blocks — and
    `quant_conv` for the moments."""
    import re
    return ["encoder." + n for n, _ in vae.encoder.named_modules()
            if re.fullmatch(r"conv_in|down\.\d+\.(block\.\d+|downsample)|mid\.(block_1|attn_1|block_2)", n)] + ["quant_conv"]


def segment_errors(net, call, taps):
    """-> [row per tap, in tap order]: engine = rel_l2(tap, o32), yard = rel_l2(o16, o32), and the worst slice of the engine's error
    per slicing, (value, index).  o32 / o16: the forced pass in fp32 / under the fp16 pattern, on identical forced inputs."""
    o32 = forced_outputs(net, call, taps)
    o16 = forced_outputs(net, call, taps, fp16=True)
    rows = []
    for name, tap in taps.items():
        tap = tap.float()
        row = {"block": name, "shape": tuple(tap.shape), "engine": rel_l2(tap, o32[name]), "yard": rel_l2(o16[name], o32[name])}
        for label, keep in SLICINGS:
            row[label] = worst_slice_rel_l2(tap, o32[name], keep)
        rows.append(row)
    return rows


def segment_kind(net, name):
    """The kind of segment a tap closes (for the report): the oracle class, or the sub-tap point."""
    for s in SUB_TAPS[:2]:
        if name.endswith(s):
            return "block" + s
    if name.endswith(CLIP_SUB_TAPS[0]):
        return "layer" + CLIP_SUB_TAPS[0]
    return type(dict(net.named_modules())[name]).__name__


def assert_segments(rows, label="", verbose=True):
    """Every segment: yard >= YARD_FLOOR, engine <= MARGIN * yard, worst slice of each slicing <= SLICE_FACTOR * MARGIN * yard.  All
    figures are printed before anything is asserted; every violation of the case is reported, not only the first."""
    assert rows, f"{label}: no taps"
    bad = []
    for r in rows:
        cap = MARGIN * r["yard"]
        if verbose:
            print(f"[teacher_forced] {label} {r['block']}: engine {r['engine']:.3e} yard {r['yard']:.3e} ratio {r['engine'] / r['yard']:.3f}"
                  + "".join(f" | worst {s} {r[s][0]:.3e} ({r[s][0] / r['yard']:.2f} x) at {r[s][1]}" for s, _ in SLICINGS))
        if not r["yard"] >= YARD_FLOOR:
            bad.append(f"block {r['block']}: yardstick {r['yard']:.3e} < {YARD_FLOOR:.0e} (engine {r['engine']:.3e}): the cap would be vacuous")
        if not r["engine"] <= cap:
            bad.append(f"block {r['block']}: engine {r['engine']:.3e} > {MARGIN} x yardstick {r['yard']:.3e} = {cap:.3e}")
        for s, _ in SLICINGS:
            worst, idx = r[s]
            if not worst <= SLICE_FACTOR * cap:
                bad.append(f"block {r['block']}: worst {s} slice at {idx}: engine {worst:.3e} > {SLICE_FACTOR} x {MARGIN} x yardstick "
                           f"{r['yard']:.3e} = {SLICE_FACTOR * cap:.3e}")
    assert not bad, f"{label}: {len(bad)} violation(s)\n" + "\n".join(bad)
    return rows
