"""Times ScuNET on the engine (profiles/scunet_time.md), HIP events around every repeat after warm-up, one step per process:

    net SIDE     a [4] * 7 network (the shipped depths) with seeded weights on a SIDE x SIDE image, B = 1: ms per image through
                 sdmi_scunet_run (fp32 out), then the engine's per-launch HIP-event table of one run
    block SIDE   one level-1 transformer Block (trans_dim 32, 'SW') on SIDE x SIDE tokens, as the network launches it (columns 32..63 of
                 64-wide rows): the fused scu_block launch, and the same Block composed from the launches the engine had before on rows
                 padded to 64 (swin_layernorm, conv_gemm, swin_window_attn; seven launches, built here only), the two alternating

    for s in "net 512" "net 1024" "block 512" "block 1024"; do timeout -k 10 300 python tools/gpu/scunet_time.py $s OUT_DIR || break; done
"""
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scunet_reference as R

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
ops = importlib.import_module("stable-diffusion-webui_amd.ops")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")
EP_GELU = 32

step, side = sys.argv[1], int(sys.argv[2])
out_dir = sys.argv[3] if len(sys.argv) > 3 else None
_lib.require_device()
dev = torch.device("cuda", 0)


def timed(fns, warm=3, reps=15):
    """Every fn of `fns` in turn per repeat (two versions alternate), each between two events -> per fn median / min / max ms."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v), "reps": reps, "warmup": warm} for k, v in ms.items()}


res = {"step": step, "side": side}
if step == "net":
    net = up.ScuNETNet(R.make_state_dict((4,) * 7), device=0)
    x = R.image(1, side, side, 1).to(dev)
    res["scratch_gib"] = net.scratch_bytes(1, side, side) / 2 ** 30
    res.update(timed({"engine": lambda: net.run(x), "engine_u8": lambda: net.run(x, out_u8=True)}, reps=10))
    torch.cuda.synchronize()
    _lib.lib.sdmi_profile_begin()
    net.run(x)
    buf = C.create_string_buffer(1 << 18)
    _lib.lib.sdmi_profile_end(buf, len(buf))
    res["profile"] = json.loads(buf.value.decode())
else:
    c, m = 32, side * side
    sd = {}
    R.make_block(sd, "b.", c, torch.Generator().manual_seed(5))
    g = {k[2:]: v.to(dev) for k, v in sd.items()}
    packs = ops.scu_block_pack(g["ln1.weight"], g["ln1.bias"], g["msa.embedding_layer.weight"], g["msa.embedding_layer.bias"], g["msa.linear.weight"],
                               g["msa.linear.bias"], g["ln2.weight"], g["ln2.bias"], g["mlp.0.weight"], g["mlp.0.bias"], g["mlp.2.weight"], g["mlp.2.bias"])
    bias = R.relative_bias(sd["b.msa.relative_position_params"]).contiguous().to(dev)
    rows = torch.zeros((1, side, side, 64), dtype=torch.float16, device=dev)
    rows[..., 32:] = torch.randn((1, side, side, c), generator=torch.Generator().manual_seed(6)).half().to(dev)
    fused_out = torch.zeros_like(rows)

    # the composed form: the Block's rows alone, padded to 64 columns with zeros, every tensor made once
    xp = torch.zeros_like(rows)
    xp[..., :c] = rows[..., 32:]
    pw = {n: ops.pack_conv_weight(g[n + ".weight"]) for n in ("msa.embedding_layer", "msa.linear", "mlp.0", "mlp.2")}      # rows / columns padded to 64
    pb = {n: ops.pack_bias(g[n + ".bias"], pw[n].shape[0]) for n in pw}
    t = {n: torch.zeros((1, side, side, w), dtype=torch.float16, device=dev) for n, w in
         (("ln", 64), ("qkv", 128), ("att", 64), ("x1", 64), ("ln2", 64), ("hid", 128), ("out", 64))}

    def gemm(a, name, o, resid=None, flags=0):
        d = _lib.ConvDesc()
        d.a0, d.w, d.bias, d.out = a.data_ptr(), pw[name].data_ptr(), pb[name].data_ptr(), o.data_ptr()
        d.resid = resid.data_ptr() if resid is not None else None
        d.c0 = d.lda0 = a.shape[3]
        d.B, d.Hi, d.Wi, d.Ho, d.Wo, d.taps, d.stride, d.batch = 1, side, side, side, side, 1, 1, 1
        d.N = d.ldo = o.shape[3]
        d.ldr = resid.shape[3] if resid is not None else 0
        d.flags, d.alpha = flags, 1.0
        _lib.check(_lib.lib.sdmi_conv_gemm(C.byref(d), _lib.stream_ptr()), "sdmi_conv_gemm")

    def composed():
        ops.swin_layernorm(xp, g["ln1.weight"], g["ln1.bias"], out=t["ln"])
        gemm(t["ln"], "msa.embedding_layer", t["qkv"])
        ops.swin_attention(t["qkv"], bias, 1, 32, shift=4, out=t["att"])
        gemm(t["att"], "msa.linear", t["x1"], resid=xp)
        ops.swin_layernorm(t["x1"], g["ln2.weight"], g["ln2.bias"], out=t["ln2"])
        gemm(t["ln2"], "mlp.0", t["hid"], flags=EP_GELU)
        gemm(t["hid"], "mlp.2", t["out"], resid=t["x1"])

    def fused():
        ops.scu_block(rows, packs, bias, c, shift=4, col=32, out=fused_out, out_col=32)

    fused()
    composed()
    a, b = fused_out[..., 32:].float(), t["out"][..., :c].float()
    res["rel_l2_fused_vs_composed"] = float((a - b).norm() / b.norm())
    res["tokens"] = m
    res.update(timed({"fused_scu_block": fused, "composed_7_launches": composed}))

print(json.dumps({k: v for k, v in res.items() if k != "profile"}), flush=True)
if "profile" in res:
    total = sum(k["ms"] for k in res["profile"]["kernels"])
    for k in res["profile"]["kernels"]:
        print(k["name"], k["launches"], f'{k["ms"]:.3f} ms', f'{100 * k["ms"] / total:.1f} %', flush=True)
if out_dir:
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, f"scunet_time_{step}{side}.json"), "w"), indent=1)
