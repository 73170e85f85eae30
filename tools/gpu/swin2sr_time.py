"""Times Swin2SR on the engine (profiles/swin2sr_time.md), HIP events around every repeat after warm-up, one step per process:

    net SIDE     the real-world x4 geometry (embed 180, 6 x 6 blocks, 6 heads, hidden 360, 1conv, nearest+conv) with seeded weights on a
                 SIDE x SIDE image, B = 1: ms per image through sdmi_swin2sr_run, alternating with a SwinIR network of the same geometry
                 through sdmi_swinir_run (the launches of swinir_pass for a SwinIR network are what they were before Swin2SR was added),
                 then the engine's per-launch HIP-event table of one run of each
    attn SIDE    swin2_window_attn against swin_window_attn on SIDE x SIDE tokens, 6 heads of 30, shift 4, the two alternating

    for s in "net 128" "net 256" "attn 128" "attn 256"; do timeout -k 10 300 python tools/gpu/swin2sr_time.py $s OUT_DIR || break; done
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
import swin2sr_reference as R2
import swinir_reference as R1

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
ops = importlib.import_module("stable-diffusion-webui_amd.ops")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")

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


def profile_of(fn):
    torch.cuda.synchronize()
    _lib.lib.sdmi_profile_begin()
    fn()
    buf = C.create_string_buffer(1 << 18)
    _lib.lib.sdmi_profile_end(buf, len(buf))
    return json.loads(buf.value.decode())


res = {"step": step, "side": side}
if step == "net":
    engine = importlib.import_module("stable-diffusion-webui_amd.engine").Engine(0)
    v2 = up.Swin2SRNet(R2.make_state_dict(180, (6,) * 6, 6, "1conv", 4, "nearest+conv"), device=0, engine=engine)
    v1 = up.SwinIRNet(R1.make_state_dict(180, (6,) * 6, 6, "1conv", 4), device=0, engine=engine)
    x = R1.image(1, side, side, 1).to(dev)
    res["scratch_gib"] = {"swin2sr": v2.scratch_bytes(1, side, side) / 2 ** 30, "swinir": v1.scratch_bytes(1, side, side) / 2 ** 30}
    res.update(timed({"swin2sr": lambda: v2.run(x), "swinir": lambda: v1.run(x)}, reps=10))
    res["ratio_swin2sr_over_swinir"] = res["swin2sr"]["median_ms"] / res["swinir"]["median_ms"]
    res["profile"] = {"swin2sr": profile_of(lambda: v2.run(x)), "swinir": profile_of(lambda: v1.run(x))}
else:
    heads, d = 6, 30
    g = torch.Generator().manual_seed(7)
    qkv = torch.zeros((1, side, side, 96 * heads), dtype=torch.float16)
    for s in range(3 * heads):
        qkv[..., 32 * s:32 * s + d] = torch.randn((1, side, side, d), generator=g).half()
    qkv = qkv.to(dev)
    bias = torch.randn((heads, 64, 64), generator=g).to(dev)
    tau = torch.full((heads,), 10.0).to(dev)
    o1, o2 = (torch.zeros((1, side, side, 32 * heads), dtype=torch.float16, device=dev) for _ in range(2))
    res["tokens"] = side * side
    res.update(timed({"swin2_window_attn": lambda: ops.swin2_attention(qkv, bias, tau, heads, d, shift=4, out=o2),
                      "swin_window_attn": lambda: ops.swin_attention(qkv, bias, heads, d, shift=4, out=o1)}))
    res["ratio_swin2_over_swin"] = res["swin2_window_attn"]["median_ms"] / res["swin_window_attn"]["median_ms"]

print(json.dumps({k: v for k, v in res.items() if k != "profile"}), flush=True)
for name, prof in res.get("profile", {}).items():
    total = sum(k["ms"] for k in prof["kernels"])
    print(f"-- {name}: {total:.3f} ms in kernels", flush=True)
    for k in prof["kernels"]:
        print(k["name"], k["launches"], f'{k["ms"]:.3f} ms', f'{100 * k["ms"] / total:.1f} %', flush=True)
if out_dir:
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, f"swin2sr_time_{step}{side}.json"), "w"), indent=1)
