"""Times HAT on the engine (profiles/hat_time.md), HIP events around every repeat after warm-up, one step per process:

    net SIDE     the HAT x4 geometry (embed 180, 6 x 6 blocks, 6 heads, compress 3, squeeze 30, mlp ratio 2, pixelshuffle) with seeded
                 weights on a SIDE x SIDE image, B = 1: ms per image through sdmi_hat_run, then the engine's per-launch HIP-event table of
                 one run
    torch SIDE   the restated reference (tests/hat_reference.py) in fp16 under torch on the same device and the whole image, same weights

    for s in "net 128" "net 256" "torch 128" "torch 256"; do timeout -k 10 300 python tools/gpu/hat_time.py $s OUT_DIR || break; done
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
import hat_reference as R

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")

step, side = sys.argv[1], int(sys.argv[2])
out_dir = sys.argv[3] if len(sys.argv) > 3 else None
_lib.require_device()
dev = torch.device("cuda", 0)


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": sorted(ms)[len(ms) // 2], "min_ms": min(ms), "max_ms": max(ms), "reps": reps, "warmup": warm}


def profile_of(fn):
    torch.cuda.synchronize()
    _lib.lib.sdmi_profile_begin()
    fn()
    buf = C.create_string_buffer(1 << 18)
    _lib.lib.sdmi_profile_end(buf, len(buf))
    return json.loads(buf.value.decode())


sd = R.make_state_dict(180, (6,) * 6, 6, 3, 30, 2, 4)
x = R.image(1, side, side, 1)
res = {"step": step, "side": side}
if step == "net":
    engine = importlib.import_module("stable-diffusion-webui_amd.engine").Engine(0)
    net = up.HATNet(sd, device=0, engine=engine)
    xd = x.to(dev)
    res["scratch_gib"] = net.scratch_bytes(1, side, side) / 2 ** 30
    res["engine"] = timed(lambda: net.run(xd))
    res["profile"] = profile_of(lambda: net.run(xd))
else:
    half = {k: (v.half() if v.is_floating_point() else v).to(dev) for k, v in sd.items()}
    xh = x.half().to(dev)
    with torch.no_grad():
        res["torch_fp16"] = timed(lambda: R.forward(half, xh))

print(json.dumps({k: v for k, v in res.items() if k != "profile"}), flush=True)
if "profile" in res:
    total = sum(k["ms"] for k in res["profile"]["kernels"])
    print(f"-- {total:.3f} ms in kernels", flush=True)
    for k in res["profile"]["kernels"]:
        print(k["name"], k["launches"], f'{k["ms"]:.3f} ms', f'{100 * k["ms"] / total:.1f} %', flush=True)
if out_dir:
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, f"hat_time_{step}{side}.json"), "w"), indent=1)
