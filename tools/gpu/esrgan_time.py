"""Times a 23-block x4 RRDBNet on a 512 x 512 image, B = 1 and 2 (profiles/esrgan_time.md): the engine (sdmi_esrgan_run), the same weights
as the torch reference module (tests/rrdb_reference.py) in .half() on the GPU on the image whole, and the same module over nine 192-px
tiles (the webui's default ESRGAN_tile = 192 / overlap 8 on a 512 x 512 image).  Then the engine's per-launch HIP-event table.

    python tools/gpu/esrgan_time.py [OUT.json]        # one process, every figure a median of synchronised wall-clock repeats after warm-up
"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rrdb_reference as R

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")

out = {}
sd = R.make_state_dict(23, 4)
net = up.EsrganNet(sd, device=0)
dev = torch.device("cuda", 0)
sdh = {k: v.half().to(dev) for k, v in sd.items()}


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps, "warmup": warm}


def tiles(x):
    outs = []
    for y0 in (0, 160, 320):
        for x0 in (0, 160, 320):
            outs.append(R.forward(sdh, x[:, :, y0:y0 + 192, x0:x0 + 192]))
    return outs


for b in (1, 2):
    x = torch.rand((b, 3, 512, 512), generator=torch.Generator().manual_seed(b)).to(dev)
    xh = x.half()
    with torch.no_grad():
        got = net.run(x)
        ref = R.forward(sdh, xh).float()
        out[f"b{b}_rel_l2_engine_vs_torch_half"] = float((got - ref).norm() / ref.norm())
        out[f"b{b}_engine"] = timed(lambda: net.run(x))
        out[f"b{b}_engine_u8"] = timed(lambda: net.run(x, out_u8=True))
        out[f"b{b}_torch_half_whole"] = timed(lambda: R.forward(sdh, xh), warm=2, reps=5)
        out[f"b{b}_torch_half_tiles192"] = timed(lambda: tiles(xh), warm=2, reps=5)
    print(json.dumps({k: v for k, v in out.items() if k.startswith(f"b{b}")}), flush=True)

x = torch.rand((1, 3, 512, 512)).to(dev)
net.run(x)
torch.cuda.synchronize()
_lib.lib.sdmi_profile_begin()
net.run(x)
buf = C.create_string_buffer(1 << 16)
_lib.lib.sdmi_profile_end(buf, len(buf))
out["profile_b1"] = json.loads(buf.value.decode())
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
for k in out["profile_b1"]["kernels"]:
    print(k["name"], k["launches"], f'{k["ms"]:.3f} ms', f'{k["flops"] / max(k["ms"], 1e-9) / 1e9:.1f} TFLOP/s')
