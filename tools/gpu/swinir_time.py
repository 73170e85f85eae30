"""Times a SwinIR-L-shaped network (embed_dim 240, depths 9 x 6, 8 heads, 3conv, mlp_ratio 2, x4, nearest+conv) on seeded weights on a
512 x 512 image, B = 1 (profiles/swinir_time.md): the engine (sdmi_swinir_run, fp32 out), and the same weights as the restated
reference module (tests/swinir_reference.py) in .half() on the GPU on the image whole — the yardstick of profiles/esrgan_time.md and
compact_time.md; then the engine's per-launch HIP-event table.

    python tools/gpu/swinir_time.py [OUT.json]        # one process, every figure a median of synchronised wall-clock repeats after warm-up
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
import swinir_reference as R

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")

out = {}
sd = R.make_state_dict(240, (6,) * 9, 8, "3conv", 4)
net = up.SwinIRNet(sd, device=0)
dev = torch.device("cuda", 0)
module = R.SwinIRModule(sd).half().to(dev)


def timed(fn, warm=2, reps=7):
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


x = R.image(1, 512, 512, 1).to(dev)
xh = x.half()
with torch.no_grad():
    got = net.run(x)
    half = module(xh).float()
    out["shape"] = list(got.shape)
    out["scratch_gib"] = net.scratch_bytes(1, 512, 512) / 2 ** 30
    out["rel_l2_engine_vs_torch_half"] = float((got - half).norm() / half.norm())
    out["engine"] = timed(lambda: net.run(x))
    out["engine_u8"] = timed(lambda: net.run(x, out_u8=True))
    out["torch_half_whole"] = timed(lambda: module(xh))
print(json.dumps(out), flush=True)

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
total = sum(k["ms"] for k in out["profile_b1"]["kernels"])
for k in out["profile_b1"]["kernels"]:
    print(k["name"], k["launches"], f'{k["ms"]:.3f} ms', f'{100 * k["ms"] / total:.1f} %', f'{k["flops"] / max(k["ms"], 1e-9) / 1e9:.1f} TFLOP/s')
