"""Times a General-4xV3-shaped compact network (num_conv 32, x4) on a 512 x 512 image, B = 1 and 2 (profiles/compact_time.md): the engine
(sdmi_compact_run, fp32 and uint8 out), the same weights as the torch reference module (tests/compact_reference.py) in .half() on the GPU
on the image whole and over nine 192-px tiles; then one layer, sdmi_compact_conv 64 -> 64 PReLU against sdmi_rrdb_conv 64 -> 64 LeakyReLU
at M = 512^2, alternating in the same process; then the engine's per-launch HIP-event table.

    python tools/gpu/compact_time.py [OUT.json]       # one process, every figure a median of synchronised wall-clock repeats after warm-up
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
import compact_reference as R

up = importlib.import_module("stable-diffusion-webui_amd.upscaler")
ops = importlib.import_module("stable-diffusion-webui_amd.ops")
_lib = importlib.import_module("stable-diffusion-webui_amd._lib")

out = {}
sd = R.make_state_dict(32, 4)
net = up.CompactNet(sd, device=0)
dev = torch.device("cuda", 0)
sdh = {k: v.half().to(dev) for k, v in sd.items()}
sdf = {k: v.to(dev) for k, v in sd.items()}


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
    x = R.image(b, 512, 512, b).to(dev)
    xh = x.half()
    with torch.no_grad():
        got = net.run(x)
        half = R.forward(sdh, xh).float()
        ref = R.forward(sdf, x)                          # the same module in fp32 on the device: the yardstick of both fp16 sides
        res = ref - R.base(sd, x)
        out[f"b{b}_residual_rel_l2_engine_vs_fp32"] = float((got - ref).norm() / res.norm())
        out[f"b{b}_residual_rel_l2_torch_half_vs_fp32"] = float((half - ref).norm() / res.norm())
        out[f"b{b}_engine"] = timed(lambda: net.run(x))
        out[f"b{b}_engine_u8"] = timed(lambda: net.run(x, out_u8=True))
        out[f"b{b}_torch_half_whole"] = timed(lambda: R.forward(sdh, xh), warm=2, reps=5)
        out[f"b{b}_torch_half_tiles192"] = timed(lambda: tiles(xh), warm=2, reps=5)
    print(json.dumps({k: v for k, v in out.items() if k.startswith(f"b{b}")}), flush=True)

# ---- the layer: the same work through both kernels, alternating ----
g = torch.Generator().manual_seed(3)
xl = (torch.randn((1, 512, 512, 64), generator=g) * 0.5).half().to(dev)
wt = (torch.randn((64, 64, 3, 3), generator=g) * 0.04).to(dev)
bias = torch.zeros(64, dtype=torch.float32, device=dev)
slope = torch.full((64,), 0.2, dtype=torch.float32, device=dev)
wc, wr = ops.pack_compact_weight(wt), ops.pack_rrdb_weight(wt, 64)
oc, orr = torch.empty_like(xl), torch.empty_like(xl)
flop = 2.0 * 512 * 512 * 64 * 9 * 64
a = ops.compact_conv(xl, wc, bias, slope=slope, ep="prelu", out=oc)
bb = ops.rrdb_conv(xl, wr, bias, out=orr, ep="lrelu")
out["layer_max_abs_diff_compact_vs_rrdb"] = float((a.float() - bb.float()).abs().max())
LAUNCHES = 200                                     # per timed window: ~10 ms of device work, one synchronise at its end
layer = {"compact_conv": [], "rrdb_conv64": []}
for rnd in range(7):
    for name, fn in (("compact_conv", lambda: ops.compact_conv(xl, wc, bias, slope=slope, ep="prelu", out=oc)),
                     ("rrdb_conv64", lambda: ops.rrdb_conv(xl, wr, bias, out=orr, ep="lrelu"))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LAUNCHES):
            fn()
        torch.cuda.synchronize()
        layer[name].append((time.perf_counter() - t0) * 1e3 / LAUNCHES)
for name, ts in layer.items():
    ts.sort()
    out[f"layer_{name}"] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "rounds": len(ts), "launches_per_round": LAUNCHES,
                            "tflops_at_median": flop / ts[len(ts) // 2] / 1e9}
print(json.dumps({k: v for k, v in out.items() if k.startswith("layer")}), flush=True)

x = R.image(1, 512, 512, 1).to(dev)
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
