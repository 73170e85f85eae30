#!/usr/bin/env python3
"""Torch-free check + isolated timing of the cross-attention chain (csrc/xattn_chain.hip) against the four launches it replaces, at the
C1 level-0 shape: 16 images x 4096 tokens x 320, 77 context keys.

    python tools/gpu/xattn_chain_time.py [--rows 65536] [--rows-per-image 4096] [--L 77] [--iters 30] [--rounds 5]

Both paths run on the same seeded random operands (not zeros): LayerNorm -> to_q GEMM -> attention over the cached K / V^T -> to_out GEMM
+ bias + residual through the C ABI's op entries, and sdmi_xattn_chain.  Their outputs are compared with each other over the whole
tensor and with the float64 graph (tests/xattn_chain_reference.py) on the first and the last 128-row tile; then loops of `--iters`
launches are timed with HIP events, the two paths interleaved over `--rounds` rounds (min / median per launch sequence).
Device memory through tools/gpu/hipmem.py (no `import torch`).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PKG = "stable-diffusion-webui_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rows-per-image", type=int, default=4096)
    ap.add_argument("--L", type=int, default=77)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the result as JSON to this file")
    args = ap.parse_args()
    import hipmem
    import xattn_chain_reference as X
    _lib = importlib.import_module(f"{PKG}._lib")
    _lib.require_device()
    lib = _lib.lib
    hipmem.set_device(0)
    rows, rpi, L = args.rows, args.rows_per_image, args.L
    images = rows // rpi
    case = X.make_case(images, rpi, L, seed=3)
    Cw, H, D, Lpad = X.C_WIDTH, X.HEADS, X.DHEAD, case["Lpad"]
    dev = {k: hipmem.DevBuf.from_numpy(case[k]) for k in ("x", "gamma", "beta", "wq", "wo", "bo", "k", "vt")}
    n2, q2, a2, out4, out1 = (hipmem.DevBuf(rows * Cw * 2) for _ in range(5))

    def linear(a, w, bias, resid, out):
        d = _lib.ConvDesc()
        d.a0, d.w, d.out = a.ptr, w.ptr, out.ptr
        d.bias = bias.ptr if bias is not None else None
        d.resid = resid.ptr if resid is not None else None
        d.c0, d.lda0 = Cw, Cw
        d.B, d.Hi, d.Wi, d.Ho, d.Wo = 1, rows, 1, rows, 1
        d.taps, d.stride, d.pad, d.up = 1, 1, 0, 0
        d.N, d.n_real, d.ldo, d.ldr = Cw, Cw, Cw, Cw
        d.alpha, d.batch = 1.0, 1
        _lib.check(lib.sdmi_conv_gemm(C.byref(d), None), "conv_gemm")

    def four():
        _lib.check(lib.sdmi_layernorm(dev["x"].ptr, dev["gamma"].ptr, dev["beta"].ptr, n2.ptr, rows, Cw, 1e-5, None), "layernorm")
        linear(n2, dev["wq"], None, None, q2)
        _lib.check(lib.sdmi_attention_vt(q2.ptr, dev["k"].ptr, dev["vt"].ptr, a2.ptr, images, H, rpi, L, D, Cw, Cw, Lpad, Cw, D ** -0.5, 0, None),
                   "attention_vt")
        linear(a2, dev["wo"], dev["bo"], dev["x"], out4)

    def chain():
        _lib.check(lib.sdmi_xattn_chain(dev["x"].ptr, out1.ptr, dev["gamma"].ptr, dev["beta"].ptr, dev["wq"].ptr, dev["wo"].ptr, dev["bo"].ptr,
                                        dev["k"].ptr, dev["vt"].ptr, rows, rpi, Cw, H, L, Lpad, 1e-5, None), "xattn_chain")

    four(); chain(); hipmem.sync()
    o4 = out4.to_numpy(np.float16, (rows, Cw)).astype(np.float64)
    o1 = out1.to_numpy(np.float16, (rows, Cw)).astype(np.float64)
    x64 = case["x"].astype(np.float64)
    res = {"rows": rows, "rows_per_image": rpi, "L": L, "iters": args.iters,
           "chain_vs_four_rel_l2": X.rel_l2(o1, o4), "chain_vs_four_branch_rel_l2": X.rel_l2(o1 - x64, o4 - x64),
           "finite": bool(np.isfinite(o1).all())}
    for name, img, r0 in (("first tile", 0, 0), ("last tile", images - 1, rows - 128)):
        sub = dict(case, x=case["x"][r0:r0 + 128], k=case["k"][img:img + 1], vt=case["vt"][img:img + 1], rpi=128, images=1)
        ref, twin = X.graph(sub), X.graph(sub, twin=True)
        xs = x64[r0:r0 + 128]
        res[name] = {"chain": X.rel_l2(o1[r0:r0 + 128], ref), "four": X.rel_l2(o4[r0:r0 + 128], ref), "twin": X.rel_l2(twin, ref),
                     "chain_branch": X.rel_l2(o1[r0:r0 + 128] - xs, ref - xs), "four_branch": X.rel_l2(o4[r0:r0 + 128] - xs, ref - xs),
                     "twin_branch": X.rel_l2(twin - xs, ref - xs)}
    print(json.dumps(res, indent=1), flush=True)

    e0, e1 = hipmem.Event(), hipmem.Event()

    def timed(fn):
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        hipmem.sync()
        return e1.ms_since(e0) / args.iters * 1e3

    us = {"four": [], "chain": []}
    for _ in range(args.rounds):
        us["four"].append(timed(four))
        us["chain"].append(timed(chain))
    for k, v in us.items():
        res[k + "_us"] = {"min": round(min(v), 1), "median": round(statistics.median(v), 1), "all": [round(t, 1) for t in v]}
        print(f"{k:6s} us per sequence: min {min(v):.1f}  median {statistics.median(v):.1f}  {[round(t, 1) for t in v]}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ok = res["finite"] and res["chain_vs_four_branch_rel_l2"] < 2e-3
    print("ok" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
