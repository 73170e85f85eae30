#!/usr/bin/env python3
"""Isolated timing of the level-0 self-attention forms (csrc/attention.hip): 17 and 27 (17 for q and k pre-scaled by
sqrt(scale * log2 e), staging addresses out of the KV loop), one process, forms interleaved round by round.

    python tools/gpu/attn_l0_time.py [--reps 5] [--iters 10] [--shapes c1|all] [--out FILE.json]

Torch-free (tools/gpu/hipmem.py), numpy inputs laid out as the engine lays them out (q | k stacked, row stride 2 * H * D), the C ABI entry
sdmi_attention_vt_ex.  Form 17 takes the unscaled fp16 operands, 27 the same fp32 values scaled and rounded once.  Reported per form:
min and median microseconds, TFLOP/s, the output's rel-L2 distance from form 17's (and whether the bits are equal) and, on the first
heads of the first image, the rel-L2 error of every form against a float64 softmax of its own operands.  Isolated loops (K / V^T
cache-resident): in-job times are 5-15 % higher.  (Does not import oracle/.)
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
import numpy as np  # noqa: E402

PKG = "stable-diffusion-webui_amd"
D = 40
FORMS = ((17, False), (27, True))
SHAPES = {"c1": [("c1 self level 0 (B*H = 128)", 16, 8, 4096)], "all": [("c4a hires self level 0", 2, 8, 16384)]}


def ref64(q, k, vt, heads, m, scale):
    """float64 softmax(scale * q k^T) v of image 0, the first `heads` heads, the first 256 queries."""
    out = []
    for h in range(heads):
        qq = q[0, :256, h * D:(h + 1) * D].astype(np.float64)
        kk = k[0, :, h * D:(h + 1) * D].astype(np.float64)
        s = qq @ kk.T * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out.append((p / p.sum(axis=1, keepdims=True)) @ vt[0, h * D:(h + 1) * D, :m].astype(np.float64).T)
    return np.concatenate(out, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="all", choices=("c1", "all"))
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    import hipmem
    _lib = importlib.import_module(f"{PKG}._lib")
    _lib.require_device()
    lib = _lib.lib
    hipmem.set_device(0)
    rng = np.random.default_rng(1)
    res = {}
    e0, e1 = hipmem.Event(), hipmem.Event()
    for name, b, h, n in SHAPES["c1"] + (SHAPES["all"] if args.shapes == "all" else []):
        c = h * D
        scale = D ** -0.5
        rs = np.float32(np.sqrt(scale * 1.4426950408889634))
        qk32 = rng.standard_normal((b, n, 2 * c), dtype=np.float32)
        qk, qks = qk32.astype(np.float16), (qk32 * rs).astype(np.float16)
        del qk32
        vt = rng.standard_normal((b, c, n), dtype=np.float32).astype(np.float16)
        dqk, dqks, dvt = hipmem.DevBuf.from_numpy(qk), hipmem.DevBuf.from_numpy(qks), hipmem.DevBuf.from_numpy(vt)
        dout = hipmem.DevBuf(b * n * c * 2)

        def launch(form, pre):
            src = dqks if pre else dqk
            _lib.check(lib.sdmi_attention_vt_ex(src.ptr, C.c_void_p(src.ptr.value + 2 * c), dvt.ptr, dout.ptr, b, h, n, n, D, 2 * c, 2 * c, n, c, C.c_float(scale),
                                                int(pre), form, 0, None), "attention_vt_ex")
        flops = 4.0 * b * h * n * n * D
        times = {f: [] for f, _ in FORMS}
        outs = {}
        for rep in range(args.reps):
            for form, pre in FORMS:
                launch(form, pre)
                hipmem.sync()
                if form not in outs:
                    outs[form] = dout.to_numpy(np.float16, (b, n, c)).astype(np.float32)
                e0.record()
                for _ in range(args.iters):
                    launch(form, pre)
                e1.record()
                times[form].append(e1.ms_since(e0) / args.iters * 1e3)
        refs = {False: ref64(qk[:, :, :c], qk[:, :, c:], vt, 2, n, scale), True: ref64(qks[:, :, :c], qks[:, :, c:], vt, 2, n, np.log(2.0))}
        res[name] = {}
        print(f"{name}  (B {b} H {h} N = M {n} D {D})")
        for form, pre in FORMS:
            us = min(times[form])
            a, base = outs[form].astype(np.float64), outs[17].astype(np.float64)
            rel = float(np.linalg.norm(a - base) / np.linalg.norm(base))
            same = bool(np.array_equal(outs[form], outs[17]))
            got = a[0, :256, :2 * D]
            err = float(np.linalg.norm(got - refs[pre]) / np.linalg.norm(refs[pre]))
            res[name][str(form)] = {"us_min": round(us, 2), "us_median": round(statistics.median(times[form]), 2), "tflops": round(flops / us / 1e6, 1),
                                    "rel_l2_vs_17": rel, "identical_to_17": same, "rel_l2_vs_float64": err}
            print(f"    form {form:2d}  min {us:9.1f} us  median {statistics.median(times[form]):9.1f} us  {flops / us / 1e6:7.1f} TFLOP/s  "
                  f"rel-L2 vs 17: {rel:.2e}{' (bit-identical)' if same else ''}  vs float64: {err:.3e}", flush=True)
        for buf in (dqk, dqks, dvt, dout):
            buf.free()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
