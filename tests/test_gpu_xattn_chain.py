"""The cross-attention chain (csrc/xattn_chain.hip, ops.xattn_chain: norm2 -> attn2.to_q -> attention over the text context -> attn2.to_out
+ bias + x1 as one launch) on the GPU against the float64 graph on the fp16 operands.  The yardstick is the same graph with LN(x1), q, P,
the attention output and x2 rounded to binary16 (tests/xattn_chain_reference.py); the rule is tests/test_gpu_esrgan.py::assert_parity's —
error <= 1.25 x yardstick on the tensor, <= 2 x 1.25 x yardstick on the worst row and the worst column, yardstick > 1e-4 — asserted on the
output and on the branch out - x1.  tests/test_cpu_xattn_chain.py checks that the twin itself passes that rule on every case below."""
import importlib

import numpy as np
import pytest
import torch

import xattn_chain_reference as X

pytestmark = pytest.mark.gpu


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


def launch(dev, case, out=None, **over):
    """-> (rc, out tensor).  Through the C ABI directly, so that a refusal can be looked at."""
    _lib = sub("_lib")
    t = {k: (torch.from_numpy(case[k]).to(dev) if case[k] is not None else None) for k in ("x", "gamma", "beta", "wq", "wo", "bo", "k", "vt")}
    out = torch.empty_like(t["x"]) if out is None else out
    a = dict(rows=case["x"].shape[0], rpi=case["rpi"], C=X.C_WIDTH, heads=X.HEADS, L=case["L"], Lpad=case["Lpad"])
    for k in list(over):
        if k in t:
            t[k] = over.pop(k)
    a.update(over)
    p = lambda v: _lib.ptr(v) if v is not None else None
    rc = _lib.lib.sdmi_xattn_chain(p(t["x"]), p(out), p(t["gamma"]), p(t["beta"]), p(t["wq"]), p(t["wo"]), p(t["bo"]), p(t["k"]), p(t["vt"]),
                                   a["rows"], a["rpi"], a["C"], a["heads"], a["L"], a["Lpad"], 1e-5, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def case_id(s):
    return f"{s['images']}x{s['rpi']}-L{s['L']}-{s.get('kind', 'plain')}" + ("-poison" if s.get("poison") else "") + ("" if s.get("bias", True) else "-nobias")


@pytest.mark.parametrize("spec", X.GPU_CASES, ids=case_id)
def test_xattn_chain_against_float64(dev, spec):
    """One tile and three images of two tiles (a context per image: tile -> image mapping, tile order, the second row half); context
    lengths 1, 32, 33, 77, 96, 154 (a single key, exact and ragged 32-key blocks, the common length, a long prompt); V^T padding columns
    poisoned in one case (the mask, not the padding, excludes keys >= L); one key about 30 log2 units above the rest in the last ragged
    block, scores climbing block by block, a first block far below the others (the online softmax's re-basing); token rows with mean 50
    and spread 0.5 (the LayerNorm's centred statistics); with and without the output bias."""
    case = X.make_case(**spec)
    rc, out = launch(dev, case)
    assert rc == 0, sub("_lib").last_error()
    X.assert_chain_parity(out.float().cpu().numpy(), case)


def test_xattn_chain_ops_wrapper_is_deterministic(dev):
    """ops.xattn_chain (the binding the engine-independent callers use) gives the C ABI's result, and two launches on the same inputs give
    identical bits."""
    ops = sub("ops")
    case = X.make_case(2, 256, 77, seed=21)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("x", "gamma", "beta", "wq", "wo", "bo", "k", "vt")}
    x3 = t["x"].view(2, 256, X.C_WIDTH)
    a = ops.xattn_chain(x3, t["gamma"], t["beta"], t["wq"], t["wo"], t["bo"], t["k"], t["vt"], case["L"])
    b = ops.xattn_chain(x3, t["gamma"], t["beta"], t["wq"], t["wo"], t["bo"], t["k"], t["vt"], case["L"])
    rc, c = launch(dev, case)
    assert rc == 0
    assert torch.equal(a, b)
    assert torch.equal(a.view(-1, X.C_WIDTH), c)


def test_xattn_chain_refusals(dev):
    """Each host-side refusal returns non-zero with its message and leaves a sentinel-filled output untouched."""
    _lib = sub("_lib")
    case = X.make_case(1, 256, 40, seed=22)
    for over, msg in ((dict(C=640), "C = 320"), (dict(heads=5), "heads * 40"), (dict(rows=200), "rows % 128"), (dict(rpi=64), "rows_per_image % 128"),
                      (dict(L=0), "L >= 1"), (dict(x=None), "null pointer"), (dict(gamma=None), "null pointer"), (dict(beta=None), "null pointer"),
                      (dict(wq=None), "null pointer"), (dict(wo=None), "null pointer"), (dict(k=None), "null pointer"), (dict(vt=None), "null pointer")):
        sentinel = torch.full((256, X.C_WIDTH), 7.0, dtype=torch.float16, device=dev)
        rc, out = launch(dev, case, out=sentinel, **over)
        assert rc != 0, over
        assert msg in _lib.last_error(), (over, _lib.last_error())
        assert bool((out == 7.0).all()), over
    rc, out = launch(dev, case)                                  # (a valid launch afterwards still works)
    assert rc == 0 and bool(torch.isfinite(out.float()).all())
