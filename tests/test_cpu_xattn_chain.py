"""CPU tier of the cross-attention chain (csrc/xattn_chain.hip): the kernel's own source on the host-emulated library against the float64
graph, the fp16-storage twin against its own parity rule on every case of the GPU test, the launcher's refusals, and the code-object
metadata of the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import xattn_chain_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def threaded(hostemu_lib):
    """The host-emulated library with every thread of the running block a fiber (real barriers, MFMA / LDS-DMA builtins emulated)."""
    lib = C.CDLL(hostemu_lib)
    lib.sdmi_last_error.restype = C.c_char_p
    lib.emu_set_threaded(1)
    yield lib
    lib.emu_set_threaded(0)


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def run(lib, case, out=None, **over):
    a = dict(x=case["x"], out=np.zeros_like(case["x"]) if out is None else out, gamma=case["gamma"], beta=case["beta"], wq=case["wq"],
             wo=case["wo"], bo=case["bo"], k=case["k"], vt=case["vt"], rows=case["x"].shape[0], rpi=case["rpi"], C=X.C_WIDTH, heads=X.HEADS,
             L=case["L"], Lpad=case["Lpad"])
    a.update(over)
    rc = lib.sdmi_xattn_chain(p(a["x"]), p(a["out"]), p(a["gamma"]), p(a["beta"]), p(a["wq"]), p(a["wo"]), p(a["bo"]), p(a["k"]), p(a["vt"]),
                              C.c_int64(a["rows"]), a["rpi"], a["C"], a["heads"], a["L"], a["Lpad"], C.c_float(1e-5), None)
    return rc, a["out"]


@pytest.mark.parametrize("L, kind", [(77, "plain"), (33, "plain"), (77, "spike")])
def test_xattn_chain_source_against_float64(threaded, L, kind):
    """One 128-row tile through norm2 -> to_q -> attention -> to_out + x1 as the kernel's source computes it: the common context length
    (two full 32-key blocks and a ragged one), one key past a block boundary, and a score spike in the ragged block that forces the
    online softmax to re-base."""
    case = X.make_case(1, 128, L, seed=L, kind=kind, poison=(L == 33))
    rc, out = run(threaded, case)
    assert rc == 0, threaded.sdmi_last_error()
    X.assert_chain_parity(out, case)


def test_xattn_chain_source_second_image_and_refusals(threaded):
    """Two images of 128 rows with their own contexts: the second tile equals a launch of its own on the second image's operands.  And what
    the launcher refuses — each with its message, the sentinel-filled output untouched."""
    case = X.make_case(2, 128, 40, seed=5)
    rc, out = run(threaded, case)
    assert rc == 0, threaded.sdmi_last_error()
    one = dict(case, x=case["x"][128:].copy(), k=case["k"][1:].copy(), vt=case["vt"][1:].copy())
    rc, out1 = run(threaded, one)
    assert rc == 0, threaded.sdmi_last_error()
    np.testing.assert_array_equal(out1, out[128:])
    for over, msg in ((dict(C=640), "C = 320"), (dict(heads=5), "heads * 40"), (dict(rows=100), "rows % 128"), (dict(rpi=64), "rows_per_image % 128"),
                      (dict(L=0), "L >= 1"), (dict(wq=None), "null pointer"), (dict(k=None), "null pointer"), (dict(x=None), "null pointer")):
        sentinel = np.full_like(case["x"], 7.0)
        rc, o = run(threaded, case, out=sentinel, **over)
        assert rc != 0, over
        assert msg in threaded.sdmi_last_error().decode(), (over, threaded.sdmi_last_error())
        assert (o == 7.0).all(), over


def test_twin_passes_its_own_rule_on_every_gpu_case():
    """The yardstick of tests/test_gpu_xattn_chain.py is only usable if the fp16-storage twin itself satisfies the rule it sets — tensor, worst
    row, worst column, on the output and on the branch — for every case, the stress cases included."""
    for spec in X.GPU_CASES:
        case = X.make_case(**spec)
        twin = X.graph(case, twin=True)
        X.assert_chain_parity(twin, case, twin=twin)
        x = case["x"].astype(np.float64)
        ref = X.graph(case)
        ratio = np.sqrt(((ref - x) ** 2).mean() / (x ** 2).mean())
        if "lnstress" not in case["name"]:
            assert 0.3 < ratio < 3.0, (case["name"], ratio)            # the branch is comparable to the residual


def test_xattn_chain_code_object():
    """gfx950 code-object metadata of the kernel from the assembly the library build keeps: no private segment (scratch), no VGPR spills,
    at most 256 registers (two waves per SIMD: the 512-thread workgroup must be resident)."""
    path = os.path.join(ROOT, "stable-diffusion-webui_amd", "csrc", "build", "asm", "xattn_chain.s")
    if not os.path.exists(path):
        import subprocess
        subprocess.run(["bash", os.path.join(ROOT, "stable-diffusion-webui_amd", "csrc", "build.sh")], check=True)
    text = open(path).read()
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", text) if "rowchain_xattn_kernel" in b and ".vgpr_count" in b]
    assert len(blocks) == 1, len(blocks)
    field = lambda name: int(re.search(r"\.%s:\s+(\d+)" % name, blocks[0]).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 256
    assert field("group_segment_fixed_size") == 0                 # LDS is dynamic: 155 648 bytes set by the launcher
