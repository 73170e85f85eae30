"""CPU tier of the level-0 self-attention form 27 (csrc/attention.hip): the kernel's own source on the host-emulated library on the
shapes of tests/test_gpu_attn_l0_forms.py, the stand-alone sanitizer driver built and run as a program, and the gfx950 loop of form 27
read from the assembly the library build keeps."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import attn_l0_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stable-diffusion-webui_amd", "csrc")


@pytest.fixture(scope="module")
def threaded(hostemu_lib):
    """The host-emulated library with every thread of the running block a fiber (real barriers, MFMA builtins emulated)."""
    lib = C.CDLL(hostemu_lib)
    lib.sdmi_last_error.restype = C.c_char_p
    lib.emu_set_threaded(1)
    yield lib
    lib.emu_set_threaded(0)


def run(lib, case, form, prescaled=False):
    qn, kn = (case["qs16"], case["ks16"]) if prescaled else (case["q16"], case["k16"])
    out = np.zeros((case["B"], case["N"], case["H"] * R.D), np.float16)
    ld = qn.strides[1] // 2
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib.sdmi_attention_vt_ex(p(qn), p(kn), p(case["vt16"]), p(out), case["B"], case["H"], case["N"], case["M"], R.D, ld, ld,
                                  case["vt16"].shape[2], out.shape[2], C.c_float(R.D ** -0.5), int(prescaled), form, 0, None)
    return rc, out


# the GPU test's shapes (attn_l0_reference.SHAPES): B = 1, H = 2 dense and B = 2, H = 8 stacked as the engine lays q | k out (row stride 640,
# batch stride, the eight-head XCD remap of the workgroup ids) at 16 tiles, 17 tiles and 16 tiles + 40 keys
EMU_SHAPES = R.SHAPES


@pytest.mark.parametrize("name, B, H, N, stacked", EMU_SHAPES, ids=[s[0] for s in EMU_SHAPES])
def test_form_27_source_on_the_emulated_library(threaded, name, B, H, N, stacked):
    """16 and 17 KV tiles and a ragged last tile (40 keys) behind 16 full ones, dense and stacked q | k: form 27 gives the bits of
    form 17 on the same pre-scaled operands (same arithmetic; only the staging addresses differ), holds the attention cap against float64
    and 1.1 x form 17's error on the unscaled twins."""
    case = R.make_case(B, H, N, stacked, seed=N)
    assert not stacked or case["qs16"].strides[1] // 2 == 2 * H * R.D
    outs = {}
    for key, form, pre in ((17, 17, False), (27, 27, True), ("17s", 17, True)):
        rc, outs[key] = run(threaded, case, form, pre)
        assert rc == 0, threaded.sdmi_last_error()
    assert np.array_equal(outs[27].view(np.uint16), outs["17s"].view(np.uint16))
    e17, e27 = R.rel_l2(outs[17], case["ref"]), R.rel_l2(outs[27], case["ref_s"])
    print(f"[attn_l0 emulated] {name}: form 17 {e17:.3e} form 27 {e27:.3e} ratio {e27 / e17:.3f}")
    assert e17 < R.ATTN_CAP and e27 < R.ATTN_CAP and e27 <= 1.1 * e17, (e17, e27)
    assert R.worst_row_rel_l2(outs[27], case["ref_s"])[0] < 2 * R.ATTN_CAP


def test_form_27_refuses_unscaled_operands_and_default_dispatch(threaded):
    case = R.make_case(1, 1, 1024, False, seed=3)
    rc, _ = run(threaded, case, 27, prescaled=False)
    assert rc != 0 and b"pre-scaled" in threaded.sdmi_last_error()
    rc, o27 = run(threaded, case, 27, prescaled=True)
    assert rc == 0
    rc, dflt = run(threaded, case, 0, prescaled=True)
    assert rc == 0 and np.array_equal(dflt.view(np.uint16), o27.view(np.uint16))
    # 27 forced for the whole process (knob attn_occ): launches that are not pre-scaled run form 17, pre-scaled ones form 27
    rc, o17 = run(threaded, case, 17)
    assert rc == 0 and threaded.sdmi_debug_set(b"attn_occ", 27) == 0
    try:
        rc, forced = run(threaded, case, 0)
        assert rc == 0 and np.array_equal(forced.view(np.uint16), o17.view(np.uint16))
        rc, forced = run(threaded, case, 0, prescaled=True)
        assert rc == 0 and np.array_equal(forced.view(np.uint16), o27.view(np.uint16))
    finally:
        assert threaded.sdmi_debug_set(b"attn_occ", 15) == 0


def test_sanitizer_driver_runs_clean():
    """(CPU tier only: where a GPU is present the program is not built or started.)
    tools/micro/attn_l0_asan_driver.cpp: a program of its own (never loaded into Python) against an AddressSanitizer build of the
    host-emulated library, form 27 on ragged key counts with q | k and V^T in exactly sized heap allocations — a read past the last
    key row is a report and a non-zero exit."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("the sanitizer driver belongs to the CPU tier: not run on a machine with a GPU")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hostemu import build as hb
    cxx = hb.compiler()
    if not cxx or os.uname().machine != "x86_64":
        pytest.skip("needs clang++ on x86-64")
    built = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostemu", "build.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(os.environ, SDMI_HOSTEMU_ASAN="1"), timeout=1200)
    lib = built.stdout.decode().strip().splitlines()[-1]
    assert built.returncode == 0 and os.path.exists(lib), built.stdout.decode()[-4000:]
    rt = subprocess.run([cxx, "-print-file-name=libclang_rt.asan-x86_64.so"], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    work = tempfile.mkdtemp(prefix="sdmi_attn_l0_asan_")
    try:
        exe = os.path.join(work, "attn_l0_asan_driver")
        cmd = [cxx, "-std=c++17", "-O1", "-g1", "-fsanitize=address", "-shared-libasan", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "micro", "attn_l0_asan_driver.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
               "-Wl,-rpath," + os.path.dirname(rt), "-o", exe]
        b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert b.returncode == 0, b.stdout.decode()[-4000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout.decode()[-4000:]
        assert b"attn_l0_asan_driver: ok" in r.stdout and b"AddressSanitizer" not in r.stdout, r.stdout.decode()[-2000:]
    finally:
        shutil.rmtree(work, ignore_errors=True)


# ---- gfx950 code of form 27 ------------------------------------------------------------------------------------------------------
def _assembly():
    path = os.path.join(CSRC, "build", "asm", "attention.s")
    if not os.path.exists(path):
        subprocess.run(["bash", os.path.join(CSRC, "build.sh")], check=True)
    return open(path).read()


def _kernel(text, var):
    m = re.search(r"^(_ZN4sdmi16attn_mfma_kernelILi40ELi64ELi%dEEEvNS_5AttnPE):[^\n]*\n(.*?)\.Lfunc_end" % var, text, re.S | re.M)
    assert m, f"attn_mfma_kernel<40, 64, {var}> not in the assembly"
    return m.group(1), m.group(2)


def _meta(text, kname):
    blocks = [b for b in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+%s\s" % kname, b)]
    assert len(blocks) == 1
    return lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, blocks[0]).group(1))


def _loop_blocks(body):
    """Basic blocks (label, Counter of mnemonics) of the innermost loop: from the block the compiler marks as the inner loop header to the
    last block that branches back to it."""
    blocks = []
    for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body):
        label = b.split(":", 1)[0]
        lines = [x.split(";")[0].strip() for x in b.split("\n")]
        ops = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
        blocks.append((label, b, collections.Counter(o.split()[0] for o in ops), ops))
    loops = []
    for head, (label, raw, _, _) in enumerate(blocks):
        if "Loop Header" not in "\n".join(raw.split("\n")[:3]):
            continue
        back = [i for i, (_, _, _, ops) in enumerate(blocks) if i >= head and any(re.match(r"s_c?branch\w*\s+%s$" % re.escape(label), o) for o in ops)]
        if back and any(o.startswith("v_mfma") for b in blocks[head:back[-1] + 1] for o in b[2]):
            loops.append(blocks[head:back[-1] + 1])
    assert len(loops) == 1, f"{len(loops)} loops with MFMAs: the KV loop was copied"
    return loops[0]


def test_form_27_steady_state_loop():
    """One copy of the KV loop; its steady-state body — every block but the one that stages a ragged last tile, which only the
    block-uniform `t + 1 >= nfull` branch reaches — holds 14 MFMAs, 4 staging loads addressed by a scalar base and a 32-bit offset, no
    packed fp32 multiply / FMA in front of exp2 and no clamp or 64-bit row product.  The whole kernel: no scratch, no spills, and within
    the 168 VGPRs that keep three workgroups on a CU (form 17's budget)."""
    text = _assembly()
    kname, body = _kernel(text, 27)
    field = _meta(text, kname)
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("vgpr_count") <= 168, field("vgpr_count")
    assert _meta(text, _kernel(text, 17)[0])("vgpr_count") <= 168
    loop = _loop_blocks(body)
    ragged = [b for b in loop if b[2]["v_min_i32"] or b[2]["v_mad_i64_i32"]]
    assert len(ragged) == 1 and sum(v for o, v in ragged[0][2].items() if o.startswith("v_mfma")) == 0
    assert ragged[0][2]["global_load_dwordx4"] == 4
    # the re-basing block (wave-uniform branch, taken when a tile's maximum exceeds the shift by more than tau: once per row with the default
    # slack) subtracts delta from the 32 scores and multiplies the 32 O accumulators by alpha: its 16 packed multiplies are form 17's too
    rebase = [b for b in loop if b[2]["v_sub_f32_e32"] >= 32]
    assert len(rebase) == 1 and sum(v for o, v in rebase[0][2].items() if o.startswith("v_mfma")) == 0 and rebase[0][2]["v_exp_f32_e32"] <= 1
    steady = collections.Counter()
    for b in loop:
        if b is not ragged[0] and b is not rebase[0]:
            steady.update(b[2])
    assert sum(v for o, v in steady.items() if o.startswith("v_mfma_f32_32x32x16")) == 14, steady
    assert steady["v_pk_mul_f32"] == 0 and steady["v_pk_fma_f32"] == 0, steady
    assert steady["v_mad_i64_i32"] == 0 and steady["v_min_i32"] == 0
    assert steady["global_load_dwordx4"] == 4 and steady["v_lshl_add_u64"] == 0, steady
    assert steady["v_exp_f32_e32"] == 32 and steady["ds_read_b128"] == 14, steady
    assert steady["s_barrier"] == 1
