"""CPU tier of the op-level C ABI tests: one run of tests/test_gpu_abi.py on the host-emulated library, and the ratchet that keeps every
op-level entry of include/sdmi.h under a direct GPU test."""
import glob
import importlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases of tests/test_gpu_abi.py: sampler updates, CFG, weight deltas and slerp | attention | rowchain | refusals
# | sdmi_conv_gemm from raw descriptors: batched scores, shared A, split-K (+ the broadcast residual), 3x3 with strided sources, GEGLU /
#   transposed / NCHW stores, wide against narrow epilogue, alpha, the misaligned batch stride, refusals; sdmi_pack_conv_weight
GPU_FILE_CASES = ((8 + 8 + 16 + 12 + 3) + (6 + 3 + 9 + 3) + (4 + 2 + 2 + 2 + 9 + 2) + (4 + 3 + 2 + 2 + 1 + 1 + 1) + (12 + 1) + 2 +
                  (18 + 4 + 12 + 1 + 22 + 3 + 3 + 2 + 4 + 2 + 1 + 1) + 8)


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


def test_gpu_abi_tests_pass_on_the_emulated_library(hostemu_lib):
    """Every case of tests/test_gpu_abi.py, none deselected (the N = 4168 wide-attention case takes a few seconds emulated)."""
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_abi.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped|deselected)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= GPU_FILE_CASES, out[-2000:]


# entries that are not ops on tensors: library / device queries, handles (engine, UNet, VAE, CLIP, upscaler networks), knobs, the profiler
NOT_OP_LEVEL = re.compile(r"^sdmi_(version|last_error|device_ok|engine_|unet_|vae_|clip_|esrgan_|compact_(blob_floats|create|destroy|scratch_bytes|run)$"
                          r"|debug_set|profile_|bench_conv_gemm)")


def wrappers_by_entry():
    """{sdmi_x: the top-level functions of ops.py / rng.py whose body calls lib.sdmi_x}, from the modules' text."""
    found = {}
    for mod in ("ops", "rng"):
        text = open(os.path.join(ROOT, "stable-diffusion-webui_amd", mod + ".py")).read()
        for block in re.split(r"^(?=def )", text, flags=re.M)[1:]:
            name = re.match(r"def (\w+)\(", block).group(1)
            for entry in set(re.findall(r"\blib\.(sdmi_\w+)\(", block)):
                found.setdefault(entry, set()).add(name)
    return found


def test_every_op_level_entry_has_a_direct_gpu_test():
    lib = sub("_lib")
    op_level = sorted(n for n in lib._SIGS if not NOT_OP_LEVEL.match(n))
    assert 85 <= len(op_level) < len(lib._SIGS) and "sdmi_attention_vt" in op_level and "sdmi_unet_forward" not in op_level
    tests = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))))
    wrappers = wrappers_by_entry()
    assert wrappers["sdmi_attention_vt"] == {"attention_vt"} and "slerp" in wrappers["sdmi_slerp"]
    # a call (`L.sdmi_x(` / `ops.wrapper(`), not a mention: a name in a comment, a docstring or a message does not count
    missing = [n for n in op_level
               if not re.search(r"\." + n + r"\(", tests) and not any(re.search(r"\." + w + r"\(", tests) for w in wrappers.get(n, ()))]
    assert not missing, f"op-level entries of include/sdmi.h that no tests/test_gpu_*.py calls, by name or through its ops / rng wrapper: {missing}"
