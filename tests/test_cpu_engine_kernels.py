"""CPU tier of the engine-only helper kernels' tests: one run of tests/test_gpu_engine_kernels.py on the host-emulated library (the kernels'
own source run by tests/hostemu/hip/hip_runtime.h with the host's libm), so that every reference, bound and buffer size of
tests/engine_kernels_cases.py is proven before it meets a GPU.  The three cases past the grid cap (nchw_to_nhwc at 2^20 + 300 pixels, the
16 x 77 x 2048 context, the 2^20 + 257 element copies) run at their full size: each takes a few seconds emulated, none needs a smaller twin."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# small_linear (grid, strides and epilogues, knob, silu_in) and silu_f32 | timestep_embedding | nchw_to_nhwc | add_nchw_residual | ctx_compare and
# ctx_update_gated | hn_act | axpy_f16 | clip_embed and clip_pool | convert | refusals
GPU_FILE_CASES = (12 + 9 + 4 + 3 + 1) + 12 + (4 + 1 + 2 + 4) + 4 + (6 + 6) + (16 + 1) + 4 + (4 + 3) + 16 + 12


def test_gpu_engine_kernel_tests_pass_on_the_emulated_library(hostemu_lib):
    """Every case of tests/test_gpu_engine_kernels.py, none deselected or skipped."""
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_engine_kernels.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped|deselected)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == GPU_FILE_CASES, out[-2000:]
