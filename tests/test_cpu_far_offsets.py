"""CPU tier of the far-offset tests: one run of tests/test_gpu_far_offsets.py on the host-emulated library (the kernels' own source run by
tests/hostemu/hip/hip_runtime.h), where a far buffer is an anonymous mapping whose untouched pages cost nothing (tests/far_buffers.py).
An index that is one cast short reads or writes the wrong host memory here exactly as it would on the device, so this tier finds such a
bug without touching a GPU; what it cannot see is the GPU builds' own address forms (LDS-direct loads, buffer offsets folded by the
compiler).

What this tier does NOT see, measured with mutants of the kernels: a dropped `(long)` in a product of two ints that is then added to a
pointer or a long — `(long)ms * p.ldo` of the GEMM's epilogue store, `((long)b * p.N + q) * p.ldq` of the attention kernels.  Signed
overflow being undefined, the host compiler computes such a product in 64 bits and the mutant gives the right answer here.  (Written
with defined 32-bit wrap, the same mutants fail 28 and 12 cases.)  For these forms only the GPU run of the file is evidence: do not
take a green run of this tier for them.

Not run here, by name:
  * test_groupnorm_at_its_row_and_element_limits and test_layernorm_past_2_31_elements (every case): dense tensors of 2^31 elements,
    which the emulation cannot stream in a test's time;
  * test_pingpong_3x3_guard_both_sides, the cases "rows", "columns", "rows-up", "columns-up" (both sides, gemm_cfg 4 / 5 / 8): 32 000
    output rows of a 3x3 convolution take 14 - 21 s each emulated (measured; all 24 pass).  The image-count guard ("images") runs."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# conv_gemm: far row stride, other stores, far batch stride, split-K, (hi, lo) pairs | attention: vt, row-major V, wide | swin layernorm |
# rrdb, compact, swin / swin2 attention, hat cab_add and channel gate, window-16 attention, scu_block, DAT row kernels | ping-pong guard,
# images only | form 27
RUN_HERE = (144 + 11 + 24 + 3 + 4) + (62 + 12 + 8) + 3 + (7 + 3 + 8 + 4 + 10 + 6 + 8) + 6 + 2
NOT_HERE = "test_groupnorm_at_its_row_and_element_limits or test_layernorm_past_2_31_elements or (test_pingpong_3x3_guard_both_sides and (rows or columns))"


def test_gpu_far_offset_tests_pass_on_the_emulated_library(hostemu_lib):
    env = dict(os.environ, SDMI_HOSTEMU="1", SDMI_LIB=hostemu_lib)
    env.pop("PYTEST_CURRENT_TEST", None)
    env.pop("SDMI_HOSTEMU_SELECT", None)
    workers = str(max(1, min(8, os.cpu_count() or 1)))
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_far_offsets.py", "-m", "gpu", "-q", "-p", "no:cacheprovider", "-n", workers,
           "-k", f"not ({NOT_HERE})", "--timeout=300", "--timeout-method=thread"]
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-6000:]
    assert not re.search(r"\d+ (failed|error|skipped)", out), out[-6000:]
    m = re.search(r"(\d+) passed", out)
    assert m and int(m.group(1)) == RUN_HERE, out[-2000:]                # the file has RUN_HERE + 6 + 2 + 24 cases
