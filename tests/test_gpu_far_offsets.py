"""GPU tests of the kernels' address arithmetic where element offsets pass 2^31 and byte offsets pass 2^32, and of both sides of the
host-side guards that keep 32-bit (and narrower) index arithmetic legal.  The method and the argument why a wrong address cannot leave
the allocation: tests/far_buffers.py; the cases, their references and pass rules (all taken from the entries' own GPU files):
tests/far_offset_cases.py.  Every case that the host emulation can hold also runs on the emulated library (tests/test_cpu_far_offsets.py);
the measured figures are in profiles/far_offsets.md."""
import importlib

import pytest
import torch

import far_offset_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    importlib.import_module("stable-diffusion-webui_amd._lib").require_device()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def abi(dev):
    lib = importlib.import_module("stable-diffusion-webui_amd._lib")
    return lib.lib, lib.check, lib.ptr, lib.stream_ptr


@pytest.fixture(autouse=True)
def release_device_copies():
    yield
    C.release()


def ids(cases):
    return ["-".join(str(x) for x in c) if isinstance(c, tuple) else str(c) for c in cases]


# ---- operands at far offsets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps,fam,far", C.CONV_LD_CASES, ids=ids(C.CONV_LD_CASES))
def test_conv_gemm_far_row_stride(dev, abi, taps, fam, far):
    C.check_conv_ld(abi, dev, taps, fam, far)


@pytest.mark.parametrize("flag,fam", C.CONV_FLAG_CASES, ids=ids(C.CONV_FLAG_CASES))
def test_conv_gemm_far_output_in_the_other_store_forms(dev, abi, flag, fam):
    C.check_conv_flags(abi, dev, flag, fam)


@pytest.mark.parametrize("taps,fam,far", C.CONV_BS_CASES, ids=ids(C.CONV_BS_CASES))
def test_conv_gemm_far_batch_stride(dev, abi, taps, fam, far):
    C.check_conv_bs(abi, dev, taps, fam, far)


@pytest.mark.parametrize("cfg,split", C.CONV_SPLIT_CASES, ids=ids(C.CONV_SPLIT_CASES))
def test_conv_gemm_split_k_reduces_into_far_rows(dev, abi, cfg, split):
    C.check_conv_splitk(abi, dev, cfg, split)


@pytest.mark.parametrize("fam,far", C.HILO_CASES, ids=ids(C.HILO_CASES))
def test_conv_gemm_ex_far_hi_lo_pairs(dev, abi, fam, far):
    C.check_conv_hilo(abi, dev, fam, far)


@pytest.mark.parametrize("d,m,far,form", C.ATTN_VT_CASES, ids=ids(C.ATTN_VT_CASES))
def test_attention_vt_far_operands(dev, abi, d, m, far, form):
    C.check_attention_vt(abi, dev, d, m, far, form)


@pytest.mark.parametrize("d,m", C.ATTN_V_CASES, ids=ids(C.ATTN_V_CASES))
def test_attention_transposes_far_rows_of_v(dev, abi, d, m):
    C.check_attention_row_major_v(abi, dev, d, m)


@pytest.mark.parametrize("m,far", C.ATTN_WIDE_CASES, ids=ids(C.ATTN_WIDE_CASES))
def test_attention_wide_far_operands(dev, abi, m, far):
    C.check_attention_wide(abi, dev, m, far)


@pytest.mark.parametrize("form", C.LN_CASES)
def test_swin_layernorm_far_rows(dev, abi, form):
    C.check_swin_layernorm(abi, dev, form)


@pytest.mark.parametrize("far,ep,up", C.RRDB_CASES, ids=ids(C.RRDB_CASES))
def test_rrdb_conv_far_rows(dev, abi, far, ep, up):
    C.check_rrdb_conv(abi, dev, far, ep, up)


@pytest.mark.parametrize("far", C.COMPACT_CASES)
def test_compact_conv_far_rows(dev, abi, far):
    C.check_compact_conv(abi, dev, far)


@pytest.mark.parametrize("kind,far,shift", C.SWIN_CASES, ids=ids(C.SWIN_CASES))
def test_swin_window_attention_far_token_rows(dev, abi, kind, far, shift):
    C.check_swin_attention(abi, dev, kind, far, shift)


@pytest.mark.parametrize("far", C.HAT_CAB_CASES)
def test_hat_cab_add_and_channel_gate_far_rows(dev, abi, far):
    C.check_hat_cab(abi, dev, far)


@pytest.mark.parametrize("kind,far", C.WIN16_CASES, ids=ids(C.WIN16_CASES))
def test_window_16_attention_far_token_rows(dev, abi, kind, far):
    C.check_window16(abi, dev, kind, far)


@pytest.mark.parametrize("far,shift", C.SCU_CASES, ids=ids(C.SCU_CASES))
def test_scu_block_far_rows(dev, abi, far, shift):
    C.check_scu_block(abi, dev, far, shift)


@pytest.mark.parametrize("which", C.DAT_ROW_CASES)
def test_dat_row_kernels_far_rows(dev, abi, which):
    C.check_dat_rows(abi, dev, which)


# ---- dense tensors at the limits the norm launchers state (too large for the host emulation) ---------------------------------------------------
@pytest.mark.parametrize("name", list(C.GN_LIMITS), ids=[n.replace(" ", "_") for n in C.GN_LIMITS])
def test_groupnorm_at_its_row_and_element_limits(dev, abi, name):
    C.check_groupnorm_limit(abi, dev, name)


@pytest.mark.parametrize("entry", ["layernorm", "ln_rowstats"])
def test_layernorm_past_2_31_elements(dev, abi, entry):
    C.check_layernorm_limit(abi, dev, entry)


# ---- both sides of the dispatch guards --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,name,side", C.PP_GUARD_CASES, ids=ids(C.PP_GUARD_CASES))
def test_pingpong_3x3_guard_both_sides(dev, abi, cfg, name, side):
    C.check_pingpong_guard(abi, dev, cfg, name, side)


@pytest.mark.parametrize("which", C.FORM27_CASES)
def test_attention_form_27_at_the_staging_limits(dev, abi, which):
    C.check_form27_limits(abi, dev, which)
