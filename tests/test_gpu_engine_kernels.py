"""GPU tests of the elementwise helpers only the engine launches (csrc/elementwise.hip), one launch at a time through the test entries
sdmi_small_linear, sdmi_silu_f32, sdmi_timestep_embedding, sdmi_nchw_to_nhwc, sdmi_add_nchw_residual, sdmi_ctx_compare, sdmi_ctx_update_gated,
sdmi_hn_act, sdmi_axpy_f16, sdmi_clip_embed, sdmi_clip_pool and sdmi_convert (include/sdmi.h).  The cases, their references and their bounds
are in tests/engine_kernels_cases.py; tests/test_cpu_engine_kernels.py runs this file on the host-emulated library.  Every case prints one
line with the measured figure and its cap (profiles/engine_kernels_accuracy.md)."""
import importlib

import numpy as np
import pytest
import torch

import engine_kernels_cases as cases

pytestmark = pytest.mark.gpu

DTYPES = [np.float16, np.float32]
DTYPE_IDS = ["f16", "f32"]


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


class Backend:
    """tests/engine_kernels_cases.py's back end on the library's test entries.  The calls stand here, by name, because the ratchet of
    tests/test_cpu_abi.py looks for them in tests/test_gpu_*.py."""

    def __init__(self, dev):
        self.lib, self.dev = sub("_lib"), dev
        self.L, self.ptr, self.sp = self.lib.lib, self.lib.ptr, self.lib.stream_ptr

    def last_error(self):
        return self.lib.last_error()

    def knob(self, name, value):
        self.lib.check(self.L.sdmi_debug_set(name.encode(), value), name)

    def small_linear(self, *args):
        return self.L.sdmi_small_linear(*args)

    def silu_f32(self, *args):
        return self.L.sdmi_silu_f32(*args)

    def timestep_embedding(self, *args):
        return self.L.sdmi_timestep_embedding(*args)

    def nchw_to_nhwc(self, *args):
        return self.L.sdmi_nchw_to_nhwc(*args)

    def add_nchw_residual(self, *args):
        return self.L.sdmi_add_nchw_residual(*args)

    def ctx_compare(self, *args):
        return self.L.sdmi_ctx_compare(*args)

    def ctx_update_gated(self, *args):
        return self.L.sdmi_ctx_update_gated(*args)

    def hn_act(self, *args):
        return self.L.sdmi_hn_act(*args)

    def axpy_f16(self, *args):
        return self.L.sdmi_axpy_f16(*args)

    def clip_embed(self, *args):
        return self.L.sdmi_clip_embed(*args)

    def clip_pool(self, *args):
        return self.L.sdmi_clip_pool(*args)

    def convert(self, *args):
        return self.L.sdmi_convert(*args)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def abi(dev):
    return Backend(dev)


@pytest.fixture(autouse=True)
def release_device_copies():
    yield
    torch.cuda.synchronize()
    cases.release()


# ---- small_linear, silu_f32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", cases.SMALL_LINEAR_GRID, ids=[f"B{b}-N{n}-K{k}" for b, n, k in cases.SMALL_LINEAR_GRID])
def test_small_linear_vs_float64(abi, B, N, K):
    cases.check_small_linear(abi, B, N, K)


@pytest.mark.parametrize("form", list(cases.SMALL_LINEAR_FORMS))
def test_small_linear_strides_and_epilogues_vs_float64(abi, form):
    B, N, K, opt = cases.SMALL_LINEAR_FORMS[form]
    cases.check_small_linear(abi, B, N, K, seed=120, label=f"{form} B {B} N {N} K {K}", **opt)


@pytest.mark.parametrize("B,N,K", cases.KNOB_SHAPES, ids=[f"B{b}-N{n}-K{k}" for b, n, k in cases.KNOB_SHAPES])
def test_small_linear_lds_knob_changes_no_bits(abi, B, N, K):
    cases.check_small_linear_knob(abi, B, N, K)


@pytest.mark.parametrize("B,N,K", [(4, 256, 320), (16, 258, 520), (17, 255, 1280)], ids=["lds4", "lds16", "plain"])
def test_small_linear_silu_in_is_silu_f32_then_the_product(abi, B, N, K):
    cases.check_small_linear_silu_in(abi, B, N, K)


def test_silu_f32_vs_float64(abi):
    cases.check_silu_f32(abi)


# ---- timestep_embedding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dim", cases.TE_SHAPES, ids=[f"B{b}-dim{d}" for b, d in cases.TE_SHAPES])
def test_timestep_embedding_vs_float64(abi, B, dim):
    cases.check_timestep_embedding(abi, B, dim)


# ---- nchw_to_nhwc ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, cases.VAE_SCALE], ids=["scale1", "vae-scale"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nchw_to_nhwc_is_one_multiply_and_a_cast(abi, dtype, scale):
    cases.check_nchw_plain(abi, dtype, scale)


def test_nchw_to_nhwc_past_the_grid_cap(abi):
    cases.check_nchw_past_the_grid_cap(abi)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nchw_to_nhwc_lo_channels(abi, dtype):
    cases.check_nchw_lo(abi, dtype)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nchw_to_nhwc_channel_mix_vs_float64(abi, dtype, with_bias):
    cases.check_nchw_mix(abi, dtype, with_bias)


# ---- add_nchw_residual -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hilo", [False, True], ids=["plain", "hilo"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_add_nchw_residual_is_the_float32_sequence(abi, dtype, hilo):
    cases.check_add_nchw_residual(abi, dtype, hilo)


# ---- ctx_compare / ctx_update_gated ----------------------------------------------------------------------------------------------------------
CTX_IDS = ["x".join(map(str, g)) for g in cases.CTX_GEOMS]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("geom", cases.CTX_GEOMS, ids=CTX_IDS)
def test_ctx_compare_sees_every_changed_element(abi, geom, dtype):
    cases.check_ctx_compare(abi, *geom, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("geom", cases.CTX_GEOMS, ids=CTX_IDS)
def test_ctx_update_gated(abi, geom, dtype):
    cases.check_ctx_update_gated(abi, *geom, dtype)


# ---- hn_act / axpy_f16 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(cases.HN_ACTS), ids=[f"{k}-{cases.HN_NAMES[k]}" for k in cases.HN_ACTS])
def test_hn_act_over_every_finite_half_vs_float64(abi, kind):
    cases.check_hn_act(abi, kind)


def test_hn_act_on_infinities_and_nan(abi):
    cases.check_hn_act_non_finite(abi)


@pytest.mark.parametrize("n", cases.SIZES)
def test_axpy_f16_is_two_float32_roundings(abi, n):
    cases.check_axpy_f16(abi, n)


# ---- clip_embed / clip_pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("embeds", [False, True], ids=["tokens", "inputs_embeds"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_clip_embed(abi, dtype, embeds):
    cases.check_clip_embed(abi, dtype, embeds)


@pytest.mark.parametrize("C", [64, 300, 1280])
def test_clip_pool(abi, C):
    cases.check_clip_pool(abi, C)


# ---- convert ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("dst", DTYPES, ids=["to-f16", "to-f32"])
@pytest.mark.parametrize("src", DTYPES, ids=DTYPE_IDS)
def test_convert(abi, src, dst, n):
    cases.check_convert(abi, src, dst, n)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", cases.ENTRIES)
def test_refusals(abi, entry):
    cases.check_refusals(abi, entry)
