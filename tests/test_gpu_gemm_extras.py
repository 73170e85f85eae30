"""GPU tests of the GEMM's engine-only epilogues, one launch at a time through the test entries sdmi_conv_gemm_ex, sdmi_groupnorm_ex,
sdmi_ln_rowstats and sdmi_ln_fold_weights (include/sdmi.h): GroupNorm statistics from the epilogue, LayerNorm row partials and the
LayerNorm fold, (hi, lo) stream tensors, bias_scale and gate.  The cases, their float64 references and their bounds are in
tests/gemm_extras_cases.py; tests/test_cpu_gemm_extras_cases.py runs the families the emulator's own entry reaches through the same
functions.  Every case prints one line with the family, the launch name and the measured figures (profiles/gemm_extras_accuracy.md)."""
import ctypes
import importlib
import json

import pytest
import torch

import gemm_extras_cases as cases
from test_gpu_abi import SCORE_FAMILIES, knobs

pytestmark = pytest.mark.gpu

MFMA_FAMILIES = [f for f in SCORE_FAMILIES if f not in ("generic", "mfma_reg")]


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


class extras_knobs(knobs):
    """test_gpu_abi.knobs, and gn_fuse back to its default on the way out as well."""

    def __exit__(self, *exc):
        super().__exit__(*exc)
        lib = sub("_lib")
        lib.check(lib.lib.sdmi_debug_set(b"gn_fuse", 1), "gn_fuse")


class GpuBackend:
    """tests/gemm_extras_cases.py's back end on the library's test entries."""

    def __init__(self, dev):
        self.lib = sub("_lib")
        self.L, self.dev = self.lib.lib, dev

    def stream(self):
        return self.lib.stream_ptr()

    def last_error(self):
        return self.lib.last_error()

    def knobs(self, kn):
        return extras_knobs(**kn)

    def conv_gemm(self, dref, x, stream):
        return self.L.sdmi_conv_gemm_ex(dref, ctypes.byref(x) if x is not None else None, stream)

    def _named(self, call):
        self.lib.check(self.L.sdmi_profile_begin(), "profile_begin")
        try:
            rc = call()
            torch.cuda.synchronize()
        finally:
            buf = ctypes.create_string_buffer(1 << 16)
            self.lib.check(self.L.sdmi_profile_end(buf, len(buf)), "profile_end")
        names = [k["name"] for k in json.loads(buf.value.decode())["kernels"]]
        return rc, names[0] if names else ""

    def groupnorm_ex(self, x0, x1, c0, c1, gamma, beta, out, B, HW, groups, eps, silu, ws, ws_bytes, pre_nchunk, x0_lo, x1_lo):
        p = self.lib.ptr
        return self._named(lambda: self.L.sdmi_groupnorm_ex(p(x0), p(x1), c0, c1, p(gamma), p(beta), p(out), B, HW, groups, eps, silu, p(ws), ws_bytes,
                                                            pre_nchunk, p(x0_lo), p(x1_lo), self.stream()))

    def ln_rowstats(self, x, stats, rows, C, eps):
        p = self.lib.ptr
        return self._named(lambda: self.L.sdmi_ln_rowstats(p(x), p(stats), rows, C, eps, self.stream()))

    def ln_fold_weights(self, w, gamma, beta, bias, wf, s_out, c_out, n_rows, K, C):
        p = self.lib.ptr
        return self._named(lambda: self.L.sdmi_ln_fold_weights(p(w), p(gamma), p(beta), p(bias), p(wf), p(s_out), p(c_out), n_rows, K, C, self.stream()))


@pytest.fixture(scope="module")
def be():
    sub("_lib").require_device()
    return GpuBackend(torch.device("cuda", 0))


@pytest.fixture(autouse=True)
def release_device_copies():
    yield
    torch.cuda.synchronize()
    cases.release()


# ---- a. GroupNorm statistics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cases.GN_FORMS)
@pytest.mark.parametrize("fam", MFMA_FAMILIES)
def test_groupnorm_statistics_epilogue(be, fam, form):
    cases.check_gn_stats(be, fam, form)


@pytest.mark.parametrize("form", cases.GN_FORMS)
@pytest.mark.parametrize("fam", cases.GN_WIDE_FAMILIES)
def test_groupnorm_statistics_epilogue_beyond_column_tile_0(be, fam, form):
    cases.check_gn_stats(be, fam, form, n=640)


@pytest.mark.parametrize("why", cases.GN_NOT_PRODUCED)
def test_groupnorm_statistics_not_produced(be, why):
    cases.check_gn_not_produced(be, why)


@pytest.mark.parametrize("ratio", cases.GN_OFFSET_RATIOS)
@pytest.mark.parametrize("fam", cases.GN_OFFSET_FAMILIES)
def test_groupnorm_from_device_written_statistics_on_offset_dominated_groups(be, fam, ratio):
    cases.check_gn_offsets(be, fam, ratio)


# ---- b. (hi, lo) stream tensors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(cases.HILO_CASES))
def test_hilo_stream_epilogues(be, label):
    cases.check_hilo(be, label)


@pytest.mark.parametrize("fam", MFMA_FAMILIES)
def test_hilo_statistics_form_on_every_family(be, fam):
    cases.check_hilo_stats(be, fam)


def test_hilo_refusals(be):
    cases.check_hilo_refusals(be)


# ---- c. LayerNorm row partials and fold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", SCORE_FAMILIES)
def test_layernorm_row_partials(be, fam):
    cases.check_lnp(be, fam)


LN_CASES = ([(f, "plain", "float64") for f in ("default", "5", "8", "7", "0", "2")] +
            [(f, "plain", s) for f in ("default", "5") for s in cases.LN_SOURCES[1:]] +
            [(f, "geglu", s) for f in ("default", "4", "0") for s in ("rowstats", "producer 9")] +
            [(f, "transposed", s) for f in ("default", "5", "7") for s in ("rowstats", "producer 8")])


@pytest.mark.parametrize("fam,form,source", LN_CASES, ids=[f"{f}-{m}-{s.replace(' ', '')}" for f, m, s in LN_CASES])
def test_layernorm_fold(be, fam, form, source):
    cases.check_ln_fold(be, fam, form, source)


@pytest.mark.parametrize("source", ["float64", "rowstats"])
@pytest.mark.parametrize("fam", ["default", "8", "7"])
def test_layernorm_fold_on_offset_heavy_rows(be, fam, source):
    cases.check_ln_fold(be, fam, "plain", source, heavy=True)


@pytest.mark.parametrize("fam,source", [("8", "rowstats"), ("0", "float64")])
def test_layernorm_fold_through_the_split_k_reduce(be, fam, source):
    cases.check_ln_fold(be, fam, "plain", source, C=1280, split=2)


def test_layernorm_fold_refusals(be):
    cases.check_ln_fold_refusals(be)


# ---- d. riders and the entry itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(cases.GATE_CASES))
def test_gate(be, label):
    cases.check_gate(be, label)


@pytest.mark.parametrize("fam", ["default", "5", "0", "generic"])
def test_bias_scale(be, fam):
    cases.check_bias_scale(be, fam)


@pytest.mark.parametrize("fam", ["default", "5", "12", "generic"])
def test_null_extras_is_sdmi_conv_gemm(be, fam):
    cases.check_null_extras(be, fam)


def test_conv_gemm_ex_refusals(be):
    cases.check_refusals(be)
