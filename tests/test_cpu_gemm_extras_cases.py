"""CPU tier of tests/gemm_extras_cases.py: a subset of the cases of tests/test_gpu_gemm_extras.py through the host emulator's own entries
(emu_conv_gemm, emu_groupnorm_hilo, emu_ln_rowstats), on the tile families that entry reaches with its (cfg, split, korder) arguments —
the heuristic one, 64x64, 128x64, 128x128, 128x320, 256x256 and 256x320 — so that the references, the buffer sizes and the bounds are
proven on a CPU before they meet a GPU.  What needs the library's own entry or a knob emu_conv_gemm does not take (the refusals of
sdmi_conv_gemm_ex, gate, gn_fuse, the two-stage forms) runs in the GPU file only."""
import contextlib
import ctypes as C

import pytest
import torch

import gemm_extras_cases as cases

KORDER_DEFAULT = 2                            # csrc/gemm.hip g_conv_korder_default


class EmuBackend:
    def __init__(self, path):
        self.L = C.CDLL(path)
        for name in ("sdmi_conv_splitk_workspace_bytes", "sdmi_groupnorm_workspace_bytes"):
            getattr(self.L, name).restype = C.c_int64
        self.L.emu_last_error.restype = self.L.emu_last_launch.restype = C.c_char_p
        self.dev = torch.device("cpu")
        self.kn = {}

    def stream(self):
        return None

    def last_error(self):
        return (self.L.emu_last_error() or b"").decode()

    @contextlib.contextmanager
    def knobs(self, kn):
        assert set(kn) <= {"gemm_cfg", "gemm_split", "conv_korder"}, ("emu_conv_gemm takes no such knob", kn)
        self.kn = kn
        try:
            yield
        finally:
            self.kn = {}

    def conv_gemm(self, dref, x, stream):
        korder = self.kn.get("conv_korder", -1)
        return self.L.emu_conv_gemm(dref, self.kn.get("gemm_cfg", -1), self.kn.get("gemm_split", 0), KORDER_DEFAULT if korder < 0 else korder,
                                    C.byref(x) if x is not None else None)

    def _named(self, rc):
        return rc, (self.L.emu_last_launch() or b"").decode()

    @staticmethod
    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def groupnorm_ex(self, x0, x1, c0, c1, gamma, beta, out, B, HW, groups, eps, silu, ws, ws_bytes, pre_nchunk, x0_lo, x1_lo):
        p = self.p
        return self._named(self.L.emu_groupnorm_hilo(p(x0), p(x1), c0, c1, p(gamma), p(beta), p(out), B, HW, groups, C.c_float(eps), silu, p(ws), pre_nchunk,
                                                     p(x0_lo), p(x1_lo)))

    def ln_rowstats(self, x, stats, rows, Cn, eps):
        return self._named(self.L.emu_ln_rowstats(self.p(x), self.p(stats), C.c_int64(rows), Cn, C.c_float(eps)))

    def ln_fold_weights(self, w, gamma, beta, bias, wf, s_out, c_out, n_rows, K, Cn):
        p = self.p
        return self.L.sdmi_ln_fold_weights(p(w), p(gamma), p(beta), p(bias), p(wf), p(s_out), p(c_out), n_rows, K, Cn, None), "ln_fold_weights"


@pytest.fixture(scope="module")
def be(hostemu_lib):
    return EmuBackend(hostemu_lib)


@pytest.fixture(autouse=True)
def threaded_and_released(be, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)     # (launch_gemm synchronises after its call; here the call has run on return)
    be.L.emu_set_threaded(1)
    yield
    be.L.emu_set_threaded(0)
    cases.release()


@pytest.mark.parametrize("fam,form", [("default", "3x3 residual"), ("8", "3x3 residual"), ("5", "1x1 rowbias"), ("7", "1x1 rowbias"), ("4", "3x3 ldo N + 4"),
                                      ("2", "3x3 ldo N + 4")])
def test_groupnorm_statistics_epilogue(be, fam, form):
    cases.check_gn_stats(be, fam, form)


@pytest.mark.parametrize("fam,form", [("8", "3x3 residual"), ("5", "1x1 rowbias")])
def test_groupnorm_statistics_epilogue_beyond_column_tile_0(be, fam, form):
    cases.check_gn_stats(be, fam, form, n=640)


@pytest.mark.parametrize("why", ["generic", "15 x 16", "split-K"])
def test_groupnorm_statistics_not_produced(be, why):
    cases.check_gn_not_produced(be, why)


@pytest.mark.parametrize("fam,ratio", [("8", 300.0), ("0", 30.0)])
def test_groupnorm_from_epilogue_statistics_on_offset_dominated_groups(be, fam, ratio):
    cases.check_gn_offsets(be, fam, ratio)


@pytest.mark.parametrize("label", ["dx 128x320 stats", "split-K x2", "output pair only", "out_lo 8 bytes off", "ldo N + 8", "dx 128x320 stats N 640"])
def test_hilo_stream_epilogues(be, label):
    cases.check_hilo(be, label)


@pytest.mark.parametrize("fam", ["2", "5", "4"])
def test_hilo_statistics_form(be, fam):
    cases.check_hilo_stats(be, fam)


@pytest.mark.parametrize("fam", ["default", "2", "7", "8", "5", "generic"])
def test_layernorm_row_partials(be, fam):
    cases.check_lnp(be, fam)


@pytest.mark.parametrize("fam,form,source", [("default", "plain", "float64"), ("5", "plain", "producer 8"), ("0", "geglu", "rowstats"),
                                             ("7", "transposed", "rowstats")])
def test_layernorm_fold(be, fam, form, source):
    cases.check_ln_fold(be, fam, form, source)


def test_layernorm_fold_on_offset_heavy_rows(be):
    cases.check_ln_fold(be, "8", "plain", "rowstats", heavy=True)


def test_layernorm_fold_through_the_split_k_reduce(be):
    cases.check_ln_fold(be, "0", "plain", "float64", C=1280, split=2)


@pytest.mark.parametrize("fam", ["5", "generic"])
def test_bias_scale(be, fam):
    cases.check_bias_scale(be, fam)
