"""The level-0 self-attention forms of csrc/attention.hip on the GPU, through sdmi_attention_vt_ex (ops.attention_vt_ex):
form 27 (q and k pre-scaled by sqrt(scale * log2 e): no scale multiply in the kernel, staging addresses out of the KV loop) must give the
bits of form 17 on the same pre-scaled operands, and is held to float64 by form 17's own error on the unscaled twins of the same case.
Cases and references: tests/attn_l0_reference.py (computed once per module)."""
import importlib

import numpy as np
import pytest
import torch

import attn_l0_reference as R

pytestmark = pytest.mark.gpu

ATTN_TAU_DEFAULT = 8          # csrc/attention.hip g_attn_tau
# Form 27 against float64 may be this much worse than form 17 on the unscaled twins: the two runs see different fp16 roundings of q and k
# and so two different fp16 realisations of P; neither is the better one (measured ratios: profiles/attn_l0_time.md)
SP_FACTOR = 1.1


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def dev():
    sub("_lib").require_device()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return {name: R.make_case(b, h, n, st, seed=i) for i, (name, b, h, n, st) in enumerate(R.SHAPES)}


def run(dev, case, form, prescaled=False):
    """One launch of the given form; q | k views keep their stacked row stride on the device."""
    ops = sub("ops")
    qn, kn = (case["qs16"], case["ks16"]) if prescaled else (case["q16"], case["k16"])
    if case["stacked"]:
        C = qn.shape[2]
        both = torch.from_numpy(np.ascontiguousarray(np.concatenate([qn, kn], axis=2))).to(dev)
        q, k = both[:, :, :C], both[:, :, C:]
    else:
        q, k = torch.from_numpy(np.ascontiguousarray(qn)).to(dev), torch.from_numpy(np.ascontiguousarray(kn)).to(dev)
    vt = torch.from_numpy(case["vt16"]).to(dev)
    out = ops.attention_vt_ex(q, k, vt, case["H"], case["M"], prescaled=prescaled, form=form)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", [s[0] for s in R.SHAPES])
def test_form_27_gives_form_17s_bits_on_its_operands_and_holds_its_bound(dev, cases, name):
    case = cases[name]
    o17, o27, o17s = run(dev, case, 17), run(dev, case, 27, prescaled=True), run(dev, case, 17, prescaled=True)
    assert np.array_equal(o27.view(np.uint16), o17s.view(np.uint16)), name
    e17, e27 = R.rel_l2(o17, case["ref"]), R.rel_l2(o27, case["ref_s"])
    w17, w27 = R.worst_row_rel_l2(o17, case["ref"]), R.worst_row_rel_l2(o27, case["ref_s"])
    print(f"[attn_l0] {name}: form 17 {e17:.3e} form 27 {e27:.3e} ratio {e27 / e17:.3f} | worst row 17 {w17[0]:.3e} 27 {w27[0]:.3e} at {w27[1]}")
    assert np.isfinite(o27.astype(np.float32)).all()
    assert e17 < R.ATTN_CAP and e27 < R.ATTN_CAP, (name, e17, e27)
    assert e27 <= SP_FACTOR * e17, (name, e27, e17)
    assert w27[0] < 2 * R.ATTN_CAP, (name, w27)                  # worst (batch, query row) within 2 x the cap (tests/test_gpu_ops.py assert_slices)
    # pre-scaled operands on a form with other arithmetic (15: unfolded shift): the scale left to apply is 1 — the same softmax
    assert R.rel_l2(run(dev, case, 15, prescaled=True), case["ref_s"]) < R.ATTN_CAP, name
    # the default dispatch: unscaled operands stay on form 17, pre-scaled ones take 27 from 1024 keys on
    assert np.array_equal(run(dev, case, 0).view(np.uint16), o17.view(np.uint16)), name
    assert np.array_equal(run(dev, case, 0, prescaled=True).view(np.uint16), o27.view(np.uint16)), name


def test_shift_bookkeeping_rows(dev):
    """Scores climbing by less / by more than tau per tile from a first tile far below zero, falling scores and a late spike: form 27
    with the re-basing slack at 0, 4, the default and 12 (form 17 on the unscaled twins beside it)."""
    lib = sub("_lib")
    for label, case in R.adversarial_cases():
        for tau in (0, 4, ATTN_TAU_DEFAULT, 12):
            lib.check(lib.lib.sdmi_debug_set(b"attn_tau", tau))
            try:
                o17, o27, o17s = run(dev, case, 17), run(dev, case, 27, prescaled=True), run(dev, case, 17, prescaled=True)
            finally:
                lib.check(lib.lib.sdmi_debug_set(b"attn_tau", ATTN_TAU_DEFAULT))
            assert np.array_equal(o27.view(np.uint16), o17s.view(np.uint16)), (label, tau)
            e17, e27 = R.rel_l2(o17, case["ref"]), R.rel_l2(o27, case["ref_s"])
            print(f"[attn_l0] {label} tau {tau}: form 17 {e17:.3e} form 27 {e27:.3e}")
            assert np.isfinite(o27.astype(np.float32)).all(), (label, tau)
            assert e17 < R.ATTN_CAP and e27 < R.ATTN_CAP, (label, tau, e17, e27)
            assert R.worst_row_rel_l2(o27, case["ref_s"])[0] < 2 * R.ATTN_CAP, (label, tau)


def test_large_norm_key_row(dev):
    """One key of 6 x the usual norm (test_attention_role_offset_kernel's spike row) under that test's bounds: 1.5e-3 on the tensor, 2 x that
    on the worst query row and head, 2e-2 absolute on the spike's own query row."""
    case, row = R.large_norm_key_case()
    for form, pre, ref in ((17, False, case["ref"]), (27, True, case["ref_s"])):
        got = run(dev, case, form, prescaled=pre).astype(np.float64)
        assert np.isfinite(got).all()
        e, w = R.rel_l2(got, ref), R.worst_row_rel_l2(got, ref)
        print(f"[attn_l0] large-norm key, form {form}: {e:.3e}, worst row {w[0]:.3e} at {w[1]}, spike row max abs {np.abs(got[0, row] - ref[0, row]).max():.3e}")
        assert e < 1.5e-3, (form, e)
        assert w[0] < 2 * 1.5e-3, (form, w)                      # one head: the per-head slice is the tensor
        assert np.abs(got[0, row] - ref[0, row]).max() < 2e-2, form


def test_form_27_refuses_unscaled_operands(dev, cases):
    case = cases[R.SHAPES[0][0]]
    with pytest.raises(RuntimeError, match="pre-scaled"):
        run(dev, case, 27, prescaled=False)
