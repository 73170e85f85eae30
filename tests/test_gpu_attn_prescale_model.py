"""The pre-scaled level-0 self-attention inside the UNet (knob `attn_prescale`, csrc/engine.cpp run_st + csrc/attention.hip form 27): the
320-wide tiny UNet of tests/test_gpu_xattn_chain_model.py at a 32x32 latent, B = 2 — 1024 token rows per image at level 0, the shortest
sequence the folded forms take — teacher-forced block by block with the knob off and on."""
import importlib

import pytest
import torch

import teacher_forcing as tf
from helpers import seeded

pytestmark = pytest.mark.gpu

TF_T = [999.0, 37.5]


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


@pytest.fixture(scope="module")
def wide():
    from oracle import unet as ou
    sub("_lib").require_device()
    schema = sub("schema")
    kw = dict(model_channels=320, num_heads=8, num_head_channels=-1, context_dim=768)
    cfg = schema.tiny_unet(**kw)
    sd = schema.synthetic_state_dict(cfg, None, dtype=torch.float16)
    eng = sub("engine").Engine(0)
    eng.load_unet(cfg, sd)
    yield dict(eng=eng, net=ou.build_unet(ou.tiny_config(**kw), sd), dev=torch.device("cuda", 0),
               x=seeded((2, 4, 32, 32), 405).half().float(), t=torch.tensor(TF_T), ctx=seeded((2, 77, 768), 406).half().float())
    eng.close()


def knobs(**kv):
    lib = sub("_lib")
    for k, v in kv.items():
        lib.check(lib.lib.sdmi_debug_set(k.encode(), v), k)


def traced(w):
    eng, dev = w["eng"], w["dev"]
    eng.set_option("trace", 1)
    try:
        got = eng.unet_forward(w["x"].to(dev), w["t"].to(dev), w["ctx"].to(dev), None).float().cpu()
        torch.cuda.synchronize()
        taps = {k: v.float().cpu() for k, v in eng.taps().items()}
    finally:
        eng.set_option("trace", 0)
    assert torch.isfinite(got).all()
    taps["out"] = got
    return taps


def test_prescaled_self_attention_holds_the_teacher_forcing_rule_and_the_knob_restores_the_old_launches(wide):
    """Every segment passes tests/teacher_forcing.py's rule with `attn_prescale` 0 and 1; on the segments that end in a level-0
    self-attention (`<320-wide block>.attn1+x`) the error against the fp32 oracle with 1 is at most 1.1 x the error with 0 (two fp16
    realisations of q, k and P; measured ratios in profiles/attn_l0_time.md).  With 0 the engine makes the launches it made before
    form 27 existed: every tap has the bits of a forward with form 17 forced through `attn_occ`."""
    net = wide["net"]
    call = lambda n: n(wide["x"], wide["t"], wide["ctx"], None)
    try:
        knobs(attn_prescale=0, attn_occ=17)            # (the 320-wide blocks' cross-attention runs in the fused chain: no other d = 40 launch)
        old = traced(wide)
        knobs(attn_prescale=0, attn_occ=15)
        off = traced(wide)
        knobs(attn_prescale=1)
        on = traced(wide)
    finally:
        knobs(attn_prescale=1, attn_occ=15)
    assert set(off) == set(tf.unet_tap_names(net))
    for name in off:
        assert torch.equal(old[name], off[name]), name
    level0 = [n for n in off if n.endswith(".attn1+x") and 320 in off[n].shape[1:] and off[n].numel() >= 2 * 1024 * 320]
    assert level0, sorted(off)
    assert any(not torch.equal(on[n], off[n]) for n in level0), "attn_prescale = 1 changed nothing: the pre-scaled form did not run"
    rows_off = tf.assert_segments(tf.segment_errors(net, call, off), "wide320@32/attn_prescale_0")
    rows_on = tf.assert_segments(tf.segment_errors(net, call, on), "wide320@32/attn_prescale_1")
    e_off = {r["block"]: r["engine"] for r in rows_off}
    e_on = {r["block"]: r["engine"] for r in rows_on}
    for n in level0:
        print(f"[attn_prescale] {n}: engine error off {e_off[n]:.3e} on {e_on[n]:.3e} ratio {e_on[n] / e_off[n]:.3f}")
    for n in level0:
        assert e_on[n] <= 1.1 * e_off[n], (n, e_on[n], e_off[n])
