"""The cases of the GEMM's engine-only epilogues — GroupNorm statistics (stats_out), LayerNorm row partials (lnp_out), the LayerNorm fold
(EP_LNFOLD), (hi, lo) stream tensors (out_lo / resid_lo) and the riders bias_scale and gate — one launch at a time against float64.

Each `check_*` function holds one case: its seeded operands, its float64 reference and its assertions.  It is written against a small
back end, "run this descriptor + extras under these knobs, give me the launch name and the written-back counts":

    be.dev                                   torch device the operands live on
    be.L                                     the library's plain entries (profiler, workspace sizes)
    be.conv_gemm(dref, x, stream) -> rc      sdmi_conv_gemm_ex(d, x) (tests/test_gpu_gemm_extras.py) or emu_conv_gemm (tests/test_cpu_gemm_extras_cases.py)
    be.knobs(kn)                             context manager: the tuning knobs for the launches inside
    be.groupnorm_ex / ln_rowstats / ln_fold_weights(...) -> (rc, launch name)
    be.last_error(), be.stream()

The descriptor, its strided operands with 3000 in every gap and the sentinel-filled output are those of tests/test_gpu_abi.py
(`launch_gemm`, `lay`, `GuardedRows`, `Guarded`), the elementwise rule is its `assert_gemm`; the statistics rules are
tests/test_cpu_kernel_emulation.py's `_assert_chunk_stats` and `_gn_worst_floor_multiple`.  Every extras buffer has the worst-case size
sdmi_conv_gemm_ex demands plus a sentinel tail, and every float the launch had no reason to write must still hold the sentinel.

Shapes: B = 2 images of 16 x 16 (a chunk index needs b > 0; 256 rows per image divide every BM into 1, 2 or 4 chunks; Wo = 16 admits the
row-shared 3x3 walk), 3x3 with 64 input channels (K = 576), 1x1 with 128; N = 256 (8 channels per group) on the 64- / 128- / 256-wide
tiles and 320 (10 per group: groups straddle the 16-lane shuffle tree and the 4-column lane fragments) on the x160 / x320 ones; N = 640 (20 per group) on 128x320, 256x320 and 128x160, so that a group's column tile is not tile 0.

Bounds that are not another module's rule:
  * LayerNorm row partials: against the float64 sums of the STORED fp16 values v of one row and column tile, |sum - S| <= 2 BN 2^-24 sum|v|
    and |sumsq - Q| <= 2 BN 2^-24 Q: BN fp32 additions in any order of terms of that magnitude (plus the square's own rounding), times 2.
  * (hi, lo): rel_l2(hi + lo, float64) < 4e-6 (two fp16 tensors carry 22 bits; 2^-22 = 2.4e-7 per element plus the K-term accumulation),
    |lo| <= ulp(hi) / 2 everywhere, hi bit-equal to the plain launch where no lo residual changes the sum.
  * LayerNorm fold: `assert_gemm` against float64 of the epilogue's formula on the operands the kernel sees; 1.2e-3 against float64
    LayerNorm -> Linear of the unfolded weights (adds the fp16 rounding of W * gamma); on the offset-heavy input (row mean 10, std 1)
    per row 2 x the error of the same formula evaluated in numpy float32 from the float64 accumulator and rounded to fp16 (the factor 2:
    the fp32 accumulation order, which that model does not reproduce).
  * ln_fold_weights: wf bit-equal to fp16(w * gamma) (rounded once, or through fp32: see ln_weights); s_out within 2 K 2^-24 sum|wf|, c_out within 2 (K + 2) 2^-24 (sum|beta w| + |bias|)."""
import importlib
import re

import numpy as np
import torch
import torch.nn.functional as F

import test_gpu_abi
from helpers import rel_l2, seeded
from test_cpu_kernel_emulation import (GN_FLOOR_FACTOR, _assert_chunk_stats, _chunk_mean_m2, _gn_ref64, _gn_worst_floor_multiple, _group_offsets,
                                       _split_hilo)
from test_gpu_abi import (EP_GEGLU, EP_OUT_F32, EP_TRANSPOSE, LEAD, OUT_FILL, Guarded, GuardedRows, assert_gemm, family, gemm_problem, lay,
                          launch_gemm, n_for, up)

EP_LNFOLD = 0x4000
U = 2.0 ** -24
B_IMG, HW = 2, 256
M_ROWS = B_IMG * HW
GEOM = dict(B=B_IMG, Hi=16, Wi=16)


def _lib():
    return importlib.import_module("stable-diffusion-webui_amd._lib")


def note(section, case, text):
    print(f"[gemm extras {section}] {case}: {text}")


def release():
    """End of a test: the device copies `lay` / `up` keep alive may go."""
    test_gpu_abi._ALIVE.clear()


class _L:
    """What launch_gemm sees as the library: its sdmi_conv_gemm is the back end's launch with the case's extras."""

    def __init__(self, be, x):
        self.be, self.x = be, x

    def sdmi_conv_gemm(self, dref, stream):
        return self.be.conv_gemm(dref, self.x, stream)

    def __getattr__(self, name):
        return getattr(self.be.L, name)


def launch(be, pr, kn, x, **kw):
    """test_gpu_abi.launch_gemm through the back end -> (stored [1, rows, cols] on the CPU, launch names); with edit=: (rc, GuardedRows)."""
    def check(rc, what="call"):
        assert rc == 0, (what, be.last_error())
    with be.knobs(kn):
        return launch_gemm((_L(be, x), check, None, be.stream), be.dev, pr, **kw)


def untouched(out, what):
    """A GuardedRows no launch may have stored to: every element still holds the sentinel."""
    out.geom = out.geom[:2] + (0,) + out.geom[3:]
    out.read(what)


def tile_of(name):
    m = re.match(r"gemm_mfma_(\d+)x(\d+)", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)), name.split("_")[2].split(" ")[0].endswith("pp")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


class Extras:
    """One sdmi_gemm_extras and the guarded buffers behind it, each of the worst-case size the entry demands."""

    def __init__(self, be, pr, *, stats_cpg=0, lnp=False, out_lo=False, resid_lo=None, ldo=0, ldr=0, out_lo_lead=LEAD, gate=None, bias_scale=0.0):
        self.be, self.x = be, _lib().GemmExtras()
        x, M, N = self.x, pr["M"], pr["N"]
        self.stats = self.lnp = self.out_lo = None
        if stats_cpg:
            self.groups = N // stats_cpg
            self.stats = Guarded((pr["B"] * 64 * self.groups * 2,), torch.float32, be.dev, fill=OUT_FILL)
            x.stats_out, x.stats_cpg, x.stats_bytes = self.stats.t.data_ptr(), stats_cpg, self.stats.t.numel() * 4
        if lnp:
            self.lnp = Guarded((M * (N // 64) * 2,), torch.float32, be.dev, fill=OUT_FILL)
            x.lnp_out, x.lnp_bytes = self.lnp.t.data_ptr(), self.lnp.t.numel() * 4
        if out_lo:
            ld = ldo or N
            self.out_lo = GuardedRows(1, M, N, ld, 0, torch.float16, be.dev, lead=out_lo_lead)
            x.out_lo, x.out_lo_bytes = self.out_lo.addr, ((M - 1) * ld + N) * 2
        if resid_lo is not None:
            ld = ldr or N
            _, x.resid_lo = lay(resid_lo, ld, 0, torch.float16, be.dev)
            x.resid_lo_bytes = ((M - 1) * ld + N) * 2
        if gate is not None:
            x.gate = up(torch.tensor([gate] + [7] * 3, dtype=torch.int32), be.dev).data_ptr()
        x.bias_scale = bias_scale

    def used(self, g, n, what):
        """The first n floats of a guarded fp32 buffer as numpy; everything beyond them, and both guards, must still hold the sentinel."""
        full = g.t.cpu()
        assert bool((full[n:] == OUT_FILL).all()) and g.intact(), (what, "floats beyond the", n, "the launch owns were written")
        return full[:n].double().numpy()


def chunk_stats_figures(s, g):
    want = _chunk_mean_m2(g)
    return (float(np.abs(s[..., 0] - want[..., 0]).max()), 4e-7 * float(np.abs(g).max()) + 1e-7,
            float((np.abs(s[..., 1] - want[..., 1]) / want[..., 1]).max()))


# ---- a. GroupNorm statistics ----------------------------------------------------------------------------------------------------------------
GN_FORMS = ("3x3 residual", "1x1 rowbias", "3x3 ldo N + 4")


def gn_problem(form, n, **over):
    if form == "1x1 rowbias":
        return gemm_problem(**dict(dict(taps=1, c0=128, N=n, rowbias=True, seed=1110, **GEOM), **over))
    return gemm_problem(**dict(dict(taps=9, c0=64, N=n, bias="col", resid=True, seed=1100, **GEOM), **over))


GN_WIDE_FAMILIES = ("8", "5", "9")            # N = 640 on the x320 / x160 tiles: 20 channels per group, and a group's column tile is not tile 0


def check_gn_stats(be, fam, form, n=0):
    """stats_out on one family: nchunk = 256 / BM and "_gn" in the name, the output bit-equal to the plain launch and within assert_gemm's
    rule of float64, the statistics those of the stored fp16 values, nothing written beyond B * nchunk * 32 pairs."""
    kn, impl, ran = family(fam)
    n = n or n_for(fam, 256, 320)
    cpg = n // 32
    pr = gn_problem(form, n)
    kw = dict(ldo=n + 4) if form == "3x3 ldo N + 4" else {}
    plain, names0 = launch(be, pr, kn, None, impl=impl, **kw)
    ex = Extras(be, pr, stats_cpg=cpg)
    got, names = launch(be, pr, kn, ex.x, impl=impl, **kw)
    name = names[0]
    assert ran(names) and ran(names0) and "_gn" not in names0[0], (fam, names, names0)
    bm, bn, _ = tile_of(name)
    nchunk = ex.x.stats_nchunk
    assert n % bn == 0 and nchunk == HW // bm and "_gn" in name and ("_ep8" in name) == bool(kw), (fam, form, name, nchunk)
    assert torch.equal(bits(got), bits(plain)), (fam, form, name, "the statistics epilogue changed the output")
    assert_gemm(got, pr, "GroupNorm statistics", f"{form} {fam} {name}")
    g = got[0].double().numpy().reshape(B_IMG, nchunk, HW // nchunk, 32, cpg)
    s = ex.used(ex.stats, B_IMG * nchunk * 32 * 2, name).reshape(B_IMG, nchunk, 32, 2)
    e_mean, cap_mean, e_m2 = chunk_stats_figures(s, g)
    note("gn", f"{form} | {fam}" + (f" | N {n}, {n // bn} column tiles" if n > 320 else ""), f"{name}: nchunk {nchunk}, worst |mean - float64| {e_mean:.2e} (cap {cap_mean:.2e}), worst M2 relative {e_m2:.2e} (cap 2e-5)")
    _assert_chunk_stats(s, g, (fam, form, name))


GN_NOT_PRODUCED = ("generic", "mfma_reg", "gn_fuse 0", "15 x 16", "cpg 3", "split-K", "fp32 store")


def check_gn_not_produced(be, why):
    """Where launch_gemm's admission rule says no: nchunk = 0, the whole statistics buffer still sentinel, the output bit-equal to plain."""
    kn, impl, kw, cpg = {}, 0, {}, 8
    pr = gn_problem("3x3 residual", 256)
    if why == "generic":
        impl = 1
    elif why == "mfma_reg":
        impl = 2
    elif why == "gn_fuse 0":
        kn = dict(gn_fuse=0)
    elif why == "15 x 16":
        pr = gn_problem("3x3 residual", 256, Hi=15)
    elif why == "cpg 3":
        pr, cpg = gn_problem("3x3 residual", 384), 3
    elif why == "split-K":
        pr, kw = gemm_problem(taps=1, c0=1024, N=256, bias="col", resid=True, seed=1120, **GEOM), dict(workspace=True)
        kn = dict(gemm_cfg=0, gemm_split=2)                 # (a forced split needs a forced tile)
    elif why == "fp32 store":
        pr = gn_problem("3x3 residual", 256, flags=EP_OUT_F32)
    plain, names0 = launch(be, pr, kn, None, impl=impl, **kw)
    ex = Extras(be, pr, stats_cpg=cpg)
    got, names = launch(be, pr, kn, ex.x, impl=impl, **kw)
    assert names == names0 and "_gn" not in names[0] and ex.x.stats_nchunk == 0, (why, names, ex.x.stats_nchunk)
    if why == "split-K":
        assert "_splitk2" in names[0], names
    ex.used(ex.stats, 0, (why, names))
    assert torch.equal(bits(got), bits(plain)), (why, names)
    assert_gemm(got, pr, "GroupNorm statistics not produced", f"{why} {names[0]}")
    note("gn", f"not produced | {why}", f"{names[0]}: nchunk 0, statistics buffer untouched")


GN_OFFSET_FAMILIES = ("8", "0", "11")          # ping-pong 128x320 (row-shared walk), 128x128 (lean 3x3 walk), the 128x128 four-stage ring
GN_OFFSET_RATIOS = (0.0, 30.0, 300.0)


def check_gn_offsets(be, fam, ratio):
    """Groups `ratio` standard deviations off zero (the offset arrives through the residual): the statistics the GEMM wrote on the device,
    consumed by the GroupNorm apply pass, within 1.25 x the fp16-rounding floor of float64 GroupNorm + SiLU of the stored tensor."""
    kn, impl, ran = family(fam)
    n = n_for(fam, 256, 320)
    cpg = n // 32
    base = gn_problem("3x3 residual", n)
    resid = np.random.default_rng(55).standard_normal((B_IMG, HW, n)) * 0.5 + _group_offsets(B_IMG, n, ratio, 56)
    pr = dict(base, resid_t=torch.from_numpy(resid.reshape(1, M_ROWS, n)).half())
    pr["ref"] = base["ref"] - base["resid_t"].double() + pr["resid_t"].double()
    pr["mag"] = base["mag"] - base["resid_t"].double().abs() + pr["resid_t"].double().abs()
    ex = Extras(be, pr, stats_cpg=cpg)
    got, names = launch(be, pr, kn, ex.x, impl=impl)
    nchunk = ex.x.stats_nchunk
    assert ran(names) and "_gn" in names[0] and nchunk > 0, (fam, names, nchunk)
    assert_gemm(got, pr, "offset-dominated groups", f"ratio {ratio} {fam} {names[0]}")
    val = got[0].double().numpy().reshape(B_IMG, HW, n)
    used = B_IMG * nchunk * 32 * 2
    s = ex.used(ex.stats, used, names).reshape(B_IMG, nchunk, 32, 2)
    _assert_chunk_stats(s, val.reshape(B_IMG, nchunk, HW // nchunk, 32, cpg), (fam, ratio))
    gamma, beta = (1 + 0.1 * seeded((n,), 58)).numpy(), (0.1 * seeded((n,), 59)).numpy()
    want = _gn_ref64(val, gamma, beta, 1e-5, True)
    own, _ = _gn_worst_floor_multiple(want.astype(np.float16), want)
    assert abs(own - 1.0) < 1e-9, own                      # the reference's own fp16 rounding IS the floor: the cap has room only for the kernel
    ws_bytes = int(be.L.sdmi_groupnorm_workspace_bytes(B_IMG, HW, 32))
    assert ws_bytes >= used * 4
    ws = Guarded((ws_bytes // 4,), torch.float32, be.dev)
    ws.t.zero_()
    ws.t[:used].copy_(ex.stats.t[:used])                   # the device-written statistics, as the engine hands them over
    out = Guarded((B_IMG, HW, n), torch.float16, be.dev)
    rc, gname = be.groupnorm_ex(up(got[0].reshape(B_IMG, HW, n), be.dev), None, n, 0, up(torch.from_numpy(gamma), be.dev), up(torch.from_numpy(beta), be.dev),
                                out.t, B_IMG, HW, 32, 1e-5, 1, ws.t, ws_bytes, nchunk, None, None)
    assert rc == 0 and "apply" in gname and out.intact() and ws.intact(), (rc, gname, be.last_error())
    mult, _ = _gn_worst_floor_multiple(out.t.cpu().numpy(), want)
    note("gn", f"offsets | {fam} ratio {ratio:g}", f"{names[0]} -> {gname}: worst (image, group) error {mult:.3f} x the fp16 floor (cap {GN_FLOOR_FACTOR})")
    assert mult <= GN_FLOOR_FACTOR, (fam, ratio, mult)


# ---- b. (hi, lo) stream tensors --------------------------------------------------------------------------------------------------------------
HILO_CASES = {
    "dx 128x320 stats": dict(fam="8", taps=9, c0=64, N=320, stats=True, **GEOM),
    "dx 256x256 stats": dict(fam="4", taps=9, c0=64, N=256, stats=True, **GEOM),
    "dx 256x320 no stats form": dict(fam="5", taps=9, c0=64, N=320, stats=True, expect_gn=False, **GEOM),
    "dx 128x320 stats N 640": dict(fam="8", taps=9, c0=64, N=640, stats=True, **GEOM),
    "1x1 128x320": dict(fam="8", taps=1, c0=128, N=320, **GEOM),
    "1x1 128x64 ragged M": dict(fam="7", taps=1, c0=128, N=64, B=1, Hi=15, Wi=8),
    "3x3 lean 128x128 stats rowbias": dict(fam="0", taps=9, c0=64, N=128, stats=True, rowbias=True, B=2, Hi=16, Wi=8),
    "64x64 general path": dict(fam="2", taps=9, c0=64, N=64, B=1, Hi=8, Wi=8),
    "split-K x2": dict(fam="2", taps=9, c0=256, N=64, B=1, Hi=8, Wi=8, split=2),
    "output pair only": dict(fam="8", taps=1, c0=128, N=320, resid_pair=False, rowbias=True, **GEOM),
    "out_lo 8 bytes off": dict(fam="8", taps=1, c0=128, N=320, lo_lead=LEAD + 4, narrow=True, **GEOM),
    "ldo N + 8": dict(fam="0", taps=9, c0=64, N=256, ldo_pad=8, stats=True, **GEOM),
}


def hilo_problem(c):
    geom = {k: c[k] for k in ("B", "Hi", "Wi")}
    pair = c.get("resid_pair", True)
    pr = gemm_problem(taps=c["taps"], c0=c["c0"], N=c["N"], bias="col", rowbias=c.get("rowbias", False), resid=pair, seed=1300, **geom)
    r_lo = None
    if pair:
        r_hi, r_lo = _split_hilo(np.random.default_rng(77).standard_normal((1, pr["M"], c["N"])))
        old = pr["resid_t"].double()
        pr = dict(pr, resid_t=torch.from_numpy(r_hi))
        pr["ref"] = pr["ref"] - old + torch.from_numpy(r_hi).double() + torch.from_numpy(r_lo).double()
        pr["mag"] = pr["mag"] - old.abs() + torch.from_numpy(r_hi).double().abs() + torch.from_numpy(r_lo).double().abs()
        r_lo = torch.from_numpy(r_lo)
    return pr, r_lo


def hilo_checks(be, c, label, kn, impl, stats_expected):
    """One (hi, lo) launch -> (hi, lo, name, Extras) after the pair's own checks."""
    pr, r_lo = hilo_problem(c)
    N, ldo = c["N"], c["N"] + c.get("ldo_pad", 0)
    ex = Extras(be, pr, out_lo=True, resid_lo=r_lo, ldo=ldo, out_lo_lead=c.get("lo_lead", LEAD), stats_cpg=N // 32 if c.get("stats") else 0)
    split = c.get("split", 0)
    hi, names = launch(be, pr, dict(kn, **({"gemm_split": split} if split else {})), ex.x, impl=impl, ldo=ldo, workspace=split > 1)
    name = names[0]
    lo = ex.out_lo.read(names)
    assert "_hl" in name and ("_ep8" in name or not c.get("narrow")) and (f"_splitk{split}" in name) == (split > 1), (label, names)
    both, want = hi.double() + lo.double(), pr["ref"]
    assert bool(torch.isfinite(both).all()), (label, name)
    e_pair, e_hi = rel_l2(both, want), rel_l2(hi, want)
    ulp = 2.0 ** (torch.floor(torch.log2(hi.double().abs().clamp_min(2.0 ** -14))) - 10)
    over = float((lo.double().abs() / ulp).max())
    figures = f"{name}: rel_l2(hi + lo) {e_pair:.2e} (cap 4e-6), rel_l2(hi) {e_hi:.2e}, worst |lo| {over:.3f} ulp(hi) (cap 0.5)"
    assert e_pair < 4e-6 and 1e-4 < e_hi < 6e-4, (label, name, e_pair, e_hi)
    assert over <= 0.5, (label, name, over)
    if r_lo is None:                                       # no lo residual: the sum is the plain launch's, so hi is what that launch stores
        plain, _ = launch(be, pr, kn, None, impl=impl, ldo=ldo)
        assert torch.equal(bits(hi), bits(plain)), (label, name, "hi is not the plain launch's fp16 rounding")
        figures += ", hi bit-equal to the plain launch"
    if c.get("stats"):
        nchunk, rows = ex.x.stats_nchunk, pr["M"] // pr["B"]
        bm, _, _ = tile_of(name)
        assert (nchunk == rows // bm if stats_expected else nchunk == 0) and ("_gn" in name) == stats_expected, (label, name, nchunk)
        s = ex.used(ex.stats, pr["B"] * nchunk * 32 * 2, name)
        if stats_expected:
            g = both[0].numpy().reshape(pr["B"], nchunk, rows // nchunk, 32, N // 32)
            s = s.reshape(pr["B"], nchunk, 32, 2)
            e_mean, cap_mean, e_m2 = chunk_stats_figures(s, g)
            figures += f", nchunk {nchunk}, statistics of hi + lo: mean {e_mean:.2e} (cap {cap_mean:.2e}), M2 {e_m2:.2e} (cap 2e-5)"
            _assert_chunk_stats(s, g, label)
        else:
            figures += ", nchunk 0, statistics buffer untouched"
    return figures


def check_hilo(be, label):
    c = HILO_CASES[label]
    kn, impl, ran = family(c["fam"])
    note("hilo", label, hilo_checks(be, c, label, kn, impl, c.get("expect_gn", True)))


def check_hilo_stats(be, fam):
    """The statistics form of the (hi, lo) epilogue on every family: 64x64 and 256x320 have none (nchunk 0, the buffer untouched)."""
    kn, impl, ran = family(fam)
    n = n_for(fam, 256, 320)
    c = dict(fam=fam, taps=9, c0=64, N=n, stats=True, **GEOM)
    if fam == "default":
        _, probe = launch(be, hilo_problem(c)[0], kn, None, impl=impl)
        bm, bn, _ = tile_of(probe[0])
    else:
        bm, bn = map(int, re.match(r"(\d+)x(\d+)", test_gpu_abi.TILE_NAMES[int(fam.rstrip("ts"))]).groups())
    expected = (bm, bn) not in ((64, 64), (256, 320)) and impl == 0
    note("hilo", f"statistics | {fam}", hilo_checks(be, c, fam, kn, impl, expected))


def check_hilo_refusals(be):
    """resid_lo without a residual, and (hi, lo) with force_generic: refused, nothing stored."""
    lib = _lib()
    c = dict(taps=1, c0=128, N=256, resid_pair=False, **GEOM)
    pr, _ = hilo_problem(c)
    for what, impl, message in (("resid_lo without resid", 0, "resid_lo without resid"), ("force_generic", 1, "(hi, lo)")):
        ex = Extras(be, pr, out_lo=True, resid_lo=torch.zeros((1, pr["M"], 256), dtype=torch.float16) if impl == 0 else None)
        rc, out = launch(be, pr, {}, ex.x, impl=impl, edit=lambda d: None)
        assert rc != 0 and message in be.last_error(), (what, rc, be.last_error())
        untouched(out, what)
        untouched(ex.out_lo, what)
        note("hilo", f"refused | {what}", be.last_error())


# ---- c. LayerNorm row partials (producer) ---------------------------------------------------------------------------------------------------
def lnp_problem(n):
    return gemm_problem(taps=1, c0=128, N=n, bias="col", resid=True, seed=1400, **GEOM)


def lnp_expected(name, impl, n):
    if impl:
        return 0
    bm, bn, pp = tile_of(name)
    return n // bn if (bm, bn) != (64, 64) and (pp or bm < 256) else 0


def check_lnp(be, fam):
    kn, impl, ran = family(fam)
    n = n_for(fam, 256, 320)
    pr = lnp_problem(n)
    plain, _ = launch(be, pr, kn, None, impl=impl)
    ex = Extras(be, pr, lnp=True)
    got, names = launch(be, pr, kn, ex.x, impl=impl)
    name = names[0]
    assert ran(names), (fam, names)
    np_ = ex.x.lnp_np
    assert np_ == lnp_expected(name, impl, n), (fam, name, np_)
    assert torch.equal(bits(got), bits(plain)), (fam, name, "the partials epilogue changed the output")
    assert_gemm(got, pr, "LayerNorm row partials", f"{fam} {name}")
    part = ex.used(ex.lnp, M_ROWS * np_ * 2, name)
    if np_ == 0:
        note("lnp", fam, f"{name}: lnp_np 0, partials buffer untouched")
        return
    bn = n // np_
    v = got[0].double().numpy().reshape(M_ROWS, np_, bn)
    part = part.reshape(M_ROWS, np_, 2)
    e_sum, e_sq = np.abs(part[..., 0] - v.sum(-1)), np.abs(part[..., 1] - (v * v).sum(-1))
    cap_sum, cap_sq = 2 * bn * U * np.abs(v).sum(-1), 2 * bn * U * (v * v).sum(-1)
    note("lnp", fam, f"{name}: lnp_np {np_}, worst sum error {float((e_sum / cap_sum).max()):.3f} of its cap 2 BN 2^-24 sum|v|, "
                     f"worst sum-of-squares error {float((e_sq / cap_sq).max()):.3f} of its cap 2 BN 2^-24 sum v^2")
    assert (e_sum <= cap_sum).all() and (e_sq <= cap_sq).all(), (fam, name, float((e_sum / cap_sum).max()), float((e_sq / cap_sq).max()))


# ---- c. LayerNorm fold (consumer) -----------------------------------------------------------------------------------------------------------
def ln_weights(be, n, C, seed):
    """W, gamma, beta, b of LayerNorm -> Linear and their fold by sdmi_ln_fold_weights, checked against numpy."""
    w16 = (seeded((n, C), seed, C ** -0.5)).half()
    gamma, beta, bl = 1 + 0.1 * seeded((C,), seed + 1), 0.1 * seeded((C,), seed + 2), 0.1 * seeded((n,), seed + 3)
    wf, s_out, c_out = (Guarded(s, dt, be.dev) for s, dt in (((n, C), torch.float16), ((n,), torch.float32), ((n,), torch.float32)))
    rc, _ = be.ln_fold_weights(up(w16, be.dev), up(gamma, be.dev), up(beta, be.dev), up(bl, be.dev), wf.t, s_out.t, c_out.t, n, C, C)
    assert rc == 0 and wf.intact() and s_out.intact() and c_out.intact(), be.last_error()
    wf_c, s_c, c_c = wf.t.cpu(), s_out.t.cpu(), c_out.t.cpu()
    # fp16(w * gamma): the product of an fp16 and an fp32 number is exact in float64, so `once` is its one correct rounding — what a
    # mixed-precision multiply-and-convert instruction gives; `twice` rounds it to fp32 first, as a separate multiply and convert do (and
    # the host emulator does).  They differ on about one element in 2^13; every element must be bit-equal to one of the two.
    # (numpy converts float64 to fp16 in one rounding; torch's .half() of a double goes through fp32)
    once, twice = torch.from_numpy((w16.double().numpy() * gamma.double().numpy()).astype(np.float16)), (w16.float() * gamma).half()
    is_once, is_twice = bits(wf_c) == bits(once), bits(wf_c) == bits(twice)
    bad = ~(is_once | is_twice)
    assert not bool(bad.any()) and (bool(is_once.all()) or bool(is_twice.all())), \
        ("wf is not fp16(w * gamma)", int((~is_once).sum()), int((~is_twice).sum()), int(bad.sum()), "first (w, gamma, wf, expected):",
         [(float(w16[i, k]), float(gamma[k]), float(wf_c[i, k]), float(once[i, k])) for i, k in bad.nonzero()[:4].tolist()])
    W = w16.double()
    e_s = (s_c.double() - wf_c.double().sum(1)).abs() / (2 * C * U * wf_c.double().abs().sum(1))
    e_c = (c_c.double() - (W @ beta.double() + bl.double())).abs() / (2 * (C + 2) * U * (W.abs() @ beta.double().abs() + bl.double().abs()))
    note("ln fold", f"weights N {n} C {C}", f"wf bit-equal; s_out {float(e_s.max()):.3f} of its cap, c_out {float(e_c.max()):.3f} of its cap")
    assert float(e_s.max()) <= 1 and float(e_c.max()) <= 1, (float(e_s.max()), float(e_c.max()))
    return dict(w16=w16, gamma=gamma, beta=beta, bl=bl, wf=wf_c, ln_s=s_c, bias=c_c)


def ln_input(be, source, C, heavy=False):
    """-> (x fp16 [M, C], ln_stats fp32 tensor on the device, ln_np, text)."""
    M = M_ROWS
    if source.startswith("producer"):                     # a producer launch's output and its partials, chained as the engine chains them
        fam = source.split(" ")[1]
        kn, impl, ran = family(fam)
        pr = gemm_problem(taps=1, c0=128, N=C, bias="col", resid=True, seed=1500, **GEOM)
        ex = Extras(be, pr, lnp=True)
        got, names = launch(be, pr, kn, ex.x, impl=impl)
        assert ran(names) and ex.x.lnp_np == lnp_expected(names[0], 0, C) > 0, (source, names, ex.x.lnp_np)
        return got[0], ex.lnp.t, ex.x.lnp_np, f"partials of {names[0]} (ln_np {ex.x.lnp_np})"
    x16 = (seeded((M, C), 1510) + 10.0).half() if heavy else (seeded((M, C), 1510, 1.5) + 0.3).half()
    if source == "float64":
        X = x16.double()
        st = torch.stack([X.mean(1), 1.0 / torch.sqrt(X.var(1, unbiased=False) + 1e-5)], dim=1).float()
        return x16, up(st, be.dev), 0, "float64 statistics rounded to fp32"
    st = Guarded((M, 2), torch.float32, be.dev)
    rc, name = be.ln_rowstats(up(x16, be.dev), st.t, M, C, 1e-5)
    assert rc == 0 and st.intact(), be.last_error()
    # fp32 sums of C fp16 values in any order: the mean to 16 x 2^-24 of the row's mean |x|; rstd to 16 x 2^-24 of itself, whatever the
    # mean is (the kernel centres its second pass: a variance taken as E[x^2] - mean^2 would lose a factor E[x^2] / var, 100 on the
    # offset-heavy rows, and miss this)
    X, s = x16.double(), st.t.cpu().double()
    var = X.var(1, unbiased=False)
    e_mean = ((s[:, 0] - X.mean(1)).abs() / (16 * U * X.abs().mean(1))).max()
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    e_rstd = ((s[:, 1] - rstd).abs() / (16 * U * rstd)).max()
    assert float(e_mean) <= 1 and float(e_rstd) <= 1, (source, float(e_mean), float(e_rstd))
    return x16, st.t, 0, f"{name} (mean {float(e_mean):.3f}, rstd {float(e_rstd):.3f} of their caps)"


def ln_problem(x16, wts, st_cpu, ln_np, n, C, flags):
    """The launch's operands in gemm_problem's form, the float64 of the epilogue's formula on the operands the kernel sees (ref, mag),
    the float64 LayerNorm -> Linear of the unfolded weights (ref2), and the formula in numpy float32 rounded to fp16 (model)."""
    M = x16.shape[0]
    X, Wf = x16.double(), wts["wf"].double()
    if ln_np > 0:
        p = st_cpu.double()[:M * ln_np * 2].view(M, ln_np, 2).sum(1)
        mean = p[:, 0] / C
        rstd = 1.0 / torch.sqrt(p[:, 1] / C - mean * mean + 1e-5)
    else:
        mean, rstd = st_cpu.double()[:, 0], st_cpu.double()[:, 1]
    acc, s, b = X @ Wf.T, wts["ln_s"].double(), wts["bias"].double()
    ref = rstd[:, None] * (acc - mean[:, None] * s[None, :]) + b[None, :]
    mag = rstd.abs()[:, None] * (X.abs() @ Wf.abs().T + (mean[:, None] * s[None, :]).abs()) + b.abs()[None, :]
    a32 = acc.float().numpy()
    model = (rstd.float().numpy()[:, None] * (a32 - mean.float().numpy()[:, None] * wts["ln_s"].numpy()[None, :]) + wts["bias"].numpy()[None, :])
    model = torch.from_numpy(model.astype(np.float16))
    mu = X.mean(1, keepdim=True)
    ln = (X - mu) / torch.sqrt(X.var(1, unbiased=False, keepdim=True) + 1e-5) * wts["gamma"].double() + wts["beta"].double()
    ref2 = ln @ wts["w16"].double().T + wts["bl"].double()

    def shape(t, is_mag=False):
        if flags & EP_GEGLU:
            if is_mag:
                return None
            v = t.double().view(M, n // 64, 2, 32)
            return (v[:, :, 0] * F.gelu(v[:, :, 1])).reshape(1, M, n // 2)
        if flags & EP_TRANSPOSE:
            return t.view(B_IMG, HW, n).transpose(1, 2).reshape(1, B_IMG * n, HW)
        return t.view(1, M, n)
    pr = dict(gemm_problem(taps=1, c0=C, N=n, bias="col", seed=1520, flags=flags & ~EP_LNFOLD, **GEOM))
    pr.update(a0=x16.view(1, B_IMG, 16, 16, C), w=wts["wf"].view(1, n, C), bias_t=wts["bias"], ref=shape(ref), mag=shape(mag, True), flags=flags)
    return pr, shape(ref2), shape(model.double())


def ln_extras(be, pr, wts, st_dev, ln_np, C):
    ex = Extras(be, pr)
    x = ex.x
    ex.keep = up(wts["ln_s"], be.dev)
    x.ln_stats, x.ln_s, x.ln_np, x.ln_inv_c, x.ln_eps = st_dev.data_ptr(), ex.keep.data_ptr(), ln_np, 1.0 / C, 1e-5
    x.ln_stats_bytes, x.ln_s_bytes = pr["M"] * max(1, ln_np) * 8, pr["N"] * 4
    return ex


LN_SOURCES = ("float64", "rowstats", "producer 8", "producer 9")
LN_FORMS = {"plain": 0, "geglu": EP_GEGLU, "transposed": EP_TRANSPOSE}


def check_ln_fold(be, fam, form, source, heavy=False, C=320, split=0):
    kn, impl, ran = family(fam)
    if split:
        kn = dict(kn, gemm_split=split)
    # N = 320 (640 with GEGLU) wherever the tile's width divides it: 5 column tiles on the 64-wide ones; 256 on 128x128, 512 on 256x256
    n = (512 if fam == "4" else 640) if form == "geglu" else 256 if fam in ("0", "4", "4ts") else 320
    flags = EP_LNFOLD | LN_FORMS[form]
    wts = ln_weights(be, n, C, 1530)
    x16, st_dev, ln_np, src_text = ln_input(be, source, C, heavy)
    pr, ref2, model = ln_problem(x16, wts, st_dev.cpu().flatten() if ln_np else st_dev.cpu(), ln_np, n, C, flags)
    ex = ln_extras(be, pr, wts, st_dev, ln_np, C)
    got, names = launch(be, pr, kn, ex.x, impl=impl, workspace=split > 1, **(dict(ldo=HW + 8) if form == "transposed" else {}))
    name = names[0]
    assert ran(names) and name.endswith(" ln") and (f"_splitk{split}" in name) == (split > 1), (fam, names)
    assert ("_geglu" in name) == (form == "geglu") and ("_tr" in name) == (form == "transposed"), names
    case = f"{form} | {fam} | {source}" + (" | offset-heavy" if heavy else "") + (f" | split {split} C {C}" if split else "")
    e2 = rel_l2(got, ref2)
    if heavy:
        rows = got.shape[1]
        err = lambda t: ((t.double() - pr["ref"]) ** 2).sum(2).sqrt() / (pr["ref"] ** 2).sum(2).sqrt()
        floor, meas = err(model)[0], err(got)[0]
        worst = int((meas / floor).argmax())
        note("ln fold", case, f"{name}, {src_text}: per-row rel_l2 at most {float((meas / floor).max()):.3f} x the float32 model's (cap 2), at row {worst}: "
                              f"measured {float(meas[worst]):.3e}, floor {float(floor[worst]):.3e}; rows {rows}; unfolded reference {e2:.2e} (cap 1.2e-3)")
        assert bool((meas <= 2 * floor).all()), (case, name, float((meas / floor).max()), worst)
    else:
        assert_gemm(got, pr, "LayerNorm fold", f"{case} {name}")
        note("ln fold", case, f"{name}, {src_text}: rel_l2 against the formula {rel_l2(got, pr['ref']):.2e}, against the unfolded reference {e2:.2e} (cap 1.2e-3)")
    assert e2 < 1.2e-3, (case, name, e2)


def check_ln_fold_refusals(be):
    """The two-stage 256-row tiles, the generic kernel and an A operand 2 bytes off: refused with their messages, the output untouched."""
    wts = {}
    for what, fam, impl, shift, message in (("5ts", "5ts", 0, 0, "needs the ping-pong kernel"), ("4ts", "4ts", 0, 0, "needs the ping-pong kernel"),
                                            ("force_generic", "default", 1, 0, "EP_LNFOLD runs on the LDS-direct MFMA kernels only"),
                                            ("a0 + 2 bytes", "default", 0, 2, "EP_LNFOLD runs on the MFMA kernels only")):
        kn, _, _ = family(fam)
        n = n_for(fam, 256, 320)
        wts[n] = wts.get(n) or ln_weights(be, n, 320, 1530)
        x16, st_dev, ln_np, _ = ln_input(be, "float64", 320)
        pr, _, _ = ln_problem(x16, wts[n], st_dev.cpu(), 0, n, 320, EP_LNFOLD)
        ex = ln_extras(be, pr, wts[n], st_dev, 0, 320)

        def edit(d, shift=shift):
            d.a0 = d.a0 + shift
        rc, out = launch(be, pr, kn, ex.x, impl=impl, edit=edit)
        assert rc != 0 and message in be.last_error(), (what, rc, be.last_error())
        untouched(out, what)
        note("ln fold", f"refused | {what}", be.last_error())


# ---- d. riders --------------------------------------------------------------------------------------------------------------------------------
GATE_CASES = {"5": {}, "0": {}, "11": {}, "generic": {}, "split-K": dict(gemm_split=2)}      # (split-K: on the 128x128 tile — a forced split needs a forced tile)


def check_gate(be, label):
    """gate -> a device int: 0 leaves the output entirely sentinel (the reduce pass of a split-K launch included), 1 is the launch without a gate."""
    fam = "0" if label == "split-K" else label
    kn, impl, ran = family(fam)
    kn = dict(kn, **GATE_CASES[label])
    split = label == "split-K"
    n = n_for(fam, 256, 320)
    pr = gemm_problem(taps=1, c0=1024 if split else 128, N=n, bias="col", resid=True, seed=1600, **GEOM)
    plain, names0 = launch(be, pr, kn, None, impl=impl, workspace=split)
    assert ran(names0) and ("_splitk2" in names0[0]) == split, names0
    rc, out = launch(be, pr, kn, Extras(be, pr, gate=0).x, impl=impl, workspace=split, edit=lambda d: None)
    assert rc == 0, be.last_error()
    untouched(out, ("gate 0", label))
    got, names = launch(be, pr, kn, Extras(be, pr, gate=1).x, impl=impl, workspace=split)
    assert names == names0 and torch.equal(bits(got), bits(plain)), (label, names, names0)
    note("riders", f"gate | {label}", f"{names[0]}: gate 0 stores nothing, gate 1 bit-equal to no gate")


def check_bias_scale(be, fam):
    """The range-extended VAE decode: alpha = 1/64 on the accumulator, bias_scale = 1/64 on the bias."""
    kn, impl, ran = family(fam)
    n = n_for(fam, 256, 320)
    base = gemm_problem(taps=9, c0=64, N=n, bias="col", resid=True, alpha=1.0 / 64, seed=1700, **GEOM)
    bias = base["bias_t"].double()
    pr = dict(base, ref=base["ref"] - bias * (1 - 1.0 / 64), mag=base["mag"] - bias.abs() * (1 - 1.0 / 64))
    got, names = launch(be, pr, kn, Extras(be, pr, bias_scale=1.0 / 64).x, impl=impl)
    assert ran(names), (fam, names)
    assert_gemm(got, pr, "bias_scale", f"bias_scale 1/64 alpha 1/64 {fam} {names[0]}")
    note("riders", f"bias_scale | {fam}", f"{names[0]}: within assert_gemm's rule of float64")


def check_null_extras(be, fam):
    """sdmi_conv_gemm_ex(d, NULL, s) is sdmi_conv_gemm(d, s): same launch, same bits."""
    kn, impl, ran = family(fam)
    n = n_for(fam, 256, 320)
    pr = gn_problem("3x3 residual", n)
    def check(rc, what="call"):
        assert rc == 0, (what, be.last_error())
    with be.knobs(kn):
        want, names0 = launch_gemm((be.L, check, None, be.stream), be.dev, pr, impl=impl)
    got, names = launch(be, pr, kn, None, impl=impl)
    assert ran(names) and names == names0 and torch.equal(bits(got), bits(want)), (fam, names, names0)
    note("riders", f"x = NULL | {fam}", f"{names[0]}: bit-equal to sdmi_conv_gemm")


def check_refusals(be):
    """What sdmi_conv_gemm_ex refuses before anything is launched: non-zero, its message, every guarded buffer untouched."""
    pr = gemm_problem(taps=1, c0=128, N=256, bias="col", resid=True, seed=1800, **GEOM)
    M, N = pr["M"], 256
    zero_lo = torch.zeros((1, M, N), dtype=torch.float16)

    def refused(message, build, *, batch=1, flags=0, what=None):
        ex = build()

        def edit(d):
            d.flags |= flags
            if batch > 1:                                  # every batch element on top of the first: only the refusal is of interest
                d.batch, d.o_bs = batch, M * N
        rc, out = launch(be, pr, {}, ex.x, edit=edit)
        assert rc != 0 and message in be.last_error(), (what or message, rc, be.last_error())
        untouched(out, message)
        for g in (ex.stats, ex.lnp):
            if g is not None:
                ex.used(g, 0, message)
        if ex.out_lo is not None:
            untouched(ex.out_lo, message)
        assert ex.x.stats_nchunk == -5 and ex.x.lnp_np == -5, (message, "the written-back counts were touched")
        note("refusals", what or message, be.last_error())

    def mk(edit_x=None, **kw):
        def build():
            ex = Extras(be, pr, **kw)
            ex.x.stats_nchunk = ex.x.lnp_np = -5
            if edit_x:
                edit_x(ex.x)
            return ex
        return build

    def setx(**fields):
        def apply(x):
            for k, v in fields.items():
                setattr(x, k, v(x) if callable(v) else v)
        return apply
    refused("stats_cpg", mk(setx(stats_cpg=0), stats_cpg=8), what="stats_cpg 0")
    refused("stats_cpg", mk(setx(stats_cpg=-8), stats_cpg=8), what="stats_cpg negative")
    refused("stats_cpg", mk(setx(stats_cpg=7), stats_cpg=8), what="N % stats_cpg != 0")
    refused("stats_bytes", mk(setx(stats_bytes=lambda x: x.stats_bytes - 4), stats_cpg=8))
    refused("lnp_bytes", mk(setx(lnp_bytes=lambda x: x.lnp_bytes - 4), lnp=True))
    st = up(torch.zeros(M * 2 * 2), be.dev).data_ptr()
    ok_ln = dict(ln_stats=st, ln_s=st, ln_np=0, ln_inv_c=1.0 / 128, ln_eps=1e-5, ln_stats_bytes=M * 8, ln_s_bytes=N * 4)
    refused("needs ln_stats and ln_s", mk(setx(**dict(ok_ln, ln_stats=None))), flags=EP_LNFOLD, what="EP_LNFOLD without ln_stats")
    refused("needs ln_stats and ln_s", mk(setx(**dict(ok_ln, ln_s=None))), flags=EP_LNFOLD, what="EP_LNFOLD without ln_s")
    refused("ln_stats_bytes", mk(setx(**dict(ok_ln, ln_stats_bytes=M * 8 - 4))), flags=EP_LNFOLD)
    refused("ln_stats_bytes", mk(setx(**dict(ok_ln, ln_np=2, ln_stats_bytes=M * 2 * 8 - 4))), flags=EP_LNFOLD, what="ln_stats_bytes with ln_np 2")
    refused("ln_s_bytes", mk(setx(**dict(ok_ln, ln_s_bytes=N * 4 - 4))), flags=EP_LNFOLD)
    refused("out_lo_bytes", mk(setx(out_lo_bytes=lambda x: x.out_lo_bytes - 2), out_lo=True))
    refused("resid_lo_bytes", mk(setx(resid_lo_bytes=lambda x: x.resid_lo_bytes - 2), out_lo=True, resid_lo=zero_lo))
    refused("batch == 1", mk(out_lo=True), batch=2, what="(hi, lo) with batch 2")
    refused("batch == 1", mk(setx(**ok_ln)), batch=2, flags=EP_LNFOLD, what="EP_LNFOLD with batch 2")
