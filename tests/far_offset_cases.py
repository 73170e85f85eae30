"""Cases of tests/test_gpu_far_offsets.py (test infrastructure; the CPU tier runs the same file on the host-emulated library).

A case hands ONE operand of one entry to the kernel inside a tests/far_buffers.FarBuffer, whose rows are 2^24 elements apart (2^23 where
a batch of two has to fit the 2^32-element span), so that the last rows of the operand start past element 2^31 and byte 2^32 of the
address the kernel is given; every other operand stays small and dense.  (Where an entry takes one stride for several operands — the
Swin LayerNorms, a (hi, lo) pair — those operands are column blocks of one far buffer.)  References and pass rules are the ones each entry's own GPU
file already has (gemm_problem / assert_gemm / family of tests/test_gpu_abi.py, _attn_ref with the 5e-4 / 1.5e-3 caps of
tests/test_gpu_ops.py, assert_parity and the float64 graphs of the upscaler files): nothing new is tolerated here.  After the launch
`FarBuffer.untouched()` requires every word of the allocation outside the stored layout to be +0 still, and an input to hold its bits.

Geometry: 136 rows (one image of 8 x 17 pixels for the convolutions: ragged against every tile; rows 128 .. 135 start past 2^31)."""
import ctypes
import importlib
import json

import numpy as np
import torch

import attn_l0_reference as L0
from far_buffers import FarBuffer
from helpers import rel_l2, seeded, worst_slice_rel_l2
from test_gpu_abi import (EP_GEGLU, EP_OUT_F32, EP_TRANSPOSE, GENERIC_CAP, GuardedRows, OUT_FILL, PINGPONG, SCORE_FAMILIES, TILE_NAMES, assert_gemm,
                          family, gemm_problem, knobs, launch_gemm, lay, n_for, ref64, up)
from test_gpu_ops import ATTN_FOLD_MIN_M_DEFAULT, assert_attn_slices
from test_gpu_swin2sr import lnadd_inputs, lnadd_ref
from test_gpu_swinir import assert_parity, ln_ref, r16d

LD = 1 << 24                    # row stride of a far operand: row 128 starts at element 2^31
LD_B2 = 1 << 23                 # ... where two batch elements of 136 rows share one span (2 x 136 x 2^23 < 2^32)
BS_FAR = (1 << 31) + 64         # a far batch stride: the second batch element starts past element 2^31
HI, WI = 8, 17                  # 136 pixels


def sub(name):
    return importlib.import_module("stable-diffusion-webui_amd." + name)


def same_bits(a, b):
    ints = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.contiguous().view(ints), b.to(a.dtype).contiguous().view(ints))


def release():
    """After each test: the dense device copies that test_gpu_abi.up keeps alive for the launch."""
    import test_gpu_abi
    torch.cuda.synchronize()
    test_gpu_abi._ALIVE.clear()


def peak(dev):
    return f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB"


class Fars:
    """The far buffers of one case: inputs keep their bits, nothing outside any stored layout is written, all freed at the end."""

    def __init__(self, dev):
        self.dev, self.inputs, self.all = dev, [], []
        torch.cuda.reset_peak_memory_stats()

    def input(self, dense, ld, batch=1, bs=0, dtype=torch.float16, zero_columns=False):
        dense = dense.reshape(batch, -1, dense.shape[-1]).to(dtype)
        fb = FarBuffer(dense.shape[1], dense.shape[2], ld, dtype, self.dev, batch, bs).fill(dense, zero_columns=zero_columns)
        self.inputs.append((fb, 0, dense))
        self.all.append(fb)
        return fb

    def block(self, fb, col0, dense):
        """An input operand as a column block of `fb` (made with `output`): filled under fill()'s rule, its bits checked at the end."""
        dense = dense.reshape(fb.geom[0], fb.geom[1], -1).to(fb.full.dtype)
        fb.fill(dense, col0)
        self.inputs.append((fb, col0, dense))
        return fb.at(col0)

    def output(self, rows, cols, ld, batch=1, bs=0, dtype=torch.float16):
        self.all.append(FarBuffer(rows, cols, ld, dtype, self.dev, batch, bs))
        return self.all[-1]

    def close(self, what):
        torch.cuda.synchronize()
        try:
            for fb, col0, dense in self.inputs:
                assert same_bits(fb.read()[:, :, col0:col0 + dense.shape[2]], dense), (what, "an input operand was written")
            for fb in self.all:
                fb.untouched(what)
            return peak(self.dev)
        finally:
            self.free()

    def free(self):
        for fb in self.all:
            fb.free()
        self.inputs, self.all = [], []


# ---- sdmi_conv_gemm ---------------------------------------------------------------------------------------------------------------------------
def launch_far(abi, dev, pr, far, *, impl=0, workspace=False, what="", ld_out=LD):
    """test_gpu_abi.launch_gemm with one operand far: `far` = "a0" | "a1" | "out" | "resid" puts that operand's rows LD apart (batch 1);
    "a_bs" | "w_bs" | "o_bs" | "r_bs" keeps the rows dense and puts the batch elements BS_FAR apart.  -> (stored output, launch names)."""
    L, check, ptr, sp = abi
    lib = sub("_lib")
    batch, B, Hi, Wi, c0, c1, N, M, flags = (pr[k] for k in ("batch", "B", "Hi", "Wi", "c0", "c1", "N", "M", "flags"))
    assert (batch == 1) == (far in ("a0", "a1", "out", "resid")) and not (far == "a_bs" and c1)
    pix = B * Hi * Wi
    fars = Fars(dev)

    def place(name, bsname, dense, ld):
        """-> (address, ld, bs) of an input operand [za, rows, cols]"""
        za, rows, _ = dense.shape
        if far == name:
            return fars.input(dense, LD, za, rows * LD).addr, LD, rows * LD
        if far == bsname:
            return fars.input(dense, ld, za, BS_FAR).addr, ld, BS_FAR
        bs = rows * ld + 8 * (1 + len(name))
        return lay(dense, ld, bs, torch.float16, dev)[1], ld, bs

    d = lib.ConvDesc()
    d.a0, lda0, a_bs = place("a0", "a_bs", pr["a0"].reshape(-1, pix, c0), c0 + 8)
    lda1 = 0
    if c1:
        d.a1, lda1, _ = place("a1", "-", pr["a1"].reshape(-1, pix, c1), c1 + 16)
        a_bs = 0                                             # two sources only come with batch 1 here
    d.w, _, w_bs = place("-", "w_bs", pr["w"], pr["K"])
    if pr["bias_t"] is not None:
        d.bias = up(pr["bias_t"], dev).data_ptr()
    if pr["rowbias_t"] is not None:
        d.rowbias = up(pr["rowbias_t"], dev).data_ptr()
    ldr = 0
    if pr["resid_t"] is not None:
        d.resid, ldr, d.r_bs = place("resid", "r_bs", pr["resid_t"], N + 16)
    _, rows, cols = pr["ref"].shape
    otype = torch.float32 if flags & EP_OUT_F32 else torch.float16
    if far == "out":
        ldo, o_bs = ld_out, rows * ld_out
        out = fars.output(rows, cols, ldo, dtype=otype)
    elif far == "o_bs":
        ldo, o_bs = cols + 8, BS_FAR
        out = fars.output(rows, cols, ldo, batch, o_bs, dtype=otype)
    else:
        ldo = cols + 8
        o_bs = rows * ldo + 24
        out = GuardedRows(batch, rows, cols, ldo, o_bs, otype, dev)
    d.out = out.addr
    d.c0, d.c1, d.lda0, d.lda1 = c0, c1, lda0, lda1
    d.B, d.Hi, d.Wi, d.Ho, d.Wo = B, Hi, Wi, pr["Ho"], pr["Wo"]
    d.taps, d.stride, d.pad, d.up = pr["taps"], pr["stride"], 1 if pr["taps"] == 9 else 0, pr["up"]
    d.N, d.n_real, d.ldo, d.ldr, d.flags = N, pr["n_real"], ldo, ldr, flags
    d.alpha = pr["alpha"]
    d.batch, d.a_bs, d.w_bs, d.o_bs = batch, a_bs, w_bs, o_bs
    d.force_generic = impl
    if workspace:
        nbytes = int(L.sdmi_conv_splitk_workspace_bytes(M, N, pr["K"], batch))
        assert nbytes > 0
        ws = up(torch.zeros(nbytes + 4096, dtype=torch.uint8), dev)
        ws[nbytes:] = 0x5A
        d.splitk_workspace, d.splitk_workspace_bytes = ws.data_ptr(), nbytes
    check(L.sdmi_profile_begin(), "profile_begin")
    try:
        rc = L.sdmi_conv_gemm(ctypes.byref(d), sp())
        torch.cuda.synchronize()
    finally:
        buf = ctypes.create_string_buffer(1 << 16)
        check(L.sdmi_profile_end(buf, len(buf)), "profile_end")
    try:
        check(rc, "sdmi_conv_gemm")
        names = [k["name"] for k in json.loads(buf.value.decode())["kernels"]]
        if workspace:
            assert bool((ws[nbytes:].cpu() == 0x5A).all()), "the split-K workspace's tail was written"
        got = out.read() if isinstance(out, FarBuffer) else out.read(names)
    except BaseException:
        fars.free()
        raise
    print(f"[far conv_gemm] {what}: {names[0]}; {fars.close(what)}")
    return got, names


def conv_problem(taps, n, **kw):
    g = dict(taps=taps, Hi=HI, Wi=WI, c0=64, c1=64, N=n, bias="col", resid=True, seed=1000 + taps)
    g.update(kw)
    return gemm_problem(**g)


CONV_LD_CASES = [(taps, fam, far) for taps in (1, 9) for fam in SCORE_FAMILIES for far in ("a0", "a1", "out", "resid")]


def check_conv_ld(abi, dev, taps, fam, far):
    """Two sources of 64 channels, a column bias and a residual, N = 256 (320 for the x160 / x320 tiles): every kernel family, confirmed
    from the launch name."""
    kn, impl, ran = family(fam)
    pr = conv_problem(taps, n_for(fam, 256, 320))
    what = f"taps {taps} {fam} far {far}"
    with knobs(**kn):
        got, names = launch_far(abi, dev, pr, far, impl=impl, what=what)
    assert ran(names), (fam, names)
    assert_gemm(got, pr, "far row stride", f"{what} {names[0]}")


CONV_FLAG_CASES = ([(flag, fam) for flag in ("f32", "geglu") for fam in ("default", "4", "generic")] + [("transpose", "default"), ("transpose", "generic")] +
                   [("ep8", fam) for fam in ("default", "5", "12")])


def check_conv_flags(abi, dev, flag, fam):
    """A far output under the other store forms: fp32 rows, GEGLU's N / 2 columns, and EP_TRANSPOSE, whose rows are (b * N + n) — N = 192
    of them, the last 64 past element 2^31 (256 rows of 2^24 would be a span of 2^32: not allowed); "ep8": fp16 rows of ldo = 2^24 + 4, which
    sends the launch to the 8-byte epilogue and its own row products."""
    kn, impl, ran = family(fam)
    if flag == "ep8":
        pr = conv_problem(1, n_for(fam, 256, 320))
        with knobs(**kn):
            got, names = launch_far(abi, dev, pr, "out", what=f"ep8 {fam} far out", ld_out=LD + 4)
        assert ran(names) and "_ep8" in names[0], names
        assert_gemm(got, pr, "far output, other stores", f"ep8 {fam} far out {names[0]}")
        return
    if flag == "transpose":
        pr = gemm_problem(Hi=HI, Wi=WI, c0=64, N=192, flags=EP_TRANSPOSE, bias="col", seed=1100)
    else:
        pr = gemm_problem(Hi=HI, Wi=WI, c0=64, N=256, flags=EP_OUT_F32 if flag == "f32" else EP_GEGLU, bias="col", resid=flag == "f32", seed=1110)
    what = f"{flag} {fam} far out"
    with knobs(**kn):
        got, names = launch_far(abi, dev, pr, "out", impl=impl, what=what)
    assert ran(names) and (impl == 1 or {"f32": "", "geglu": "_geglu", "transpose": "_tr"}[flag] in names[0]), (fam, names)
    assert_gemm(got, pr, "far output, other stores", f"{what} {names[0]}")


CONV_BS_CASES = [(taps, fam, far) for taps in (1, 9) for fam in ("default", "5", "generic") for far in ("a_bs", "w_bs", "o_bs", "r_bs")]


def check_conv_bs(abi, dev, taps, fam, far):
    """Batch 2, rows dense, one batch stride of 2^31 + 64 elements."""
    kn, impl, ran = family(fam)
    pr = gemm_problem(taps=taps, batch=2, Hi=HI, Wi=WI, c0=64, N=n_for(fam, 256, 320), bias="col", resid=True, seed=1200 + taps)
    what = f"taps {taps} {fam} far {far}"
    with knobs(**kn):
        got, names = launch_far(abi, dev, pr, far, impl=impl, what=what)
    assert ran(names) and (impl == 1 or names[0].endswith(" x2")), (fam, names)
    assert_gemm(got, pr, "far batch stride", f"{what} {names[0]}")


CONV_SPLIT_CASES = [(8, 2), (5, 2), (0, 4)]


def check_conv_splitk(abi, dev, cfg, split):
    """K = 1152 in a caller's split-K workspace, the reduce pass storing into far rows (with a far residual beside it in a second case)."""
    n = 320 if cfg in (5, 8) else 128
    pr = gemm_problem(Hi=HI, Wi=WI, c0=1152, N=n, bias="col", resid=True, alpha=0.5, seed=1300)
    for far in ("out", "resid"):
        what = f"split-K cfg {cfg} split {split} far {far}"
        with knobs(gemm_cfg=cfg, gemm_split=split):
            got, names = launch_far(abi, dev, pr, far, workspace=True, what=what)
        assert f"_splitk{split}" in names[0] and names[0].startswith("gemm_mfma_" + TILE_NAMES[cfg]), names
        assert_gemm(got, pr, "far rows, split-K", f"{what} {names[0]}")


# ---- attention --------------------------------------------------------------------------------------------------------------------------------
ATTN_D = (40, 64, 80, 128, 160, 32)
VT_HEADS = {40: 4, 64: 3, 80: 2, 128: 1, 160: 1, 32: 5}        # H * D = 160 rows of V^T (192 / 128 where D does not divide 160)
ATTN_VT_CASES = ([(d, m, far, 0) for d in ATTN_D for m in (136, 77) for far in ("q", "k", "out", "vt")] +
                 [(40, 136, far, form) for form in (15, 17) for far in ("q", "k", "out", "vt")] +
                 [(40, 384, far, form) for form in (20, 30) for far in ("q", "k", "out")])        # the 8- / 12-wave kernels: N >= 256 / 384, M >= 256
_ATTN = {}


def attn_problem(d, heads, b, n, m, seed):
    key = (d, heads, b, n, m, seed)
    if key not in _ATTN:
        q, k, v = (seeded((b, r, heads * d), seed + i).half() for i, r in enumerate((n, m, m)))
        _ATTN[key] = (q, k, v, ref64(q, k, v, heads))
    return _ATTN[key]


def assert_attn(got, ref, heads, cap, what):
    e = rel_l2(got, ref)
    print(f"[far attention] {what}: {e:.3e} (cap {cap})")
    assert bool(torch.isfinite(got.float()).all()) and e < cap, (what, e, cap)
    assert_attn_slices(got.double(), ref, heads, cap, what)


def vt_dense(v, m, pad_value=1000.0):
    """[B, M, C] -> V^T [B, C, M rounded up to 64], the padding columns finite and not zero."""
    b, _, c = v.shape
    vt = torch.full((b, c, (m + 63) // 64 * 64), pad_value, dtype=torch.float16)
    vt[:, :, :m] = v.transpose(1, 2)
    return vt


def check_attention_vt(abi, dev, d, m, far, form):
    """sdmi_attention_vt(_ex): q, k, out far in turn with two heads and batch 2 (rows 2^23 apart: b * N * ld passes 2^31 in the second
    batch element), V^T far with vt_ld = 2^24 and batch 1.  D = 32 runs the generic kernel."""
    L, check, ptr, sp = abi
    n = 136
    heads, b = (VT_HEADS[d], 1) if far == "vt" else (2, 2)
    if form in (20, 30):                                     # N = M = 384 rows of one image, 2^23 apart: rows 256 .. 383 start past 2^31
        n, b = 384, 1
    c = heads * d
    q, k, v, ref = attn_problem(d, heads, b, n, m, 2000 + d)
    vt = vt_dense(v, m)
    fars = Fars(dev)
    what = f"vt D {d} heads {heads} B {b} N {n} M {m} far {far} form {form}"
    qa, ldq = (fars.input(q, LD_B2, b, n * LD_B2).addr, LD_B2) if far == "q" else (up(q, dev).data_ptr(), c)
    ka, ldk = (fars.input(k, LD_B2, b, m * LD_B2).addr, LD_B2) if far == "k" else (up(k, dev).data_ptr(), c)
    va, vt_ld = (fars.input(vt, LD, 1, c * LD).addr, LD) if far == "vt" else (up(vt, dev).data_ptr(), vt.shape[2])
    if far == "out":
        out = fars.output(n, c, LD_B2, b, n * LD_B2)
        oa, ldo = out.addr, LD_B2
    else:
        out = GuardedRows(b, n, c, c + 8, n * (c + 8), torch.float16, dev)
        oa, ldo = out.addr, c + 8
    try:
        check(L.sdmi_attention_vt_ex(qa, ka, va, oa, b, heads, n, m, d, ldq, ldk, vt_ld, ldo, float(d ** -0.5), 0, form, 0, sp()), "sdmi_attention_vt_ex")
        torch.cuda.synchronize()
        got = out.read() if far == "out" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far attention] {what}: {fars.close(what)}")
    assert_attn(got, ref, heads, GENERIC_CAP if d == 32 else 5e-4, what)


ATTN_V_CASES = [(d, m) for d in ATTN_D for m in (136, 77)]


def check_attention_row_major_v(abi, dev, d, m):
    """sdmi_attention with V row-major in far rows: transpose_v_kernel's ((long)b * M + m) * ldv."""
    L, check, ptr, sp = abi
    n, heads, b = 136, 2, 2
    c = heads * d
    q, k, v, ref = attn_problem(d, heads, b, n, m, 2000 + d)
    fars = Fars(dev)
    what = f"row-major V D {d} M {m} far v"
    va = fars.input(v, LD_B2, b, m * LD_B2).addr
    out = GuardedRows(b, n, c, c + 8, n * (c + 8), torch.float16, dev)
    nbytes = int(L.sdmi_attention_workspace_bytes(b, heads, m, d))
    ws = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    try:
        check(L.sdmi_attention(up(q, dev).data_ptr(), up(k, dev).data_ptr(), va, out.addr, b, heads, n, m, d, c, c, LD_B2, c + 8, float(d ** -0.5),
                               ptr(ws), nbytes, sp()), "sdmi_attention")
        torch.cuda.synchronize()
        assert bool((ws[nbytes:].cpu() == 0x5A).all()), "the workspace's tail was written"
        got = out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far attention] {what}: {fars.close(what)}")
    assert_attn(got, ref, heads, GENERIC_CAP if d == 32 else 5e-4, what)


ATTN_WIDE_CASES = [(m, far) for m in (136, 77) for far in ("q", "k", "v", "out")]


def check_attention_wide(abi, dev, m, far):
    """sdmi_attention_wide (one head of D = 64, batch 2; the cap 1e-3 of its own test): its GEMMs read q rows and k rows (as weight rows)
    and store the output rows through the far stride."""
    L, check, ptr, sp = abi
    n, d, b = 136, 64, 2
    q, k, v, ref = attn_problem(d, 1, b, n, m, 2100)
    fars = Fars(dev)
    what = f"wide M {m} far {far}"
    addr, ld = {}, {}
    for name, t in (("q", q), ("k", k), ("v", v)):
        if far == name:
            addr[name], ld[name] = fars.input(t, LD_B2, b, t.shape[1] * LD_B2).addr, LD_B2
        else:
            addr[name], ld[name] = lay(t, d + 8, t.shape[1] * (d + 8), torch.float16, dev)[1], d + 8
    if far == "out":
        out = fars.output(n, d, LD_B2, b, n * LD_B2)
        ldo = LD_B2
    else:
        out = GuardedRows(b, n, d, d + 8, n * (d + 8), torch.float16, dev)
        ldo = d + 8
    nbytes = int(L.sdmi_attention_wide_workspace_bytes(b, n, m, d))
    ws = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    try:
        check(L.sdmi_attention_wide(addr["q"], addr["k"], addr["v"], out.addr, b, n, m, d, ld["q"], ld["k"], ld["v"], ldo, float(d ** -0.5), ptr(ws),
                                    nbytes, sp()), "sdmi_attention_wide")
        torch.cuda.synchronize()
        assert bool((ws[nbytes:].cpu() == 0x5A).all()), "the workspace's tail was written"
        got = out.read() if far == "out" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far attention] {what}: {fars.close(what)}")
    assert_attn(got, ref, 1, 1e-3, what)


# ---- attention form 27 at attn_stage_fits' limits ---------------------------------------------------------------------------------------------
FORM27_CASES = ["ldk", "vt_ld"]
LDK_LAST, LDK_FIRST_REFUSED = (1 << 24) - 8, 1 << 24                    # 64 * ldk * 2 < 2^31
VTLD_LAST, VTLD_FIRST_REFUSED = 26843544, 26843552                      # 40 * vt_ld * 2 < 2^31 <=> vt_ld < 26843545.6; multiples of 8
_L0 = {}


def check_form27_limits(abi, dev, which):
    """Pre-scaled operands, N = M = 136, D = 40, two heads, through sdmi_attention_vt_ex.  At the largest stride attn_stage_fits admits
    (a tile's byte offsets just below 2^31) form 27 must hold its bound of tests/test_gpu_attn_l0_forms.py: the bits of form 17 on the same
    operands, the cap, 1.1 x form 17's own error on the unscaled twins, every query row within 2 x the cap.  One step further form 27 is
    refused with its message, and the default dispatch (form 0, with the fold threshold lowered to these 136 keys so that it is the
    17 / 27 choice that is asked) computes through form 17: bit-equal to form 17 asked for by name."""
    L, check, ptr, sp = abi
    lib = sub("_lib")
    assert 64 * LDK_LAST * 2 < 2 ** 31 <= 64 * LDK_FIRST_REFUSED * 2 and 40 * VTLD_LAST * 2 < 2 ** 31 <= 40 * VTLD_FIRST_REFUSED * 2
    if "case" not in _L0:
        _L0["case"] = L0.make_case(1, 2, 136, False, seed=27)
    case = _L0["case"]
    n, heads, d, c = 136, 2, 40, 80
    vt16 = torch.from_numpy(case["vt16"]).clone()
    vt16[:, :, n:] = 1000.0                                              # padding columns: finite, not zero

    def run(form, prescaled, stride):
        q, k = (torch.from_numpy(np.ascontiguousarray(case[key])) for key in (("qs16", "ks16") if prescaled else ("q16", "k16")))
        fars = Fars(dev)
        what = f"form {form} prescaled {prescaled} {which} {stride}"
        ka, ldk = (fars.input(k, stride, 1, n * stride).addr, stride) if which == "ldk" and stride else (up(k, dev).data_ptr(), c)
        va, vt_ld = (fars.input(vt16, stride, 1, c * stride).addr, stride) if which == "vt_ld" and stride else (up(vt16, dev).data_ptr(), vt16.shape[2])
        out = GuardedRows(1, n, c, c, n * c, torch.float16, dev)
        try:
            rc = L.sdmi_attention_vt_ex(up(q, dev).data_ptr(), ka, va, out.addr, 1, heads, n, n, d, c, ldk, vt_ld, c, float(d ** -0.5), int(prescaled), form,
                                        0, sp())
            torch.cuda.synchronize()
            got = out.read(what)
        except BaseException:
            fars.free()
            raise
        fars.close(what)
        return rc, got[0].numpy()

    last, refused = (LDK_LAST, LDK_FIRST_REFUSED) if which == "ldk" else (VTLD_LAST, VTLD_FIRST_REFUSED)
    (rc27, o27), (rc17s, o17s), (rc17, o17) = run(27, True, last), run(17, True, last), run(17, False, last)
    assert rc27 == 0 and rc17s == 0 and rc17 == 0, lib.last_error()
    assert np.array_equal(o27.view(np.uint16), o17s.view(np.uint16)), which
    e17, e27 = L0.rel_l2(o17[None], case["ref"]), L0.rel_l2(o27[None], case["ref_s"])
    w27 = L0.worst_row_rel_l2(o27[None], case["ref_s"])
    print(f"[far attention] form 27 at {which} = {last}: form 17 {e17:.3e} form 27 {e27:.3e} ratio {e27 / e17:.3f} worst row {w27[0]:.3e} at {w27[1]}")
    assert np.isfinite(o27.astype(np.float32)).all()
    assert e17 < L0.ATTN_CAP and e27 < L0.ATTN_CAP, (which, e17, e27)
    assert e27 <= 1.1 * e17, (which, e27, e17)
    assert w27[0] < 2 * L0.ATTN_CAP, (which, w27)
    rc, o = run(27, True, refused)
    assert rc != 0 and "attention form 27: a tile's byte offsets must fit 32 bits" in lib.last_error(), (rc, lib.last_error())
    assert bool((o.view(np.uint16) == np.float16(-777.0).view(np.uint16)).all())          # nothing ran
    lib.check(lib.lib.sdmi_debug_set(b"attn_fold_min_m", 128))
    try:
        (rc0, o0), (rc0d, o0d) = run(0, True, refused), run(0, True, 0)
    finally:
        lib.check(lib.lib.sdmi_debug_set(b"attn_fold_min_m", ATTN_FOLD_MIN_M_DEFAULT))
    rcs, o17r = run(17, True, refused)
    assert rc0 == 0 and rc0d == 0 and rcs == 0, lib.last_error()
    assert np.array_equal(o0.view(np.uint16), o17r.view(np.uint16)) and np.array_equal(o0.view(np.uint16), o17s.view(np.uint16)), which
    assert np.array_equal(o0d.view(np.uint16), o27.view(np.uint16)), which          # dense strides: the same dispatch takes form 27


# ---- the ping-pong 3x3 guard ------------------------------------------------------------------------------------------------------------------
# name: (geometry at the last admitted size, geometry at the first refused one); launch_gemm admits < 128 images and < 2040 rows / columns
# of the (upsampled) window grid.  The two sides of the row / column limits are two problems; Hi = 2040 takes over 10 s emulated.
PP_GUARD = {
    "images": (dict(B=127, Hi=4, Wi=16), dict(B=128, Hi=4, Wi=16)),
    "rows": (dict(Hi=2039, Wi=16), dict(Hi=2040, Wi=16)),
    "columns": (dict(Hi=16, Wi=2039), dict(Hi=16, Wi=2040)),
    "rows-up": (dict(Hi=1019, Wi=8, up=1), dict(Hi=1020, Wi=8, up=1)),
    "columns-up": (dict(Hi=8, Wi=1019, up=1), dict(Hi=8, Wi=1020, up=1)),
}
PP_GUARD_CASES = [(cfg, name, side) for cfg in PINGPONG for name in PP_GUARD for side in (0, 1)]


def check_pingpong_guard(abi, dev, cfg, name, side):
    """3x3, c0 = 64, gemm_cfg 4 / 5 / 8 against float64 F.conv2d under assert_gemm.  side 0: the ping-pong kernel must run ("pp" in the
    launch name); side 1: the row descriptor (image in 8 bits, window coordinates in 12) cannot hold the problem and the same tile's
    two-stage kernel must run."""
    n = 320 if cfg in (5, 8) else 256
    pr = gemm_problem(taps=9, c0=64, N=n, bias="col", seed=1400, **PP_GUARD[name][side])
    with knobs(gemm_cfg=cfg):
        got, names = launch_gemm(abi, dev, pr)
    tile = "gemm_mfma_" + TILE_NAMES[cfg]
    head = names[0].split(" ")[0].split("_conv3x3")[0]
    print(f"[far guards] ping-pong guard cfg {cfg} {name} side {side}: {names[0]}")
    assert head == tile + ("pp" if side == 0 else ""), names
    assert_gemm(got, pr, "ping-pong guard", f"cfg {cfg} {name} {'admitted' if side == 0 else 'refused'} {names[0]}")


# ---- swin_layernorm / swin_layernorm_add ------------------------------------------------------------------------------------------------------
LN_CASES = ["plain", "add", "add-in-place"]


def check_swin_layernorm(abi, dev, form):
    """sdmi_swin_layernorm / sdmi_swin_layernorm_add, C = 180 of 192 columns, 136 rows of stride 2^24.  Both entries take ONE row stride
    for all their operands, so every operand of the launch is far: they are column blocks 256 apart of the rows of one FarBuffer (one
    slack in front of all of them, so each stays inside the allocation whatever its address arithmetic does).  A read that goes astray
    shows in the result, a write in the blocks' surroundings."""
    L, check, ptr, sp = abi
    rows, c, cp, blk = 136, 180, 192, 256
    y, resid, g, b = lnadd_inputs(rows, c, cp, 3000)
    add = form != "plain"
    ref = lnadd_ref(y, resid, g, b, c) if add else ln_ref(y, g, b, c)
    fars = Fars(dev)
    fb = fars.output(rows, 3 * blk, LD)
    fars.block(fb, 0, y[:, :c].half())                                  # the pad columns of the inputs stay zero
    if form != "add-in-place":
        fars.block(fb, blk, resid[:, :c].half())                        # (also for the plain form, which must not touch it)
    else:
        fb.fill(resid[:, :c].half(), blk)                               # the stream that is updated in place: not an input that keeps its bits
    at = lambda i: fb.addr + 2 * blk * i
    out_blk = 1 if form == "add-in-place" else 2
    gd, bd = up(g, dev), up(b, dev)
    what = f"swin layernorm {form}"
    try:
        if add:
            check(L.sdmi_swin_layernorm_add(at(0), ptr(gd), ptr(bd), at(1), at(out_blk), rows, c, LD, 1e-5, sp()), what)
        else:
            check(L.sdmi_swin_layernorm(at(0), ptr(gd), ptr(bd), at(2), rows, c, LD, 1e-5, sp()), what)
        torch.cuda.synchronize()
        got = fb.read()[0]
    except BaseException:
        fars.free()
        raise
    print(f"[far norms] {what}: {fars.close(what)}")
    o = got[:, out_blk * blk:(out_blk + 1) * blk]
    assert bool((got[:, c:blk] == 0).all()) and bool((got[:, blk + c:2 * blk] == 0).all()), "the gap behind an input block was written"
    if out_blk == 1:
        assert bool((got[:, 2 * blk:] == 0).all()), "the unused block was written"
    assert bool((o[:, c:] == 0).all())                                   # C .. Cp - 1 are written as zeros, Cp .. stay zero
    assert_parity(o[:, :c], ref, r16d(ref), 1, (0,), what)


# ---- dense tensors at the limits the norm launchers state (GPU only: the emulation cannot stream 2^31 elements) ---------------------------------
class profiled:
    """The launch names of a block, from the library's profiler."""

    def __init__(self, abi):
        self.abi, self.names = abi, []

    def __enter__(self):
        self.abi[1](self.abi[0].sdmi_profile_begin(), "profile_begin")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        self.abi[1](self.abi[0].sdmi_profile_end(buf, len(buf)), "profile_end")
        self.names = [k["name"] for k in json.loads(buf.value.decode())["kernels"]]


class GuardedDense:
    """A dense device output between two runs of 64 sentinel elements."""

    def __init__(self, n, dtype, dev):
        self.full = torch.full((n + 128,), OUT_FILL, dtype=dtype, device=dev)
        self.t = self.full[64:64 + n]

    def intact(self):
        return bool((self.full[:64] == OUT_FILL).all()) and bool((self.full[-64:] == OUT_FILL).all())


def periodic_mismatches(out, period_elems):
    """out: flat device tensor whose content must repeat every period_elems elements, bit for bit (a ragged tail included): the number
    of elements that differ from the first period, counted on the device in chunks."""
    ints = out.view(torch.int16 if out.dtype == torch.float16 else torch.int32)
    first = ints[:period_elems]
    whole = ints.numel() // period_elems
    per = max(1, (1 << 27) // period_elems)
    bad = 0
    for lo in range(0, whole, per):
        blk = ints[lo * period_elems:min(lo + per, whole) * period_elems].view(-1, period_elems)
        bad += int((blk != first).sum())
    tail = ints[whole * period_elems:]
    return bad + int((tail != first[:tail.numel()]).sum())


P_GN = 64
# name: (HW, c0, c1, B, the launch name's head, bands); launch_groupnorm bands from HW >= 2^24 rows or HW * C >= 2^31 elements per image
GN_LIMITS = {
    "just under the row limit": ((1 << 24) - 64, 64, 0, 1, "groupnorm_silu ", 0),
    "row limit": (1 << 24, 64, 0, 1, "groupnorm_silu_banded ", 2),
    "just under the element limit": (1 << 20, 2016, 0, 1, "groupnorm_silu ", 0),
    "element limit": (1 << 20, 2048, 0, 1, "groupnorm_silu_banded ", 2),
    "batch offsets past 2^31": ((1 << 24) - 64, 64, 0, 3, "groupnorm_silu ", 0),
    "two sources": (1 << 20, 1024, 992, 1, "groupnorm_silu ", 0),
}


def check_groupnorm_limit(abi, dev, name):
    """sdmi_groupnorm, 32 groups, SiLU on.  Every image is a seeded block of 64 pixel rows repeated HW / 64 times (on the device), so each
    group's mean and variance are the block's and the float64 reference is computed on the block alone.  Rule: output rows p and p + 64
    of an image are bit-equal (the position must not change the arithmetic; counted over the whole tensor on the device), and the block
    holds the GroupNorm rules of tests/test_gpu_ops.py — rel_l2 < 5e-4 and every (image, group) within 1.25 x its own fp16 floor — which,
    the rows being bit-equal, is then true of every chunk of the tensor.  Which path ran is read from the launch name."""
    import torch.nn.functional as F
    from test_gpu_ops import GN_FLOOR_FACTOR, gn_worst_floor_multiple
    L, check, ptr, sp = abi
    HW, c0, c1, B, head, bands = GN_LIMITS[name]
    C = c0 + c1
    assert HW % P_GN == 0
    blocks = (seeded((B, P_GN, C), 3100) * 1.7 + 0.3).half()
    g, bt = 1 + 0.1 * seeded((C,), 3101), 0.1 * seeded((C,), 3102)
    ref = F.silu(F.group_norm(blocks.double().permute(0, 2, 1), 32, g.double(), bt.double(), eps=1e-5)).permute(0, 2, 1)
    torch.cuda.reset_peak_memory_stats()
    rep = lambda t: t.to(dev).repeat(1, HW // P_GN, 1).contiguous()
    x0 = rep(blocks[..., :c0])
    x1 = rep(blocks[..., c0:]) if c1 else None
    out = GuardedDense(B * HW * C, torch.float16, dev)
    wsb = int(L.sdmi_groupnorm_workspace_bytes(B, HW, 32))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    gd, bd = g.to(dev), bt.to(dev)
    with profiled(abi) as prof:
        check(L.sdmi_groupnorm(ptr(x0), ptr(x1), c0, c1, ptr(gd), ptr(bd), ptr(out.t), B, HW, 32, 1e-5, 1, ptr(ws), wsb, sp()), "sdmi_groupnorm")
    names = prof.names
    assert len(names) == 1 and names[0].startswith(head) and (not bands or names[0].endswith(f" x{bands}")), (name, names)
    assert out.intact(), name
    bad = sum(periodic_mismatches(out.t[b * HW * C:(b + 1) * HW * C], P_GN * C) for b in range(B))
    got = torch.stack([out.t[b * HW * C:b * HW * C + P_GN * C].view(P_GN, C) for b in range(B)]).float().cpu()
    e = rel_l2(got, ref)
    mult, where, err, floor = gn_worst_floor_multiple(got[:, :, None, :], ref[:, :, None, :])
    print(f"[far norms] groupnorm {name}: {names[0]}; elements differing from their row's first period {bad}; block rel_l2 {e:.3e} (cap 5e-4), "
          f"worst (image, group) {where} {err:.3e} = {mult:.3f} x floor {floor:.3e} (cap {GN_FLOOR_FACTOR}); {peak(dev)}")
    del x0, x1, out
    torch.cuda.empty_cache()
    assert bad == 0, (name, bad)
    assert e < 5e-4 and mult <= GN_FLOOR_FACTOR, (name, e, mult, where)


LN_ROWS, LN_C, LN_PERIOD = (1 << 21) + 3, 1024, 257            # 2^31 + 3072 elements


def check_layernorm_limit(abi, dev, entry):
    """sdmi_layernorm / sdmi_ln_rowstats on 2^21 + 3 rows of 1024 channels, rows of period 257: the float64 reference on the 257 rows, the
    caps the entries' own tests use (layernorm: rel_l2 < 5e-4, every row within 2 x that; rowstats: the mean to 16 x 2^-24 of the row's
    mean |x|, rstd to 16 x 2^-24 of itself), and every later row bit-equal to its first occurrence."""
    import torch.nn.functional as F
    from test_gpu_ops import assert_slices
    L, check, ptr, sp = abi
    block = (seeded((LN_PERIOD, LN_C), 3200) * 2 + 0.5).half()
    g, bt = 1 + 0.1 * seeded((LN_C,), 3201), 0.1 * seeded((LN_C,), 3202)
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty((LN_ROWS, LN_C), dtype=torch.float16, device=dev)
    whole = LN_ROWS // LN_PERIOD
    bd = block.to(dev)
    x[:whole * LN_PERIOD].view(whole, LN_PERIOD, LN_C).copy_(bd)
    x[whole * LN_PERIOD:].copy_(bd[:LN_ROWS - whole * LN_PERIOD])
    if entry == "layernorm":
        out = GuardedDense(LN_ROWS * LN_C, torch.float16, dev)
        gd, btd = g.to(dev), bt.to(dev)
        with profiled(abi) as prof:
            check(L.sdmi_layernorm(ptr(x), ptr(gd), ptr(btd), ptr(out.t), LN_ROWS, LN_C, 1e-5, sp()), "sdmi_layernorm")
        assert out.intact()
        bad = periodic_mismatches(out.t, LN_PERIOD * LN_C)
        got = out.t[:LN_PERIOD * LN_C].view(LN_PERIOD, LN_C).float().cpu()
        ref = F.layer_norm(block.double(), (LN_C,), g.double(), bt.double(), eps=1e-5)
        e = rel_l2(got, ref)
        worst = worst_slice_rel_l2(got, ref, (0,))
        print(f"[far norms] layernorm rows {LN_ROWS} C {LN_C}: {prof.names}; elements differing from their first occurrence {bad}; rel_l2 {e:.3e} "
              f"(cap 5e-4), worst row {worst[0]:.3e} at {worst[1]} (cap 1e-3); {peak(dev)}")
        del x, out
        torch.cuda.empty_cache()
        assert bad == 0 and e < 5e-4
        assert_slices(got, ref, 5e-4, ((0,),), ctx="layernorm at 2^31 elements")
    else:
        st = GuardedDense(LN_ROWS * 2, torch.float32, dev)
        with profiled(abi) as prof:
            check(L.sdmi_ln_rowstats(ptr(x), ptr(st.t), LN_ROWS, LN_C, 1e-5, sp()), "sdmi_ln_rowstats")
        assert st.intact()
        bad = periodic_mismatches(st.t, LN_PERIOD * 2)
        s = st.t[:LN_PERIOD * 2].view(LN_PERIOD, 2).cpu().double()
        X = block.double()
        u = 2.0 ** -24
        rstd = 1.0 / torch.sqrt(X.var(1, unbiased=False) + 1e-5)
        e_mean = float(((s[:, 0] - X.mean(1)).abs() / (16 * u * X.abs().mean(1))).max())
        e_rstd = float(((s[:, 1] - rstd).abs() / (16 * u * rstd)).max())
        print(f"[far norms] ln_rowstats rows {LN_ROWS} C {LN_C}: {prof.names}; words differing from their first occurrence {bad}; mean {e_mean:.3f}, "
              f"rstd {e_rstd:.3f} of their caps; {peak(dev)}")
        del x, st
        torch.cuda.empty_cache()
        assert bad == 0 and e_mean <= 1 and e_rstd <= 1, (bad, e_mean, e_rstd)


# ---- upscaler entries with strides (descriptors filled here: the ops.py wrappers insist on contiguous tensors) ---------------------------------
def _rows(t):
    """[b, h, w, c] -> [1, b h w, c]"""
    return t.reshape(1, -1, t.shape[-1])


RRDB_CASES = [("in", "lrelu", 0), ("out", "relu", 0), ("in", "lrelu", 1), ("out", "lrelu", 1), ("r1", "res2", 0), ("r2", "res2", 0), ("out", "res2", 0)]


def check_rrdb_conv(abi, dev, far, ep, up_):
    """sdmi_rrdb_conv, 64 -> 64 channels, one image of 8 x 17 pixels.  With the fused x2 gather the far input is 12 x 12 (its 144 rows
    pass 2^31; the 24 x 24 output is dense) and the far output 8 x 18 from a dense 4 x 9 input.  test_gpu_esrgan's float64-free rule:
    the fp32 reference, the fp16-storage twin as the yardstick."""
    import torch.nn.functional as F
    import test_gpu_esrgan as E
    from fp16_emu import r16
    L, check, ptr, sp = abi
    lib = sub("_lib")
    hi, wi = ((12, 12) if far == "in" else (4, 9)) if up_ else (HI, WI)
    ho, wo = (2 * hi, 2 * wi) if up_ else (hi, wi)
    x, w, bias, xd, wp, bp = E.conv_case(dev, 1, hi, wi, 64, 64, 3300 + up_)
    r1, r2 = seeded((1, ho, wo, 64), 3301).half(), seeded((1, ho, wo, 64), 3302).half()
    conv = E.ref_conv(x, w, bias, 64, up=bool(up_))
    if ep == "res2":
        ref = (conv * 0.2 + r1.float()) * 0.2 + r2.float()
        twin = r16(r16(r16(conv) * 0.2 + r1.float()) * 0.2 + r2.float())
    else:
        ref = F.leaky_relu(conv, 0.2) if ep == "lrelu" else F.relu(conv)
        twin = r16(ref)
    fars = Fars(dev)
    what = f"rrdb_conv far {far} ep {ep} up {up_}"
    d = lib.RrdbDesc()
    d.w, d.bias = wp.data_ptr(), bp.data_ptr()
    d.in_, d.lda = (fars.input(_rows(x.half()), LD).addr, LD) if far == "in" else (xd.data_ptr(), 64)
    if ep == "res2":
        d.r1, d.ldr1 = (fars.input(_rows(r1), LD).addr, LD) if far == "r1" else (up(r1, dev).data_ptr(), 64)
        d.r2, d.ldr2 = (fars.input(_rows(r2), LD).addr, LD) if far == "r2" else (up(r2, dev).data_ptr(), 64)
    if far == "out":
        out = fars.output(ho * wo, 64, LD)
        d.ldo = LD
    else:
        out = GuardedRows(1, ho * wo, 64, 72, 0, torch.float16, dev)
        d.ldo = 72
    d.out = out.addr
    d.B, d.H, d.W, d.cin, d.up, d.nout, d.n_real = 1, ho, wo, 64, up_, 64, 64
    d.ep = {"lrelu": lib.RRDB_EP_LRELU, "relu": lib.RRDB_EP_RELU, "res2": lib.RRDB_EP_RES2}[ep]
    d.store, d.alpha, d.beta = lib.RRDB_ST_F16, 0.2, 0.2
    try:
        check(L.sdmi_rrdb_conv(ctypes.byref(d), sp()), "sdmi_rrdb_conv")
        torch.cuda.synchronize()
        got = out.read() if far == "out" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far upscalers] {what}: {fars.close(what)}")
    E.assert_parity(got.view(1, ho, wo, 64), ref, twin, 3, (0, 1), what)


COMPACT_CASES = ["in", "out", "behind"]


def check_compact_conv(abi, dev, far):
    """sdmi_compact_conv with PReLU, 64 channels, 8 x 17 pixels, under test_gpu_compact's rule."""
    import torch.nn.functional as F
    import test_gpu_compact as K
    from fp16_emu import r16
    L, check, ptr, sp = abi
    lib = sub("_lib")
    x, w, bias, xd, wp, bp = K.conv_case(dev, 1, HI, WI, 64, 3400)
    slope = torch.linspace(-0.3, 1.2, 64)
    ref = F.prelu(K.ref_conv(x, w, bias, 64).permute(0, 3, 1, 2), slope).permute(0, 2, 3, 1)
    fars = Fars(dev)
    what = f"compact_conv far {far}"
    d = lib.CompactDesc()
    d.w, d.bias, d.slope = wp.data_ptr(), bp.data_ptr(), up(slope, dev).data_ptr()
    d.in_, d.lda = (fars.input(_rows(x.half()), LD).addr, LD) if far == "in" else (xd.data_ptr(), 64)
    if far == "behind":
        # The output starts right behind the channels of the input's last row, inside what would be that row's stride: disjoint bytes.
        # (The entry's overlap check once measured a tensor as rows x stride and refused this — and, depending on where the allocator put
        # the output, the far input above.)
        m, lda = HI * WI, 136
        both = up(torch.zeros((m - 1) * lda + 64 + m * 64, dtype=torch.float16), dev)
        torch.as_strided(both, (m, 64), (lda, 1)).copy_(x.half().reshape(m, 64).to(dev))
        d.in_, d.lda = both.data_ptr(), lda
        tail = both[(m - 1) * lda + 64:]
        d.out, d.ldo = tail.data_ptr(), 64
    elif far == "out":
        out = fars.output(HI * WI, 64, LD)
        d.out, d.ldo = out.addr, LD
    else:
        out = GuardedRows(1, HI * WI, 64, 72, 0, torch.float16, dev)
        d.out, d.ldo = out.addr, 72
    d.B, d.H, d.W, d.cin, d.n_real, d.ep = 1, HI, WI, 64, 64, lib.COMPACT_EP_PRELU
    try:
        check(L.sdmi_compact_conv(ctypes.byref(d), sp()), "sdmi_compact_conv")
        torch.cuda.synchronize()
        got = tail.cpu().clone() if far == "behind" else out.read() if far == "out" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far upscalers] {what}: {fars.close(what)}")
    K.assert_parity(got.view(1, HI, WI, 64), ref, r16(ref), 3, (0, 1), what)


SWIN_CASES = [(kind, far, shift) for kind in ("swin", "swin2") for far in ("qkv", "out") for shift in (0, 4)]


def check_swin_attention(abi, dev, kind, far, shift):
    """sdmi_swin_attention / sdmi_swin2_attention on a grid of 8 x 24 tokens (three whole windows, 192 token rows), two heads of D = 32
    (no slot tails: every stored element of qkv is data), against the float64 graphs of the entries' own files under assert_parity."""
    S = importlib.import_module("test_gpu_swinir" if kind == "swin" else "test_gpu_swin2sr")
    L, check, ptr, sp = abi
    lib = sub("_lib")
    b, h, w, heads, dd = 1, 8, 24, 2, 32
    case = S.attn_case(b, h, w, heads, dd, 3500)
    qkv = S.packed_qkv(case)
    fars = Fars(dev)
    what = f"{kind}_attention far {far} shift {shift}"
    d = lib.SwinAttnDesc() if kind == "swin" else lib.Swin2AttnDesc()
    d.bias = up(S.expanded_bias(case).float().contiguous(), dev).data_ptr()
    d.qkv, d.ldq = (fars.input(_rows(qkv), LD).addr, LD) if far == "qkv" else (up(qkv, dev).data_ptr(), 96 * heads)
    if far == "out":
        out = fars.output(h * w, 32 * heads, LD)
        d.ldo = LD
    else:
        out = GuardedRows(1, h * w, 32 * heads, 32 * heads + 8, 0, torch.float16, dev)
        d.ldo = 32 * heads + 8
    d.out = out.addr
    d.B, d.H, d.W, d.heads, d.D, d.shift = b, h, w, heads, dd, shift
    if kind == "swin":
        d.scale = dd ** -0.5
    else:
        d.head_scale = up(case["scale"].float().contiguous(), dev).data_ptr()
    try:
        check((L.sdmi_swin_attention if kind == "swin" else L.sdmi_swin2_attention)(ctypes.byref(d), sp()), what)
        torch.cuda.synchronize()
        got = out.read() if far == "out" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far upscalers] {what}: {fars.close(what)}")
    S.assert_parity(got.view(b, h, w, heads * dd), S.graph(case, shift), S.graph(case, shift, S.r16d), 3, (0, 1), what)


HAT_CAB_CASES = ["ldt", "ldc", "ldo", "gate-ld"]


def check_hat_cab(abi, dev, far):
    """sdmi_hat_cab_add (out = t + 0.5 gate[image] conv; two images of 68 rows, 64 channels; the gate is the float64 one, rounded to fp32)
    with t, conv, out far in turn, and sdmi_hat_channel_gate pooling far rows of y ("gate-ld"), under the rules of tests/test_gpu_hat.py."""
    import test_gpu_hat as Hh
    L, check, ptr, sp = abi
    n, c, cs = 68, 64, 2
    case = Hh.cab_case(n, c, cs)
    gref = Hh.gate_ref(case)
    fars = Fars(dev)
    what = f"hat far {far}"
    if far == "gate-ld":
        y = fars.input(case["conv"].half(), LD, 2, n * LD)
        hold = [up(case[k].float().contiguous(), dev) for k in ("w1", "b1", "w3", "b3")]
        ws = up(torch.zeros((2, (n + 255) // 256, c), dtype=torch.float32), dev)
        gate = up(torch.full((2, c), 7.0, dtype=torch.float32), dev)
        try:
            check(L.sdmi_hat_channel_gate(y.addr, *(ptr(x) for x in hold), ptr(ws), ptr(gate), 2, n, c, cs, LD, sp()), "sdmi_hat_channel_gate")
            torch.cuda.synchronize()
        except BaseException:
            fars.free()
            raise
        err = rel_l2(gate.cpu(), gref)
        print(f"[far upscalers] {what}: channel gate {err:.3e} (fp32 out: bound 1e-5); {fars.close(what)}")
        assert err < 1e-5
        return
    ref = case["t"].double() + 0.5 * gref.float().double()[:, None] * case["conv"].double()
    gate = up(gref.float().contiguous(), dev)
    ta, ldt = (fars.input(case["t"].half(), LD, 2, n * LD).addr, LD) if far == "ldt" else (up(case["t"].half(), dev).data_ptr(), c)
    ca, ldc = (fars.input(case["conv"].half(), LD, 2, n * LD).addr, LD) if far == "ldc" else (up(case["conv"].half(), dev).data_ptr(), c)
    if far == "ldo":
        out = fars.output(n, c, LD, 2, n * LD)
        ldo = LD
    else:
        out = GuardedRows(2, n, c, c + 8, n * (c + 8), torch.float16, dev)
        ldo = c + 8
    try:
        check(L.sdmi_hat_cab_add(ta, ca, ptr(gate), out.addr, 2 * n, n, c, ldt, ldc, ldo, 0.5, sp()), "sdmi_hat_cab_add")
        torch.cuda.synchronize()
        got = out.read() if far == "ldo" else out.read(what)
    except BaseException:
        fars.free()
        raise
    print(f"[far upscalers] {what}: {fars.close(what)}")
    Hh.assert_parity(got, ref, Hh.r16d(ref), 2, (0, 1), what)


# ---- the window-16 kernels, ScuNET's block and DAT's row kernels -------------------------------------------------------------------------------
def _launch(fars, what, call):
    """One launch with the module's error pattern: free on error, close (and check) on success -> the peak-memory text."""
    try:
        call()
        torch.cuda.synchronize()
    except BaseException:
        fars.free()
        raise


WIN16_CASES = [(kind, far) for kind in ("hat-self", "hat-self-shift", "hat-overlap", "dat", "dat-shifted") for far in ("qkv", "out")]


def check_window16(abi, dev, kind, far):
    """sdmi_hat_window_attention (self, shifted by 8, overlapping) and sdmi_dat_window_attention (8 x 16 | 16 x 8 windows, plain and
    shifted) on two images of 16 x 16 tokens, two heads of D = 32 (no slot tails): 512 token rows 2^23 apart, the second image's rows past
    element 2^31.  The descriptors are the entries' own test files' (`win_desc`), with the far address and stride put in."""
    L, check, ptr, sp = abi
    hat = kind.startswith("hat")
    S = importlib.import_module("test_gpu_hat" if hat else "test_gpu_dat")
    b, h, w, heads, dd = 2, 16, 16, 2, 32
    if hat:
        case = S.win_case(1 if kind == "hat-overlap" else 0, b, h, w, heads, dd)
        arg = 8 if kind == "hat-self-shift" else 0
    else:
        case = S.win_case(b, h, w, heads, dd, (8, 16))
        arg = kind == "dat-shifted"
    fars = Fars(dev)
    what = f"window-16 {kind} far {far}"
    fields = {}
    if far == "qkv":
        qkv = torch.cat([S.to_slots(case[n].flatten(3), heads, dd) for n in "qkv"], dim=-1)
        fields.update(qkv=fars.input(_rows(qkv), LD_B2).addr, ldq=LD_B2)
        out = GuardedRows(1, b * h * w, 32 * heads, 32 * heads + 8, 0, torch.float16, dev)
        fields.update(out=out.addr, ldo=32 * heads + 8)
    else:
        out = fars.output(b * h * w, 32 * heads, LD_B2)
        fields.update(out=out.addr, ldo=LD_B2)
    desc, hold = S.win_desc(dev, case, arg, fields=fields)
    entry = L.sdmi_hat_window_attention if hat else L.sdmi_dat_window_attention
    _launch(fars, what, lambda: check(entry(ctypes.byref(desc), sp()), what))
    got = out.read() if far == "out" else out.read(what)
    print(f"[far upscalers] {what}: {fars.close(what)}")
    got, tails = S.from_slots(got.view(b, h, w, 32 * heads), heads, dd)
    ref, twin = S.win_graph(case, arg), S.win_graph(case, arg, S.r16d)
    S.assert_parity(got, ref, twin, 3, (0, 1), what)


SCU_CASES = [(far, shift) for far in ("x", "out", "in-place") for shift in (0, 4)]


def check_scu_block(abi, dev, far, shift):
    """sdmi_scu_block, C = 64, 8 x 24 tokens (192 rows 2^24 apart): far x, far out, and out == x in place in the far rows."""
    S = importlib.import_module("test_gpu_scunet")
    L, check, ptr, sp = abi
    lib = sub("_lib")
    b, h, w, c = 1, 8, 24, 64
    case = S.block_case(b, h, w, c)
    packs, bias = S.on_device(dev, case)
    bias = bias.float().contiguous()
    x = case["x"].half()
    fars = Fars(dev)
    what = f"scu_block far {far} shift {shift}"
    d = lib.ScuBlockDesc()
    d.packs, d.bias = packs.data_ptr(), bias.data_ptr()
    d.B, d.H, d.W, d.C, d.shift = b, h, w, c, shift
    if far == "in-place":
        out = fars.output(h * w, c, LD)
        out.fill(_rows(x))
        d.x, d.ldx, d.out, d.ldo = out.addr, LD, out.addr, LD
    else:
        d.x, d.ldx = (fars.input(_rows(x), LD).addr, LD) if far == "x" else (up(x, dev).data_ptr(), c)
        if far == "out":
            out = fars.output(h * w, c, LD)
            d.out, d.ldo = out.addr, LD
        else:
            out = GuardedRows(1, h * w, c, c + 8, 0, torch.float16, dev)
            d.out, d.ldo = out.addr, c + 8
    _launch(fars, what, lambda: check(L.sdmi_scu_block(ctypes.byref(d), sp()), what))
    got = out.read(what) if far == "x" else out.read()
    print(f"[far upscalers] {what}: {fars.close(what)}")
    S.assert_parity(got.view(b, h, w, c), S.graph(case, shift), S.graph(case, shift, S.r16d), 3, (0, 1), what)


DAT_ROW_CASES = ["dwconv-ldx", "dwconv-ldm", "dwconv-ldo", "gram-ldq", "aim-lds", "aim-ldt", "aim-ldo", "pool-gate-ld"]


def check_dat_rows(abi, dev, which):
    """DAT's row kernels with one row stride of 2^24 at a time: sdmi_dat_dwconv3x3 (8 x 17 pixels, 64 channels; GELU, or the product with
    `mul` for ldm), sdmi_dat_channel_gram (two images of 68 tokens, two heads of D = 32; the matrix after sdmi_dat_channel_softmax),
    sdmi_dat_aim_combine and sdmi_dat_pool_gate (two images of 68 rows of six 30-wide head slots: the slot tails are zero columns).
    References and rules: tests/test_gpu_dat.py."""
    import torch.nn.functional as F
    import test_gpu_dat as Dd
    from fp16_emu import r16
    L, check, ptr, sp = abi
    lib = sub("_lib")
    fars = Fars(dev)
    what = f"dat rows {which}"
    kind, _, far = which.partition("-")
    if kind == "dwconv":
        b, h, w, c = 1, HI, WI, 64
        ep = 1 if far == "ldm" else 0
        x, mul = r16(seeded((b, h, w, c), 5100)), r16(seeded((b, h, w, c), 5103))
        wt, bias = seeded((c, 1, 3, 3), 5101, 0.5), seeded((c,), 5102, 0.3)
        conv = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), padding=1, groups=c).permute(0, 2, 3, 1)
        ref = F.gelu(conv) if ep == 0 else conv * mul.double()
        xa, ldx = (fars.input(_rows(x.half()), LD).addr, LD) if far == "ldx" else (up(x.half(), dev).data_ptr(), c)
        ma, ldm = (fars.input(_rows(mul.half()), LD).addr, LD) if far == "ldm" else (up(mul.half(), dev).data_ptr(), c)
        if far == "ldo":
            out = fars.output(h * w, c, LD)
            ldo = LD
        else:
            out = GuardedRows(1, h * w, c, c + 8, 0, torch.float16, dev)
            ldo = c + 8
        w9, bd = up(wt.view(c, 9).t().contiguous(), dev), up(bias, dev)
        _launch(fars, what, lambda: check(L.sdmi_dat_dwconv3x3(xa, ptr(w9), ptr(bd), ma if ep else None, out.addr, b, h, w, c, ldx, ldm if ep else 0, ldo, ep,
                                                               sp()), what))
        got = out.read() if far == "ldo" else out.read(what)
        print(f"[far upscalers] {what}: {fars.close(what)}")
        Dd.assert_parity(got.view(b, h, w, c), ref, Dd.r16d(ref), 3, (0, 1), what)
    elif kind == "gram":
        b, n, heads, dd = 2, 68, 2, 32
        q, k, temp = Dd.channel_case(b, n, heads, dd, False)
        qk = torch.cat([Dd.to_slots(q.flatten(2), heads, dd), Dd.to_slots(k.flatten(2), heads, dd)], dim=-1)
        qa = fars.input(qk, LD, b, n * LD).addr
        part = up(torch.full((b, heads, (n + 511) // 512, 1088), 7.0, dtype=torch.float32), dev)
        a = up(torch.full((b, 32 * heads, 32 * heads), 7.0, dtype=torch.float16), dev)
        t = up(temp.float().contiguous(), dev)

        def call():
            check(L.sdmi_dat_channel_gram(qa, ptr(part), b, n, heads, LD, sp()), "sdmi_dat_channel_gram")
            check(L.sdmi_dat_channel_softmax(ptr(part), ptr(t), ptr(a), b, n, heads, dd, sp()), "sdmi_dat_channel_softmax")
        _launch(fars, what, call)
        print(f"[far upscalers] {what}: {fars.close(what)}")
        blocks = a.cpu().view(b, heads, 32, heads, 32)
        got = torch.stack([blocks[:, hd, :dd, hd, :dd] for hd in range(heads)], dim=1)
        ref = Dd.channel_graph(q, k, temp)
        Dd.assert_parity(got, ref, Dd.r16d(ref), 1, (0, 2), what)
    else:
        n = 68
        case = Dd.aim_case(n)
        s_, t_ = case["att"], case["conv"]
        gref = Dd.gate_ref(case, t_)
        if kind == "pool":
            xa = fars.input(t_.half(), LD, 2, n * LD, zero_columns=True).addr
            hold = [up(case[k].float().contiguous(), dev) for k in ("ci_w1", "ci_b1", "ci_w2", "ci_b2")]
            ws = up(torch.zeros((2, (n + 255) // 256, 192), dtype=torch.float32), dev)
            gate = up(torch.full((2, 192), 7.0, dtype=torch.float32), dev)
            _launch(fars, what, lambda: check(L.sdmi_dat_pool_gate(xa, *(ptr(v) for v in hold), ptr(ws), ptr(gate), 2, n, 192, case["c8"], LD, sp()), what))
            err = rel_l2(gate.cpu(), gref)
            print(f"[far upscalers] {what}: pool gate {err:.3e} (fp32 out: bound 1e-5); {fars.close(what)}")
            assert err < 1e-5
            return
        hid = F.gelu(s_.double() @ case["si_w1"].double().t() + case["si_b1"].double())
        sg = torch.sigmoid(hid @ case["si_w2"].double() + case["si_b2"])
        ref = s_.double() * gref.float().double()[:, None] + t_.double() * sg[..., None]
        sa, lds = (fars.input(s_.half(), LD, 2, n * LD, zero_columns=True).addr, LD) if far == "lds" else (up(s_.half(), dev).data_ptr(), 192)
        ta, ldt = (fars.input(t_.half(), LD, 2, n * LD, zero_columns=True).addr, LD) if far == "ldt" else (up(t_.half(), dev).data_ptr(), 192)
        if far == "ldo":
            out = fars.output(n, 192, LD, 2, n * LD)
            ldo = LD
        else:
            out = GuardedRows(2, n, 192, 200, n * 200, torch.float16, dev)
            ldo = 200
        hold = [up(gref.float().contiguous(), dev)] + [up(case[k].float().contiguous(), dev) for k in ("si_w1", "si_b1", "si_w2")]
        d = lib.DatAimDesc()
        d.s, d.t, d.gate, d.w1, d.b1, d.w2 = [sa, ta] + [v.data_ptr() for v in hold]
        d.b2, d.out, d.rows, d.rows_per_image, d.C, d.C16, d.lds, d.ldt, d.ldo = case["si_b2"], out.addr, 2 * n, n, 192, case["c16"], lds, ldt, ldo
        _launch(fars, what, lambda: check(L.sdmi_dat_aim_combine(ctypes.byref(d), sp()), what))
        got = out.read() if far == "ldo" else out.read(what)
        print(f"[far upscalers] {what}: {fars.close(what)}")
        got, tails = Dd.from_slots(got, 6, 30)
        assert bool((tails == 0).all())
        ref = Dd.from_slots(ref, 6, 30)[0]
        Dd.assert_parity(got, ref, Dd.r16d(ref), 2, (0, 1), what)


# ---- sdmi_conv_gemm_ex: (hi, lo) stream tensors -----------------------------------------------------------------------------------------------
HILO_CASES = [(fam, far) for fam in ("8", "0") for far in ("out", "resid")]


def check_conv_hilo(abi, dev, fam, far):
    """sdmi_conv_gemm_ex with out_lo and resid_lo, 1x1, K = 128, on the 128x320 ping-pong tile (gemm_epilogue_hilo) and the 128x128 one.
    A pair shares its row stride, so `out` | `out_lo` (or `resid` | `resid_lo`) are two column blocks of ONE far buffer: both halves far,
    one slack in front of both.  The rule of tests/gemm_extras_cases.py: rel_l2(hi + lo) < 4e-6 against float64 of the formula with the
    residual pair's sum, rel_l2(hi) in (1e-4, 6e-4), |lo| <= ulp(hi) / 2."""
    from test_cpu_kernel_emulation import _split_hilo
    L, check, ptr, sp = abi
    lib = sub("_lib")
    kn, impl, ran = family(fam)
    N = n_for(fam, 256, 320)
    pr = gemm_problem(taps=1, Hi=HI, Wi=WI, c0=128, N=N, bias="col", resid=True, seed=1350)
    M, blk = pr["M"], N + 64
    r_hi, r_lo = _split_hilo(np.random.default_rng(77).standard_normal((1, M, N)))
    r_lo[r_lo == 0] = np.float16(2.0 ** -24)                  # no exact zeros in a far input; the reference takes the pair as stored
    r_hi, r_lo = torch.from_numpy(r_hi), torch.from_numpy(r_lo)
    want = pr["ref"] - pr["resid_t"].double() + r_hi.double() + r_lo.double()
    fars = Fars(dev)
    what = f"(hi, lo) {fam} far {far}"
    d, x = lib.ConvDesc(), lib.GemmExtras()
    _, d.a0 = lay(pr["a0"].reshape(1, M, 128), 136, 0, torch.float16, dev)
    _, d.w = lay(pr["w"], 128, 0, torch.float16, dev)
    d.bias = up(pr["bias_t"], dev).data_ptr()
    if far == "resid":
        rb = fars.output(M, 2 * blk, LD)
        d.resid, x.resid_lo, ldr = fars.block(rb, 0, r_hi), fars.block(rb, blk, r_lo), LD
    else:
        ldr = N + 16
        (_, d.resid), (_, x.resid_lo) = lay(r_hi, ldr, 0, torch.float16, dev), lay(r_lo, ldr, 0, torch.float16, dev)
    if far == "out":
        ob = fars.output(M, 2 * blk, LD)
        d.out, x.out_lo, ldo = ob.at(0), ob.at(blk), LD
    else:
        ldo = N + 8
        hi_g, lo_g = GuardedRows(1, M, N, ldo, 0, torch.float16, dev), GuardedRows(1, M, N, ldo, 0, torch.float16, dev)
        d.out, x.out_lo = hi_g.addr, lo_g.addr
    x.out_lo_bytes, x.resid_lo_bytes = ((M - 1) * ldo + N) * 2, ((M - 1) * ldr + N) * 2
    d.c0, d.lda0, d.B, d.Hi, d.Wi, d.Ho, d.Wo, d.taps, d.stride = 128, 136, 1, HI, WI, HI, WI, 1, 1
    d.N, d.ldo, d.ldr, d.alpha, d.batch, d.force_generic = N, ldo, ldr, 1.0, 1, impl
    with knobs(**kn):
        with profiled(abi) as prof:
            try:
                check(L.sdmi_conv_gemm_ex(ctypes.byref(d), ctypes.byref(x), sp()), "sdmi_conv_gemm_ex")
                torch.cuda.synchronize()
            except BaseException:
                fars.free()
                raise
    names = prof.names
    if far == "out":
        both = ob.read()[0]
        hi, lo = both[:, :N], both[:, blk:blk + N]
        assert bool((both[:, N:blk] == 0).all()) and bool((both[:, blk + N:] == 0).all()), "the gap behind a half of the pair was written"
    else:
        hi, lo = hi_g.read(names)[0], lo_g.read(names)[0]
    peak_text = fars.close(what)
    assert ran(names) and "_hl" in names[0], (fam, names)
    pair = hi.double() + lo.double()
    e_pair, e_hi = rel_l2(pair, want[0]), rel_l2(hi, want[0])
    ulp = 2.0 ** (torch.floor(torch.log2(hi.double().abs().clamp_min(2.0 ** -14))) - 10)
    over = float((lo.double().abs() / ulp).max())
    print(f"[far conv_gemm] {what}: {names[0]}; rel_l2(hi + lo) {e_pair:.2e} (cap 4e-6), rel_l2(hi) {e_hi:.2e}, worst |lo| {over:.3f} ulp(hi) (cap 0.5); {peak_text}")
    assert bool(torch.isfinite(pair).all()) and e_pair < 4e-6 and 1e-4 < e_hi < 6e-4 and over <= 0.5, (what, names, e_pair, e_hi, over)
