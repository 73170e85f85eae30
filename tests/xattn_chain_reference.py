"""float64 reference of the cross-attention chain (csrc/xattn_chain.hip) and its fp16-storage twin, plus the seeded test cases shared by
tests/test_cpu_xattn_chain.py, tests/test_gpu_xattn_chain.py and tools/gpu/xattn_chain_time.py.

    x2 = x1 + Wo attention(Wq LN(x1), K, V) + bo

`graph(..., twin=False)` is the float64 graph on the fp16 operands; `twin=True` is the same graph with the tensors the four launches (and
the chain) store in binary16 — LN(x1), q, the softmax weights P (unnormalised, relative to the row maximum), the normalised attention
output and x2 — rounded to binary16.  The twin's distance from the reference is the yardstick of the parity rule.
"""
import numpy as np

C_WIDTH, HEADS, DHEAD = 320, 8, 40
LOG2E = 1.4426950408889634


def r16(a):
    return a.astype(np.float16).astype(np.float64)


def graph(case, twin=False, eps=1e-5):
    r = r16 if twin else (lambda a: a)
    x = case["x"].astype(np.float64)
    rows, rpi, L = x.shape[0], case["rpi"], case["L"]
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    n = r((x - m) / np.sqrt(v + eps) * case["gamma"].astype(np.float64) + case["beta"].astype(np.float64))
    q = r(n @ case["wq"].astype(np.float64).T)
    k = case["k"].astype(np.float64)
    vt = case["vt"].astype(np.float64)
    a = np.empty_like(q)
    for img in range(rows // rpi):
        sl = slice(img * rpi, (img + 1) * rpi)
        for h in range(HEADS):
            cs = slice(h * DHEAD, (h + 1) * DHEAD)
            s = q[sl, cs] @ k[img, :, cs].T / np.sqrt(DHEAD)
            e = r(np.exp(s - s.max(-1, keepdims=True)))
            a[sl, cs] = (e @ vt[img, cs, :L].T) / e.sum(-1, keepdims=True)     # (columns >= L of V^T: padding, never weighted)
    a = r(a)
    out = x + a @ case["wo"].astype(np.float64).T
    if case["bo"] is not None:
        out = out + case["bo"].astype(np.float64)
    return r(out)


def make_case(images, rpi, L, seed, kind="plain", bias=True, poison=False):
    """Operands as the engine holds them: x [rows][320] fp16, gamma / beta fp32, wq / wo [320][320] fp16, bo fp32 or None, k [images][L][320]
    fp16, vt [images][320][Lpad] fp16 with Lpad = L rounded up to 64 (set_context's layout; padding columns zero, or — `poison` — 100.0).
    Wo is scaled so that the branch's rms is comparable to x's.  kinds:
      plain     standard-normal tokens and context projections
      spike     key L - 2 (in the last, ragged 32-key block) scores about 30 log2 units above the rest for every query
      climb     the scores rise by about 12 log2 units from each 32-key block to the next
      lowfirst  the first 32-key block lies about 40 log2 units below the others
      lnstress  token rows with mean 50 and spread 0.5
    The softmax kinds shift the scores of the ODD heads (one of every wave's two) through the constant part c = beta Wq^T of q: beta is three
    times the size of the normalised tokens, so adding t c_h / |c_h|^2 to key j's head-h columns raises its scaled score by t (1 +- 0.05) log2
    units for every query.  The even heads' rows of Wq are made orthogonal to beta: their q, and so their attention, varies with the token as
    in the plain cases — every column of the branch keeps a token-dependent part (a spike makes a head's output the same for every query, and
    a branch column that is one constant can lie near zero, where a relative error means nothing)."""
    rng = np.random.default_rng(seed)
    rows = images * rpi
    stress = kind in ("spike", "climb", "lowfirst")
    x = rng.standard_normal((rows, C_WIDTH))
    if kind == "lnstress":
        x = 50.0 + 0.5 * x
    x = x.astype(np.float16)
    gamma = (1 + 0.1 * rng.standard_normal(C_WIDTH)).astype(np.float32)
    beta = ((3.0 if stress else 0.1) * rng.standard_normal(C_WIDTH)).astype(np.float32)
    wq = rng.standard_normal((C_WIDTH, C_WIDTH)) / np.sqrt(C_WIDTH)
    if stress:
        bd = beta.astype(np.float64)
        for h in range(0, HEADS, 2):
            cs = slice(h * DHEAD, (h + 1) * DHEAD)
            wq[cs] -= np.outer(wq[cs] @ bd, bd) / (bd @ bd)
    wq = wq.astype(np.float16)
    wo = (rng.standard_normal((C_WIDTH, C_WIDTH)) * (1.8 / np.sqrt(C_WIDTH))).astype(np.float16)
    k = rng.standard_normal((images, L, C_WIDTH))
    v = rng.standard_normal((images, L, C_WIDTH))
    if stress:
        c = beta.astype(np.float64) @ wq.astype(np.float64).T                       # the constant part of q
        t = np.zeros(L)
        if kind == "spike":
            t[L - 2] = 30.0
        elif kind == "climb":
            t = 12.0 * (np.arange(L) // 32)
        else:
            t[:32] = -40.0
        unit = np.sqrt(DHEAD) / LOG2E                                                # one log2 unit of the scaled score
        for h in range(1, HEADS, 2):
            cs = slice(h * DHEAD, (h + 1) * DHEAD)
            k[:, :, cs] += (t[None, :, None] * unit) * (c[cs] / (c[cs] @ c[cs]))[None, None, :]
    lpad = (L + 63) // 64 * 64
    vt = np.full((images, C_WIDTH, lpad), 100.0 if poison else 0.0)
    vt[:, :, :L] = v.transpose(0, 2, 1)
    case = dict(x=x, gamma=gamma, beta=beta, wq=wq, wo=wo, bo=None, k=k.astype(np.float16), vt=vt.astype(np.float16), rpi=rpi, L=L,
                Lpad=lpad, images=images, name=f"{images}x{rpi} L{L} {kind}{'' if bias else ' nobias'}{' poison' if poison else ''}")
    if bias:
        # bo puts the mean of every column of the branch at +-(0.7 .. 1.5): with a single key, or a spike, (part of) the branch is the same
        # for every query, and a column that is one constant near zero would make the per-column relative error meaningless
        mean = (graph(case) - x.astype(np.float64)).mean(0)
        target = rng.uniform(0.7, 1.5, C_WIDTH) * rng.choice([-1.0, 1.0], C_WIDTH)
        case["bo"] = (target - mean).astype(np.float32)
    return case


# the GPU test's cases (tests/test_gpu_xattn_chain.py); the CPU tier checks that the twin passes the parity rule on each of them
GPU_CASES = (
    [dict(images=1, rpi=128, L=L, seed=100 + L) for L in (1, 32, 33, 77, 96, 154)]
    + [dict(images=3, rpi=256, L=77, seed=7), dict(images=3, rpi=256, L=33, seed=8, poison=True),
       dict(images=1, rpi=128, L=77, seed=9, kind="spike"), dict(images=1, rpi=128, L=154, seed=10, kind="climb"),
       dict(images=1, rpi=128, L=96, seed=11, kind="lowfirst"), dict(images=1, rpi=128, L=77, seed=12, kind="lnstress"),
       dict(images=1, rpi=128, L=77, seed=13, bias=False)])


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def worst_slices(got, ref, pool=1):
    """Largest rel-L2 over the rows and over the columns of a [rows][C] tensor (rows pooled in runs of `pool`)."""
    e2, r2 = (got - ref) ** 2, ref ** 2
    rows = np.sqrt(e2.reshape(-1, pool * e2.shape[1]).sum(-1) / r2.reshape(-1, pool * e2.shape[1]).sum(-1)).max()
    cols = np.sqrt(e2.sum(0) / r2.sum(0)).max()
    return float(rows), float(cols)


def parity(got, ref, twin, ctx):
    """The rule of tests/test_gpu_esrgan.py::assert_parity on a [rows][C] tensor: error <= 1.25 x yardstick on the tensor, <= 2 x 1.25 x
    yardstick on the worst row and the worst column, yardstick > 1e-4."""
    yard, err = rel_l2(twin, ref), rel_l2(got, ref)
    rows, cols = worst_slices(got, ref)
    print(f"[xattn_chain parity] {ctx}: error {err:.3e}  twin {yard:.3e}  worst row {rows:.3e}  worst column {cols:.3e}")
    assert np.isfinite(got).all(), ctx
    assert yard > 1e-4, (ctx, yard)
    assert err <= 1.25 * yard, (ctx, err, yard)
    assert rows <= 2 * 1.25 * yard, (ctx, "worst row", rows, yard)
    assert cols <= 2 * 1.25 * yard, (ctx, "worst column", cols, yard)


def assert_chain_parity(got, case, ref=None, twin=None):
    """Twice: on the output, and on the branch out - x1 (the residual dominates the output and would hide a wrong branch)."""
    ref = graph(case) if ref is None else ref
    twin = graph(case, twin=True) if twin is None else twin
    x = case["x"].astype(np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(x.shape)
    parity(got, ref, twin, case["name"] + " / output")
    parity(got - x, ref - x, twin - x, case["name"] + " / branch")
