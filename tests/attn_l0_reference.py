"""Cases and float64 references for the level-0 self-attention forms of csrc/attention.hip (test infrastructure, numpy only; shared by
tests/test_gpu_attn_l0_forms.py, tests/test_cpu_attn_l0_forms.py and tools/gpu/attn_l0_time.py).

Form 17 takes unscaled fp16 q, k and applies scale * log2(e) itself; form 27 takes q and k that already carry sqrt(scale * log2(e)) each,
applies no scale and addresses its full KV tiles without per-tile address arithmetic.  Handed the same pre-scaled operands, form 17 (scale
left to apply: 1) does the same arithmetic in the same order, so 27 must give its bits — which checks the staging; the numerics of
pre-scaling are held against float64 by form 17's own error on the unscaled twins.  A case holds both operand sets, made from the same
fp32 q, k — each rounded to fp16 ONCE — and the float64 softmax of each set's own rounded values.
"""
import numpy as np

D = 40
LOG2E = 1.4426950408889634
C_L0 = D ** -0.5 * LOG2E            # scale * log2(e) of a d = 40 head
ATTN_CAP = 5e-4                     # the project's cap for attention against fp32 / float64 (tests/test_gpu_ops.py)

# (name, B, H, N = M, stacked): the shortest sequence the default dispatch gives the folded forms (16 tiles), an odd tile count for the
# double buffer (17), and a ragged last tile of 40 keys + a ragged query block whose prefetch starts from a steady-state iteration (1064)
SHAPES = [(f"n{n}_{'stacked' if st else 'dense'}", b, h, n, st)
          for n in (1024, 1088, 1064) for (b, h, st) in ((1, 2, False), (2, 8, True))]


def rup(x, m):
    return (x + m - 1) // m * m


def make_case(B, H, N, stacked, seed=0, M=None, q=None, k=None, v=None):
    """fp32 q [B, N, H*D], k, v [B, M, H*D] (seeded normal unless given) -> dict with
         q16 / k16    unscaled fp16 operands (views into one [B, N, 2*H*D] tensor when `stacked`, as the engine lays q | k out)
         qs16 / ks16  the same fp32 values times sqrt(C_L0), rounded to fp16 once
         vt16         V^T [B, H*D, rup(M, 64)], zero padded
         ref / ref_s  float64 softmax attention of (q16, k16, scale) / of (qs16, ks16) in the log2 domain, [B, N, H*D]"""
    M = N if M is None else M
    assert not stacked or M == N
    C = H * D
    g = np.random.default_rng(seed)
    q = g.standard_normal((B, N, C), dtype=np.float32) if q is None else q.astype(np.float32)
    k = g.standard_normal((B, M, C), dtype=np.float32) if k is None else k.astype(np.float32)
    v = g.standard_normal((B, M, C), dtype=np.float32) if v is None else v.astype(np.float32)
    rs = np.float32(np.sqrt(C_L0))

    def pair(a, b):
        a, b = a.astype(np.float16), b.astype(np.float16)
        if not stacked:
            return a, b
        both = np.ascontiguousarray(np.concatenate([a, b], axis=2))
        return both[:, :, :C], both[:, :, C:]
    q16, k16 = pair(q, k)
    qs16, ks16 = pair(q * rs, k * rs)
    v16 = v.astype(np.float16)
    vt16 = np.zeros((B, C, rup(M, 64)), np.float16)
    vt16[:, :, :M] = v16.transpose(0, 2, 1)
    return dict(B=B, H=H, N=N, M=M, stacked=stacked, q16=q16, k16=k16, qs16=qs16, ks16=ks16, vt16=vt16,
                ref=softmax_attention(q16, k16, v16, H, D ** -0.5), ref_s=softmax_attention(qs16, ks16, v16, H, np.log(2.0)))


def softmax_attention(q, k, v, H, scale):
    """float64: softmax(scale * q k^T) v per head; scale = ln 2 evaluates 2^(q k^T) weights (operands in the log2 domain)."""
    B, N, C = q.shape
    sp = lambda t: t.astype(np.float64).reshape(B, t.shape[1], H, C // H).transpose(0, 2, 1, 3)
    s = np.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * scale
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("bhij,bhjd->bhid", p, sp(v)).transpose(0, 2, 1, 3).reshape(B, N, C)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def worst_row_rel_l2(got, ref):
    """Worst (batch, query row) of a [B, N, C] output."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    e = np.linalg.norm(got - ref, axis=2) / np.linalg.norm(ref, axis=2)
    i = np.unravel_index(np.argmax(e), e.shape)
    return float(e[i]), tuple(int(x) for x in i)


# ---- rows built against the shift bookkeeping (generators of tests/test_gpu_ops.py::test_attention_lazy_rebase_slack, d = 40, one head,
# 256 queries, 10 KV tiles): the first score column is set per key tile in log2 units, everything else is small noise -------------------
def adversarial_cases():
    n, m = 256, 640
    g = np.random.default_rng(151)
    q = np.zeros((1, n, D), np.float32)
    q[..., 0] = 1.0
    q[:, :, 1:] = 0.05 * g.standard_normal((1, n, D - 1), dtype=np.float32)
    scale = D ** -0.5
    tile = np.arange(m) // 64
    out = []
    # climbing by less than tau per tile (never re-based after the first tile), by more than tau per tile (re-based in every tile), with a
    # first tile far below zero (-60) in both; then falling scores
    for name, per_tile in (("climbs by 3 per tile", 3.0), ("climbs by 11 per tile", 11.0), ("falls by 5 per tile", -5.0)):
        k = 0.05 * g.standard_normal((1, m, D), dtype=np.float32)
        k[0, :, 0] = (per_tile * tile - (60.0 if per_tile > 0 else 0.0)) / (scale * LOG2E)
        out.append((name, make_case(1, 1, n, False, M=m, q=q, k=k, v=g.standard_normal((1, m, D), dtype=np.float32))))
    k = 0.05 * g.standard_normal((1, m, D), dtype=np.float32)
    k[0, 500, 0] = 40.0 / scale                          # one key 40 nats above the rest, in the 8th tile
    out.append(("late spike", make_case(1, 1, n, False, M=m, q=q, k=k, v=g.standard_normal((1, m, D), dtype=np.float32))))
    return out


def large_norm_key_case():
    """The spike row of tests/test_gpu_ops.py::test_attention_role_offset_kernel: key 500 = 6 x query 5 (384 queries, 576 keys, one head)."""
    g = np.random.default_rng(71)
    n, m = 384, 576
    q = g.standard_normal((1, n, D), dtype=np.float32)
    k = g.standard_normal((1, m, D), dtype=np.float32)
    v = g.standard_normal((1, m, D), dtype=np.float32)
    k[0, 500] = q[0, 5] * 6.0
    return make_case(1, 1, n, False, M=m, q=q, k=k, v=v), 5
