"""Shared test helpers (seeded inputs identical to tests/golden/make_golden.py)."""
import numpy as np
import torch


def seeded(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def seeded_module_weights(module, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if p.ndim >= 2:
                fan_in = int(np.prod(p.shape[1:]))
                p.copy_(torch.randn(p.shape, generator=g) * fan_in ** -0.5)
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.02 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))


def clip_tokens(batch, vocab, seed, length=77):
    """Token ids as the CLIP tokenizer lays them out, for a vocabulary whose two largest ids are BOS and EOS: BOS in column 0, random
    ids below them, then EOS to the end of the row from a column that differs per row (equal maximal ids in a row: the pooled row is
    taken at the FIRST of them) — except the last of several rows, whose only EOS is the last column."""
    bos, eos = vocab - 2, vocab - 1
    tok = torch.randint(0, bos, (batch, length), generator=torch.Generator(device="cpu").manual_seed(seed))
    tok[:, 0] = bos
    starts = (12, 60, 33, 45, 7, 70, 21, 52)
    assert batch <= len(starts) and length > max(starts)
    for b in range(batch):
        tok[b, (length - 1 if batch > 1 and b == batch - 1 else starts[b]):] = eos
    return tok


def rel_l2(a, b):
    a = torch.as_tensor(a).double().flatten()
    b = torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def usable_cpus(cap=32):
    """Hardware threads this process may use (affinity mask; os.cpu_count() reports the host's even on a restricted box, and
    oversubscribing the oracle's fp32 GEMMs is pathological), capped where they stop scaling."""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(cap, n))


def worst_slice_rel_l2(got, ref, keep_dims, min_elems=64):
    """-> (worst, index): the largest ||got - ref|| / ||ref|| over the slices indexed by the dimensions `keep_dims` (every other dimension
    is reduced), in float64, and the index of that slice along the kept dimensions.  One global rel_l2 cannot see a single wrong row of a
    large tensor; this can.  Slices of fewer than `min_elems` elements are pooled with their neighbours along the LAST kept dimension (whole
    runs of ceil(min_elems / size) consecutive indices, a remainder joining the last run; a dimension too short for that is pooled whole and
    the pooling goes on along the kept dimension before it): the error of a 40-element slice fluctuates too much to be capped tightly.
    The index of a pooled slice is that of its first member."""
    got = torch.as_tensor(got).double()
    ref = torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    keep = [d % ref.ndim for d in keep_dims]
    assert len(set(keep)) == len(keep) and keep
    rest = [d for d in range(ref.ndim) if d not in keep]
    kshape = [ref.shape[d] for d in keep]
    err2 = ((got - ref) ** 2).permute(keep + rest).reshape(kshape + [-1]).sum(-1)
    ref2 = (ref ** 2).permute(keep + rest).reshape(kshape + [-1]).sum(-1)
    size = ref.numel() // max(1, err2.numel())
    step = [1] * len(keep)                                     # index scale per kept dimension after pooling
    d = len(keep) - 1
    while size < min_elems and d >= 0:
        length = err2.shape[d]
        run = min(length, -(-min_elems // size))
        groups = length // run

        def pool(t):
            t = t.movedim(d, -1)
            main = t[..., :groups * run].reshape(t.shape[:-1] + (groups, run)).sum(-1)
            main[..., -1] += t[..., groups * run:].sum(-1)
            return main.movedim(-1, d)
        err2, ref2 = pool(err2), pool(ref2)
        step[d], size, d = run, size * run, d - 1
    ratio = (err2 / (ref2 + 1e-60)).sqrt()
    flat = int(ratio.argmax())
    idx = np.unravel_index(flat, tuple(ratio.shape))
    return float(ratio.flatten()[flat]), tuple(int(i) * s for i, s in zip(idx, step))
