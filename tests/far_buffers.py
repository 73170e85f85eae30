"""Operands whose element offsets pass 2^31 (and whose byte offsets pass 2^32), for tests of the kernels' address arithmetic.

A `FarBuffer` is ONE allocation of zeros that holds, in this order,
  * a front slack of 2^31 elements,
  * the tensor: element (z, r, c) at z * bs + r * ld + c from the base, the whole span below 2^32 elements,
  * 64 trailing elements.
On the device the zeros are one torch.zeros, a memset of a few milliseconds.  Under the host emulation the "device" is host memory and
torch.zeros would write all of it (9 GB resident per buffer); there the allocation is an anonymous mapping, whose pages are zero until
somebody writes them, and `untouched()` reads only the pages that mincore reports resident — the stored rows and whatever a kernel wrote.
(A page of an anonymous mapping that is not resident has never been written on a machine without swap; with swap configured the whole
mapping is read.)

Why this layout: a kernel is handed the base and strides with which every offset it has to form is non-negative and below 2^32 elements.
Each way of getting such an offset wrong then lands INSIDE the allocation, where it is seen and faults nothing:
  * an element index kept in 32 signed bits comes out at most 2^31 elements too low: not below the start of the slack;
  * a byte offset kept in 32 signed bits comes out at most 2^32 bytes = 2^31 fp16 (2^30 fp32) elements too low: inside the slack too;
  * an unsigned 32-bit index or byte offset wraps to a smaller non-negative one: inside the span;
  * a 24-bit multiply (__umul24) drops high bits of a factor: a smaller non-negative product, inside the span.
A read that went astray returns zeros (the slack and the gaps) or another row, and the result is wrong by the size of the operand, which
every float64 rule of the suite sees; a write that went astray leaves a non-zero word where `untouched()` looks.  Neither is a GPU
fault.  The argument needs the span to stay below 2^32 elements: the constructor refuses anything else, and no case may relax that.

Inputs are seeded data without exact zeros in the stored part (`fill` checks), so that "read zeros" can never agree with "read the row".
One far operand per case; everything else stays small and dense, so a failure names the address computation that is wrong."""
import ctypes
import mmap

import numpy as np
import torch

SLACK = 1 << 31                 # elements in front of the tensor
TAIL = 64                       # elements behind it
CHUNK = 1 << 26                 # elements per reduction of `untouched()`: no index of one torch call gets near 2^31, its temporaries stay small


class FarBuffer:
    def __init__(self, rows, cols, ld, dtype, dev, batch=1, bs=0):
        assert dtype in (torch.float16, torch.float32)
        assert ld >= cols and (batch == 1 or bs >= rows * ld)
        self.geom = (batch, rows, cols, ld, bs)
        self.span = (batch - 1) * bs + (rows - 1) * ld + cols
        assert self.span < (1 << 32), "a stored span of 2^32 elements or more lets a wrapped access leave the allocation"
        n = SLACK + self.span + TAIL
        self.map = None
        if torch.device(dev).type == "cpu":                             # the host emulation
            self.map = mmap.mmap(-1, n * (2 if dtype == torch.float16 else 4))
            self.full = torch.frombuffer(self.map, dtype=dtype)
        else:
            self.full = torch.zeros(n, dtype=dtype, device=dev)
        self.addr = self.full.data_ptr() + SLACK * self.full.element_size()
        self.nbytes = self.full.numel() * self.full.element_size()
        self.stored = torch.as_strided(self.full, (batch, rows, cols), (bs, ld, 1), SLACK)

    def fill(self, dense, col0=0, zero_columns=False):
        """dense [batch, rows, n] -> columns col0 .. col0 + n - 1 of the stored elements (through the strided view, on the device): the
        whole tensor, or one column block of several operands that share the rows.  No exact zeros; with zero_columns a column may be
        zero as a whole (the zero tails of 32-wide head slots), every other column holds none."""
        batch, rows, cols = self.geom[:3]
        dense = dense.reshape(batch, rows, -1).to(self.full.dtype)
        assert col0 + dense.shape[2] <= cols
        per_column = torch.count_nonzero(dense.reshape(-1, dense.shape[2]), dim=0)
        full = per_column == batch * rows
        assert bool((full | (per_column == 0)).all() if zero_columns else full.all()), "an input with exact zeros could hide a read that went astray"
        assert bool(full.any())
        self.stored[:, :, col0:col0 + dense.shape[2]].copy_(dense.to(self.full.device))
        return self

    def at(self, col0):
        """The address of column col0 of row 0: the base of a column block."""
        return self.addr + col0 * self.full.element_size()

    def read(self):
        """The stored elements [batch, rows, cols], on the CPU."""
        return self.stored.cpu().clone()

    def untouched(self, what=""):
        """Every element of the allocation outside the stored ones is still +0 bit for bit, the slack and the tail included.  Counted, not
        masked: the non-zero words of the whole allocation (chunk by chunk, reduced where the buffer lives) against those of the stored part."""
        ints = self.full.view(torch.int16 if self.full.dtype == torch.float16 else torch.int32)
        total = 0
        first = None
        for a, b in ([(0, ints.numel())] if self.map is None else resident_runs(ints)):
            for lo in range(a, b, CHUNK):
                n = int(torch.count_nonzero(ints[lo:min(lo + CHUNK, b)]))
                if n and first is None:
                    first = lo
                total += n
        batch, rows, cols, ld, bs = self.geom
        inside = int(torch.count_nonzero(torch.as_strided(ints, (batch, rows, cols), (bs, ld, 1), SLACK)))
        assert total == inside, (what, "words outside the stored layout were written", total - inside, "first non-zero chunk starts at element", first,
                                 "the tensor at", SLACK)

    def free(self):
        self.full = self.stored = self.map = None                      # (the mapping goes with its last tensor)
        torch.cuda.empty_cache()


def resident_runs(t):
    """[(first, last + 1)] element ranges of the resident pages of a host tensor; everything, if that cannot be told or swap exists."""
    everything = [(0, t.numel())]
    try:
        if any(ln.startswith("SwapTotal:") and int(ln.split()[1]) > 0 for ln in open("/proc/meminfo")):
            return everything
        libc = ctypes.CDLL(None, use_errno=True)
        page, size = mmap.PAGESIZE, t.element_size()
        lo = t.data_ptr() // page * page
        npages = (t.data_ptr() + t.numel() * size - lo + page - 1) // page
        vec = (ctypes.c_ubyte * npages)()
        if libc.mincore(ctypes.c_void_p(lo), ctypes.c_size_t(npages * page), vec) != 0:
            return everything
    except (OSError, AttributeError):
        return everything
    res = np.frombuffer(vec, dtype=np.uint8) & 1
    edges = np.flatnonzero(np.diff(np.concatenate(([0], res, [0]))))
    runs = []
    for a, b in zip(edges[::2].tolist(), edges[1::2].tolist()):
        first, last = max(0, (lo + a * page - t.data_ptr()) // size), min(t.numel(), (lo + b * page - t.data_ptr() + size - 1) // size)
        runs.append((first, last))
    return runs
