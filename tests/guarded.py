"""Guarded memory for the kernel tests: every operand between two guard bands, every scratch buffer exactly the size asked for.

A plain module (like golden_cases.py), used by tests/test_gpu_memory_bounds.py and by the CPU-tier controls in
tests/test_guarded_harness.py.

    arena = Arena(ws_fill="nan")
    x = arena.guarded_copy(x0, "x")                  # an input between guard bands
    with arena.installed(monkeypatch):               # ops._empty / ops._zeros / ops._workspace allocate guarded buffers
        y = ops.something(x, ...)
    torch.cuda.synchronize()
    arena.check_guards()                             # every guard band bit-identical to its fill

Layout of one guarded buffer:  [GUARD bytes of fill | the view, nbytes | GUARD bytes of fill].  The allocation comes from torch's
caching allocator (512-byte aligned), GUARD is a multiple of 256, so the view starts 256-byte aligned and the tail guard starts at
the byte after its last element (no rounding gap).

Fills.  Floating tensors: a quiet-NaN bit pattern no kernel produces, chosen to stay NaN through the bf16 rounding of
csrc/ipsr_common.h (f2bf adds 0x7fff + lsb, which turns a NaN with payload in the low half only into Inf / 0): fp32 0x7fc05a5a,
bf16 0x7fc1.  Integer tensors (index lists, counts, masks): 0, a valid index — a kernel reading past an index array is then
caught by comparing results, never handed a wild index.  Workspaces: guards of 0 bytes; the interior is `ws_fill` ("nan": the
fp32 pattern, only for workspaces audited to hold floats alone; "zero"; "stale": the bytes the production workspace cache holds,
i.e. what an earlier call of another shape left there).
"""
import contextlib

import torch

GUARD = 4096
NAN32 = 0x7fc05a5a
NAN16 = 0x7fc1

_INT_VIEW = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}


def fill_bits(dtype):
    """The guard word of a dtype, as an integer of the same width."""
    if dtype == torch.float32:
        return NAN32                        # (below 2**31: the same bits as an int32)
    if dtype == torch.bfloat16:
        return NAN16
    return 0


def _bits(t):
    """The integer view of a tensor's bytes (same element width)."""
    return t.view(_INT_VIEW[t.element_size()])


class Arena:
    def __init__(self, ws_fill="nan", device="cuda"):
        self.ws_fill = ws_fill
        self.device = torch.device(device)
        self.buffers = []               # (name, raw, lo, hi, guard word)
        self.workspaces = []            # (nbytes, view)
        self.n_alloc = 0

    # ---- allocation -------------------------------------------------------------------------------------------------------------
    def _raw(self, n, dtype, name, word, interior=None, device=None):
        es = torch.empty((), dtype=dtype).element_size()
        g = GUARD // es
        raw = torch.empty(2 * g + n, dtype=dtype, device=device or self.device)
        _bits(raw).fill_(word)
        if interior is not None:
            _bits(raw[g:g + n]).fill_(interior)
        self.buffers.append((name, raw, g, g + n, word))
        return raw[g:g + n]

    def guarded(self, shape, dtype, fill=None, name=None, device=None):
        """A contiguous tensor of `shape` inside a guarded allocation.  fill: None = the guard word (NaN for floats: an output that
        must be fully written), "zero", or a tensor to copy in."""
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = 1
        for s in shape:
            n *= int(s)
        self.n_alloc += 1
        name = name or "alloc%d%s" % (self.n_alloc, list(shape))
        word = fill_bits(dtype)
        v = self._raw(n, dtype, name, word, 0 if fill == "zero" else None, device)
        v = v.view(shape)
        if torch.is_tensor(fill):
            v.copy_(fill)
        return v

    def guarded_copy(self, t, name):
        return self.guarded(t.shape, t.dtype, t, name, t.device)

    # the replacements of ops._empty / ops._zeros / ops._workspace
    def empty(self, shape, dtype, device):
        return self.guarded(shape, dtype, None, device=device)

    def zeros(self, shape, dtype, device):
        return self.guarded(shape, dtype, "zero", device=device)

    def workspace(self, nbytes, device):
        nbytes = int(nbytes)
        self.n_alloc += 1
        v = self._raw(nbytes, torch.uint8, "workspace%d[%d B]" % (self.n_alloc, nbytes), 0, device=device)
        if self.ws_fill == "nan" and nbytes >= 4:
            v[:nbytes // 4 * 4].view(torch.int32).fill_(NAN32)
        elif self.ws_fill == "stale":
            from deepinpainting_amd import ops
            old = [b for b in ops._ws_cache.values() if b.device == v.device]
            if old and old[0].numel() >= nbytes:
                v.copy_(old[0][:nbytes])
        self.workspaces.append((nbytes, v))
        return v

    @contextlib.contextmanager
    def installed(self, monkeypatch):
        from deepinpainting_amd import ops
        with monkeypatch.context() as m:
            m.setattr(ops, "_empty", self.empty)
            m.setattr(ops, "_zeros", self.zeros)
            m.setattr(ops, "_workspace", self.workspace)
            yield self

    # ---- checks -----------------------------------------------------------------------------------------------------------------
    def guard_bytes(self):
        return sum((lo + raw.numel() - hi) * raw.element_size() for _, raw, lo, hi, _ in self.buffers)

    def check_guards(self):
        """Every guard band bit-identical to its fill; raises AssertionError naming the buffer, the side and the first changed
        offset (in elements from the band's start)."""
        bad = []
        for name, raw, lo, hi, word in self.buffers:
            b = _bits(raw)
            for side, band in (("head", b[:lo]), ("tail", b[hi:])):
                diff = (band != word).nonzero()
                if diff.numel():
                    off = int(diff[0]) if side == "tail" else int(diff[-1]) - lo
                    bad.append("%s: %s guard changed at element %+d (%d elements differ)" % (name, side, off, diff.numel()))
        assert not bad, "; ".join(bad)
