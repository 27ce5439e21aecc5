"""Guard bands around the buffers handed to the op-level entry points (test_ops_guards_gpu.py).

A store past the end (or before the start) of an output lands in whatever the caching allocator put
next to it: no fault, no compared value changes.  `guarded` turns such a store into a comparison:
the buffer is the middle of one flat allocation whose two ends hold a fixed bit pattern, compared as
integers after the call.  `Inputs` does the same for what a kernel may only read."""
import torch

PATTERN = 0x5A          # every guard byte; as fp32 0x5A5A5A5A = 1.5368e16, as bf16 / fp16 finite too
MIN_GUARD_BYTES = 4096
ALIGN = 16              # the ABI's pointer alignment; guards are whole multiples of it


def guard_elems(dtype, elems=0):
    """guard length in elements of `dtype`: at least `elems`, at least 4096 bytes, a multiple of 16
    bytes so that the guarded view keeps the allocation's alignment"""
    size = torch.empty((), dtype=dtype).element_size()
    nbytes = max(int(elems) * size, MIN_GUARD_BYTES)
    nbytes = (nbytes + ALIGN - 1) // ALIGN * ALIGN
    return nbytes // size


def _first_hit(band):
    bad = (band != PATTERN).nonzero()
    return None if bad.numel() == 0 else int(bad[0])


def guarded(numel, dtype=torch.float32, fill=float("nan"), guard=0, name="buffer", device="cuda"):
    """One flat allocation [G | numel | G]; returns (view of the middle, check).  `guard` = the
    largest block a kernel of the family stores in one go, in elements (raised to 4096 bytes).
    `fill` initialises the view (None: left as the pattern).  check() asserts both bands still hold
    the pattern bit for bit and names the buffer, the side and the first byte offset hit."""
    numel = int(numel)
    size = torch.empty((), dtype=dtype).element_size()
    G = guard_elems(dtype, guard)
    raw = torch.full(((2 * G + numel) * size,), PATTERN, dtype=torch.uint8, device=device)
    flat = raw.view(dtype)
    view = flat[G:G + numel]
    assert view.data_ptr() % ALIGN == 0
    if fill is not None and numel:
        view.fill_(fill)

    def check():
        torch.cuda.synchronize()
        lo, hi = raw[:G * size], raw[(G + numel) * size:]
        at = _first_hit(hi)
        assert at is None, f"{name}: written past its end, first at byte +{at} after the buffer " \
                           f"({numel} elements of {dtype})"
        at = _first_hit(lo)
        assert at is None, f"{name}: written before its start, first at byte -{G * size - at} " \
                           f"({numel} elements of {dtype})"

    return view, check


def guarded_rows(rows, cols, ld, dtype=torch.float32, fill=float("nan"), guard=0, name="matrix"):
    """A [rows][cols] matrix with row pitch ld > cols inside guards: the pad columns hold the pattern
    too.  Returns (pitched [rows, ld] view, logical [rows, cols] view, check)."""
    flat, check_ends = guarded(rows * ld, dtype, None, guard, name)
    full = flat.view(rows, ld)
    logical = full[:, :cols]
    if fill is not None:
        logical.fill_(fill)
    size = flat.element_size()

    def check():
        check_ends()
        pad = full[:, cols:].contiguous().view(torch.uint8)
        at = _first_hit(pad.flatten())
        assert at is None, f"{name}: pad columns written, first in row {at // ((ld - cols) * size)}"

    return full, logical, check


class Inputs:
    """Snapshot of the `const` inputs of a call: clone() before, torch.equal on the byte views after
    a synchronise."""

    def __init__(self, **tensors):
        self.live = {k: t for k, t in tensors.items() if t is not None}
        self.saved = {k: t.clone() for k, t in self.live.items()}

    def check(self):
        torch.cuda.synchronize()
        for k, t in self.live.items():
            a = t.contiguous().view(-1).view(torch.uint8)
            b = self.saved[k].contiguous().view(-1).view(torch.uint8)
            assert torch.equal(a, b), f"const input `{k}` was modified by the call"


def all_finite(t, name="output"):
    """every element written: the buffer was NaN before the call"""
    assert bool(torch.isfinite(t.float()).all()), f"{name}: elements left unwritten (NaN) or not finite"
