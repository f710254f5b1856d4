"""Memory-edge helpers for the kernel tests (tests/test_edges_gpu.py, tests/test_guard_cpu.py).  Not a conftest: plain functions only.

A kernel's contract names the elements it may read as values and the elements it may write.  These helpers put both inside a larger
*arena* so that a violation shows instead of passing by luck:

  embed(t, ...)         copies an operand into an arena pre-filled with POISON (NaN for floats, 0x7F for e4m3 bytes, 0xFF for E8M0
                        scales) and returns the strided view of it: leading-dimension padding, rows past the last row, gaps between
                        batches, everything before the first and after the last element hold poison.  A kernel that lets one of these
                        reach its result produces a non-finite (or grossly wrong) output.
  sentinel_out(...)     an output view inside an arena filled with a fixed bit pattern that no test output produces (fp16 0x7DDD,
                        fp32 0x7FC0DEAD, bytes 0xA5, int32 0x5EADBEE5).
  assert_untouched      every arena element outside the view still holds that pattern, compared as INTEGERS (the float patterns are
                        NaNs: NaN != NaN as floats); a failure names the first and last touched element as (batch, row, column)
                        relative to the view (row -1 = before the view, column >= cols = the leading-dimension padding).
  assert_fully_written  no element of the view still holds the pattern (a skipped ragged tile).

Layout of an arena of a [batch, rows, cols] view (a 2-D view is batch 1, a 1-D one a single row):

  | head | batch 0: (rows + row_pad) x ld | batch 1 ... | tail |      ld = cols + col_pad rounded up to the alignment

head, ld and the batch stride are multiples of `ALIGN_ELEMS[dtype]` elements (8 fp16, 8 fp32, 16 bytes: the 16-byte / 8-element
alignment the entry points ask for), and the arena itself comes from torch's allocator (>= 64-byte aligned), so every view starts
16-byte aligned with aligned rows.  The default tail covers the largest overshoot a tile can make - 256 rows of `ld` elements past
the last row, capped at TAIL_CAP_BYTES - so that a store past the end lands in the arena, in owned memory, and not outside the allocation.
"""
from __future__ import annotations

import torch

ALIGN_ELEMS = {torch.float16: 8, torch.float32: 8, torch.uint8: 16, torch.int32: 8}
_INT_OF = {torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32}
# the signed integer each pattern reads as in _INT_OF[dtype]
SENTINEL_BITS = {torch.float16: 0x7DDD, torch.float32: 0x7FC0DEAD, torch.uint8: 0xA5, torch.int32: 0x5EADBEE5}
POISON_BITS = {torch.float16: 0x7E00, torch.float32: 0x7FC00000, torch.uint8: 0x7F}       # quiet NaN, quiet NaN, e4m3 NaN (S.1111.111)
E8M0_POISON = 0xFF                                                                       # the NaN encoding of an E8M0 scale
TAIL_ROWS = 256                      # the tallest tile of any kernel here
TAIL_CAP_BYTES = 4 << 20


def _up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def bits(t: torch.Tensor) -> torch.Tensor:
    """t reinterpreted as integers of the same width (same storage)."""
    return t.view(_INT_OF[t.dtype])


def _fill_bits(arena: torch.Tensor, pattern: int) -> None:
    bits(arena).fill_(pattern)                                        # every pattern here is below 2^(width - 1): no sign wrap


def _geometry(shape, dtype, row_pad, col_pad, head, tail):
    """(batch, rows, cols, ld, bs, head, tail) in elements."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 1:
        batch, rows, cols = 1, 1, shape[0]
    elif len(shape) == 2:
        batch, (rows, cols) = 1, shape
    elif len(shape) == 3:
        batch, rows, cols = shape
    else:
        raise ValueError(f"guard: 1-D, 2-D or 3-D shapes only (flatten the leading dims of a contiguous tensor), got {shape}")
    if min(batch, rows, cols) <= 0 or row_pad < 0 or col_pad < 0:
        raise ValueError(f"guard: empty shape or negative padding ({shape}, row_pad {row_pad}, col_pad {col_pad})")
    a = ALIGN_ELEMS[dtype]
    ld = cols if len(shape) == 1 else _up(cols + col_pad, a)
    bs = (rows + row_pad) * ld
    item = torch.empty((), dtype=dtype).element_size()
    span = ld if len(shape) > 1 else min(cols, 4096)      # a flat tensor has no rows: guard it like rows of at most 4096 elements
    if head is None:
        head = 2 * span + 64
    if tail is None:
        tail = min(TAIL_ROWS * span + 256, TAIL_CAP_BYTES // item)
    return batch, rows, cols, ld, bs, _up(head, a), _up(tail, a)


def _carve(shape, dtype, device, row_pad, col_pad, head, tail, pattern):
    batch, rows, cols, ld, bs, head, tail = _geometry(shape, dtype, row_pad, col_pad, head, tail)
    arena = torch.empty(head + batch * bs + tail, dtype=dtype, device=device)
    _fill_bits(arena, pattern)
    nd = len(tuple(shape))
    size, stride = {1: ((cols,), (1,)), 2: ((rows, cols), (ld, 1)), 3: ((batch, rows, cols), (bs, ld, 1))}[nd]
    return torch.as_strided(arena, size, stride, head), arena


def embed(t: torch.Tensor, *, row_pad: int = 0, col_pad: int = 0, head=None, tail=None, poison=None, device=None):
    """(view, arena): t copied into a poisoned arena (module docstring).  poison: None = the dtype's NaN pattern (POISON_BITS), a float =
    that value (e.g. inf or 6e4 where a path launders NaN), an int with a uint8 tensor = that byte.  A tensor of more than 3 dims
    (contiguous by the entry points' contract) is embedded flat, poison before its first and after its last element only, and returned
    in its own shape."""
    device = t.device if device is None else device
    shape = tuple(t.shape)
    flat = t.dim() > 3
    if flat:
        if row_pad or col_pad:
            raise ValueError("guard.embed: a tensor of more than 3 dims is contiguous by contract: no row / column padding")
        shape = (t.numel(),)
    if poison is None or (t.dtype == torch.uint8 and isinstance(poison, int)):
        view, arena = _carve(shape, t.dtype, device, row_pad, col_pad, head, tail, POISON_BITS[t.dtype] if poison is None else poison)
    else:
        view, arena = _carve(shape, t.dtype, device, row_pad, col_pad, head, tail, 0)
        arena.fill_(float(poison))
    view.copy_(t.reshape(shape).to(device))
    return (view.view(t.shape) if flat else view), arena


def sentinel_out(shape, *, row_pad: int = 0, col_pad: int = 0, head=None, tail=None, dtype=torch.float16, device="cpu"):
    """(view, arena): an output of `shape` (1-D, 2-D or [batch, rows, cols]) inside an arena filled with SENTINEL_BITS[dtype]."""
    return _carve(shape, dtype, device, row_pad, col_pad, head, tail, SENTINEL_BITS[dtype])


def _offset(arena: torch.Tensor, view: torch.Tensor) -> int:
    off = view.storage_offset() - arena.storage_offset()
    if view.untyped_storage().data_ptr() != arena.untyped_storage().data_ptr() or view.dtype != arena.dtype or off < 0:
        raise ValueError("guard: the view does not live in this arena")
    return off


def _owned(arena: torch.Tensor, view: torch.Tensor) -> torch.Tensor:
    own = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
    torch.as_strided(own, tuple(view.shape), tuple(view.stride()), _offset(arena, view)).fill_(True)
    return own


def locate(arena: torch.Tensor, view: torch.Tensor, index: int):
    """(batch, row, column) of arena element `index` relative to a 1-D / 2-D / 3-D view with unit inner stride: row -1, -2, ... lie before
    the view's first row, rows >= view rows after its last, columns >= view columns in the leading-dimension padding."""
    off = index - _offset(arena, view)
    if view.dim() == 1 or view.dim() > 3:                 # flat: row 0 holds the numel() elements, column = the linear offset
        return 0, (0 if 0 <= off < view.numel() else (-1 if off < 0 else 1)), off
    ld = view.stride(-2)
    if view.dim() == 2:
        return 0, off // ld, off % ld
    bs = view.stride(0)
    b = min(max(off // bs, 0), view.shape[0] - 1)
    off -= b * bs
    return b, off // ld, off % ld


def touched(arena: torch.Tensor, view: torch.Tensor, pattern=None):
    """Sorted arena indices outside `view` whose bits differ from the fill pattern (default: the dtype's sentinel)."""
    pattern = SENTINEL_BITS[arena.dtype] if pattern is None else pattern
    bad = (bits(arena) != pattern) & ~_owned(arena, view)
    return torch.nonzero(bad).flatten().cpu()


def assert_untouched(arena: torch.Tensor, view: torch.Tensor, what: str = "", pattern=None) -> None:
    """Every arena element outside `view` still holds the fill pattern bit for bit."""
    idx = touched(arena, view, pattern)
    if idx.numel():
        first, last = locate(arena, view, int(idx[0])), locate(arena, view, int(idx[-1]))
        raise AssertionError(f"{what}: {idx.numel()} element(s) outside the {tuple(view.shape)} output were written: first at "
                             f"(batch, row, column) = {first}, last at {last} (leading dim {view.stride(-2) if view.dim() > 1 else view.shape[0]})")


def assert_fully_written(view: torch.Tensor, what: str = "") -> None:
    """No element of the view still holds the sentinel (a tile that was skipped leaves it)."""
    left = bits(view) == SENTINEL_BITS[view.dtype]
    n = int(left.sum())
    if n:
        first = torch.nonzero(left)[0].tolist()
        raise AssertionError(f"{what}: {n} element(s) of the {tuple(view.shape)} output were never written, first at index {tuple(first)}")


def assert_aligned(view: torch.Tensor, what: str = "") -> None:
    """The view starts on 16 bytes and its row and batch strides are multiples of ALIGN_ELEMS[dtype] elements."""
    a = ALIGN_ELEMS[view.dtype]
    assert view.data_ptr() % 16 == 0, f"{what}: view starts at {view.data_ptr():#x}, not 16-byte aligned"
    assert view.stride(-1) == 1, f"{what}: inner stride {view.stride(-1)}"
    for s in view.stride()[:-1]:
        assert s % a == 0, f"{what}: stride {s} is not a multiple of {a} elements"
