"""tests/guard.py is not vacuous: with torch CPU functions standing in for kernels, a correct op passes and each planted violation -
a read one column into the padding, one row past M, a store one element / one 16-byte vector past N or past the last row - fails
and names where."""
import re

import pytest
import torch

import guard


def _linear(a_view, w_view, out_view):
    """The 'kernel': out = a @ w^T through raw strided views (reads only the logical extents)."""
    out_view.copy_((a_view.float() @ w_view.float().t()).half())


def _operands(M=13, N=24, K=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).half(), torch.randn(N, K, generator=g).half()


def _wider(arena, view, rows, cols):
    """The view a buggy kernel uses: same origin and strides, other extents."""
    return torch.as_strided(arena, (rows, cols), tuple(view.stride()), view.storage_offset() - arena.storage_offset())


def test_correct_op_passes_all_four_checks():
    a, w = _operands()
    av, _ = guard.embed(a, row_pad=3, col_pad=8)
    wv, _ = guard.embed(w, row_pad=2, col_pad=16)
    out, arena = guard.sentinel_out((13, 24), row_pad=2, col_pad=8)
    _linear(av, wv, out)
    assert torch.equal(out, (a.float() @ w.float().t()).half())            # padding changes no bit
    guard.assert_untouched(arena, out, "linear")
    guard.assert_fully_written(out, "linear")
    assert torch.isfinite(out.float()).all()


def test_read_one_column_into_the_padding_is_seen():
    a, w = _operands()
    av, aa = guard.embed(a, col_pad=8)
    wv, wa = guard.embed(w, col_pad=8)
    out, _ = guard.sentinel_out((13, 24), col_pad=8)
    _linear(_wider(aa, av, 13, 17), _wider(wa, wv, 24, 17), out)             # K + 1 columns of both operands
    assert not torch.isfinite(out.float()).any(), "poison in the leading-dimension padding must reach every output"


def test_read_one_row_past_m_is_seen():
    a, w = _operands()
    av, aa = guard.embed(a, row_pad=1)
    out, _ = guard.sentinel_out((14, 24))
    _linear(_wider(aa, av, 14, 16), w, out)                                   # row M of A
    got = out.float()
    assert torch.isfinite(got[:13]).all() and not torch.isfinite(got[13]).any()


def test_read_before_the_first_and_after_the_last_element_is_seen():
    x = torch.randn(2, 3, 4, 8, generator=torch.Generator().manual_seed(1)).half()     # a contiguous NHWC tensor
    xv, xa = guard.embed(x)
    assert xv.shape == x.shape and xv.is_contiguous() and torch.equal(xv, x)
    off = xv.storage_offset()
    assert torch.isnan(xa[off - 1].float()) and torch.isnan(xa[off + x.numel()].float())
    assert torch.isfinite(xa[off:off + x.numel()].float()).all()


@pytest.mark.parametrize("where,rows,cols,first,last", [
    ("one element past N", 13, 25, (0, 0, 24), (0, 12, 24)),
    ("one 16-byte vector past N", 13, 32, (0, 0, 24), (0, 12, 31)),
    ("one row past M", 14, 24, (0, 13, 0), (0, 13, 23)),
])
def test_store_outside_the_output_names_the_location(where, rows, cols, first, last):
    a, w = _operands()
    out, arena = guard.sentinel_out((13, 24), row_pad=2, col_pad=8)
    _wider(arena, out, rows, cols).fill_(1.0)                                  # the overshooting store
    guard.assert_fully_written(out, where)
    with pytest.raises(AssertionError) as e:
        guard.assert_untouched(arena, out, where)
    msg = str(e.value)
    assert f"first at (batch, row, column) = {first}" in msg and f"last at {last}" in msg, msg


def test_store_one_element_before_the_view_and_past_the_last_row_of_a_batch():
    out, arena = guard.sentinel_out((2, 5, 8), row_pad=1, col_pad=8, dtype=torch.float32)
    off, (bs, ld, _) = out.storage_offset(), out.stride()
    arena[off - 1] = 0.0
    with pytest.raises(AssertionError, match=re.escape("first at (batch, row, column) = (0, -1, 15)")):
        guard.assert_untouched(arena, out, "before")
    guard.bits(arena)[off - 1] = guard.SENTINEL_BITS[torch.float32]
    guard.assert_untouched(arena, out, "restored")
    arena[off + bs + 5 * ld] = 0.0                                             # row 5 of batch 1: its row padding
    with pytest.raises(AssertionError, match=re.escape("(1, 5, 0)")):
        guard.assert_untouched(arena, out, "batch gap")


def test_skipped_tile_is_seen():
    out, arena = guard.sentinel_out((13, 24), col_pad=8)
    out[:8].fill_(0.5)                                                         # the ragged last tile (rows 8 .. 12) never stored
    guard.assert_untouched(arena, out, "skipped tile")
    with pytest.raises(AssertionError, match=re.escape("first at index (8, 0)")):
        guard.assert_fully_written(out, "skipped tile")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8, torch.int32])
def test_integer_compare_survives_nan_sentinels(dtype):
    out, arena = guard.sentinel_out((3, 10), row_pad=1, col_pad=3, dtype=dtype)
    if dtype.is_floating_point:
        assert torch.isnan(arena).all() and not (arena == arena).any()         # as floats every element differs from itself
    guard.assert_untouched(arena, out, "fresh arena")                          # ... as integers nothing was touched
    assert (guard.bits(arena) == guard.SENTINEL_BITS[dtype]).all()
    with pytest.raises(AssertionError):
        guard.assert_fully_written(out, "fresh arena")
    # a NaN with OTHER bits written outside the view is a touch
    if dtype.is_floating_point:
        arena[-1] = float("nan")
        assert guard.bits(arena)[-1] != guard.SENTINEL_BITS[dtype]
        with pytest.raises(AssertionError):
            guard.assert_untouched(arena, out, "foreign NaN")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8])
@pytest.mark.parametrize("shape,row_pad,col_pad", [((5,), 0, 0), ((7, 40), 0, 0), ((7, 40), 3, 1), ((333, 100), 1, 4), ((3, 9, 24), 2, 8),
                                                   ((1, 1, 8), 0, 0), ((2, 130, 4), 1, 0)])
def test_alignment_of_every_view(dtype, shape, row_pad, col_pad):
    a = guard.ALIGN_ELEMS[dtype]
    for view, arena in (guard.sentinel_out(shape, row_pad=row_pad, col_pad=col_pad, dtype=dtype),
                        guard.embed(torch.ones(shape).to(dtype), row_pad=row_pad, col_pad=col_pad)):
        guard.assert_aligned(view, str(shape))
        assert tuple(view.shape) == shape and view.storage_offset() % a == 0
        if len(shape) > 1:
            assert view.stride(-2) >= shape[-1] + col_pad
        if len(shape) == 3:
            assert view.stride(0) >= (shape[1] + row_pad) * view.stride(1)
        # the tail covers a 256-row tile at this leading dimension (or the cap)
        end = view.storage_offset() + (view.stride(0) * (shape[0] - 1) if len(shape) == 3 else 0) + \
            (view.stride(-2) * (shape[-2] + row_pad) if len(shape) > 1 else shape[0])
        ld = view.stride(-2) if len(shape) > 1 else shape[0]
        assert arena.numel() - end >= min(guard.TAIL_ROWS * ld, guard.TAIL_CAP_BYTES // arena.element_size())


def test_poison_values():
    x = torch.ones(4, 8).half()
    v, a = guard.embed(x, col_pad=8)
    assert int(guard.bits(a)[0]) == 0x7E00 and torch.isnan(a[0])
    v, a = guard.embed(x, col_pad=8, poison=float("inf"))
    assert torch.isinf(a[0]) and torch.equal(v, x)
    v, a = guard.embed(x, col_pad=8, poison=6e4)
    assert a[0].item() == torch.tensor(6e4).half().item()
    v, a = guard.embed(torch.zeros(4, 16, dtype=torch.uint8), col_pad=16)
    assert int(a[0]) == 0x7F and int(v.sum()) == 0
    v, a = guard.embed(torch.zeros(4, 16, dtype=torch.uint8), col_pad=16, poison=guard.E8M0_POISON)
    assert int(a[0]) == 0xFF
    assert torch.isnan(torch.tensor([0x7F], dtype=torch.uint8).view(torch.float8_e4m3fn).float()).all()


def test_view_from_another_arena_is_refused():
    out, arena = guard.sentinel_out((4, 8))
    other, _ = guard.sentinel_out((4, 8))
    with pytest.raises(ValueError):
        guard.assert_untouched(arena, other, "wrong arena")
