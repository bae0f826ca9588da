"""tests/guard.py can fail: every kind of fault the GPU bounds tests rely on it to see is planted on the CPU and must be reported at its place.
Each test runs the same steps without the plant first, so that removing the plant is seen to flip the outcome."""
import pytest
import torch

from tests.guard import ALIGN, BAND_ROWS, POISON, SENTINEL, guarded, poisoned

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8]


def _flat(g):
    """the typed flat image of the backing buffer, addressed relative to the view's first element"""
    return g.bits if g.view.dtype == g.bits.dtype else g.bits.view(g.view.dtype)


def _plant(g, row, col, value=1):
    _flat(g)[g.off + row * g.ld + col] = value


def _caught(g, **kw):
    with pytest.raises(AssertionError) as e:
        g.check(**kw)
    return str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row,col,where", [(2, 10, "(row 2, column 10)"),        # one element past the end of row 2 (cols = 10, ld = 13)
                                           (5, 0, "(row 5, column 0)"),          # the row behind the view's last
                                           (4, 12, "(row 4, column 12)"),        # the padding of the last row
                                           (-1, 3, "(row -1, column 3)"),        # the front band, next to the view
                                           (-BAND_ROWS, 0, f"(row {-BAND_ROWS}, column 0)"),      # and its far end
                                           (5 + BAND_ROWS - 1, 12, f"(row {5 + BAND_ROWS - 1}, column 12)")])
def test_a_planted_stray_store_is_reported_at_its_row_and_column(dtype, row, col, where):
    view, g = guarded(5, 10, dtype, ld=13)
    view.fill_(3)
    g.check()                                       # no plant: passes
    _plant(g, row, col)
    msg = _caught(g)
    assert "stray write" in msg and where in msg, msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_element_left_unwritten_is_reported(dtype):
    view, g = guarded(5, 10, dtype, ld=13)
    view.fill_(3)
    g.check()
    g.bits[g.off + 3 * g.ld + 7] = SENTINEL[view.element_size()]             # put the sentinel back: element (3, 7) never written
    msg = _caught(g)
    assert "never written" in msg and "(row 3, column 7)" in msg, msg
    g.check(written=False)                          # an accumulate target is not asked for it


def test_a_preset_view_is_an_accumulate_target_and_its_surroundings_still_count():
    view, g = guarded(4, 8, torch.float32, ld=12, fill=0.5)
    assert bool((view == 0.5).all())
    g.check()                                       # nothing written at all: fine for a preset view
    view += 1.0
    g.check()
    _plant(g, 1, 8, 2.0)
    assert "(row 1, column 8)" in _caught(g)


def test_a_valid_mask_narrows_what_the_kernel_owns():
    """packed buffers: only some columns / rows of the view are the kernel's; the rest of the view counts as surroundings"""
    view, g = guarded(6, 16, torch.bfloat16, ld=16)
    valid = torch.zeros(6, 16, dtype=torch.bool)
    valid[:4, :8] = True
    view[:4, :8] = 1.0
    g.check(valid=valid)
    view[4, 0] = 1.0                                # a row the kernel does not own
    assert "(row 4, column 0)" in _caught(g, valid=valid)
    view2, g2 = guarded(6, 16, torch.bfloat16, ld=16)
    view2[:4, :7] = 1.0                             # column 7 of the owned block forgotten
    assert "never written" in _caught(g2, valid=valid)
    # preset by hand (the zero tail of a planes buffer), then re-armed: the preset must survive
    view3, g3 = guarded(6, 16, torch.bfloat16, ld=16)
    view3[4:] = 0
    g3.rearm()
    view3[:4] = 1.0
    rows4 = torch.zeros(6, 16, dtype=torch.bool)
    rows4[:4] = True
    g3.check(valid=rows4)
    view3[5, 15] = 1.0
    assert "(row 5, column 15)" in _caught(g3, valid=rows4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (3, 33, 33), (5, 10, 13), (129, 227, 232), (2, 227, 235)])
def test_alignment_and_band_sizes_are_what_the_helper_promises(dtype, rows, cols, ld):
    view, g = guarded(rows, cols, dtype, ld=ld)
    es = view.element_size()
    assert view.data_ptr() % ALIGN == 0 and tuple(view.shape) == (rows, cols) and view.stride() == (ld, 1)
    assert g.front_rows >= BAND_ROWS and g.back_rows >= BAND_ROWS
    first = (view.data_ptr() - g.bits.data_ptr()) // es
    assert first == g.off and first >= BAND_ROWS * ld
    assert g.bits.numel() - (first + rows * ld) >= BAND_ROWS * ld           # behind a full last row
    assert bool((g.bits == SENTINEL[es]).all())                              # everything, the view included, starts as the sentinel
    if dtype.is_floating_point:
        assert bool(torch.isnan(view).all())                                 # which is a NaN in float32 and in bfloat16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_poisoned_input_equals_its_source_inside_and_is_nan_outside(dtype):
    src = torch.arange(5 * 10, dtype=torch.float32).reshape(5, 10).to(dtype)
    p = poisoned(src, ld=16, extra_rows=3, front_rows=2)
    assert torch.equal(p, src) and p.stride() == (16, 1) and p.data_ptr() % ALIGN == 0
    whole = torch.as_strided(p, (2 + 5 + 3, 16), (16, 1), p.storage_offset() - 2 * 16)
    inside = torch.zeros(10, 16, dtype=torch.bool)
    inside[2:7, :10] = True
    assert bool(torch.isnan(whole[~inside]).all()) and not bool(torch.isnan(whole[inside]).any())
    # the poison is not the guard's sentinel, and does not become it on the way through arithmetic or a rounding to bfloat16
    es = src.element_size()
    assert POISON[es] != SENTINEL[es]
    through = (whole[0, :4].float() + 1.0).to(dtype)
    assert bool((through.view(torch.int16 if es == 2 else torch.int32) != SENTINEL[es]).all())
    assert bool((whole[0, :4].float().bfloat16().view(torch.int16) != SENTINEL[2]).all())
    q = poisoned(src)                               # default: one 16-byte group of padding
    assert q.stride(0) == 10 + ALIGN // src.element_size() and torch.equal(q, src)
    pad = torch.as_strided(q, (5, q.stride(0) - 10), (q.stride(0), 1), q.storage_offset() + 10)
    assert bool(torch.isnan(pad).all())
