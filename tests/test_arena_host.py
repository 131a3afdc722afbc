"""tests/_arena.py on CPU tensors: the proof that the containment harness of tests/test_containment_gpu.py can FAIL.  A byte written one
element in front of the view, one behind it, into a pad column or past the last row is reported, at the right (row, column); a write
inside the view is not; the layout keeps what the kernels need (256-byte aligned first byte, guards of a whole 256-row tile block)."""
import pytest
import torch

from tests import _arena as AR

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32, torch.int64]


def _poke(a, row, col):
    """flip one byte of element (row, col) of the arena's row grid (any row / column, outside the view included) through the raw buffer"""
    at = a.start + row * a.row_bytes + col * a.esz
    assert 0 <= at < a.buf.numel()
    a.buf[at] ^= 0x5A


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["random", 0xFF, 0x00])
def test_layout_alignment_and_guard_size(dtype, fill):
    rows, cols, ld = 5, 13, 16
    a = AR.guarded((rows, cols), dtype, ld=ld, fill=fill)
    assert a.view.shape == (rows, cols) and a.view.stride() == (ld, 1) and a.view.dtype == dtype
    assert a.view.data_ptr() % 256 == 0
    assert a.view.data_ptr() == a.buf.data_ptr() + a.start
    esz = a.view.element_size()
    assert a.guard_bytes >= max(256 * ld * esz, 64 * 1024)
    assert a.start >= a.guard_bytes and a.buf.numel() - (a.start + rows * ld * esz) >= a.guard_bytes
    a.check()
    if fill == "random":                                   # no constant can match the fill: every byte value occurs in a guard
        assert len(torch.unique(a.buf[:a.guard_bytes])) == 256
    else:
        assert bool((a.pristine == fill).all())


def test_all_ones_bytes_are_nan_in_every_float_format():
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        a = AR.guarded((3, 8), dtype, ld=12, fill=AR.NAN_BYTE)
        whole = a.buf[a.start - 64 * a.esz:a.start + 64 * a.esz].view(dtype).float()
        assert bool(torch.isnan(whole).all()), dtype
    # e8m0: 0xFF is the format's NaN by definition (OCP MX), there is nothing to decode on the host


def test_explicit_byte_offset_for_the_misalignment_cases():
    a = AR.guarded((4, 8), torch.bfloat16, ld=8, offset=2)
    assert a.view.data_ptr() % 256 == 2
    a.view.zero_()
    a.check()
    with pytest.raises(AssertionError):
        AR.guarded((4, 8), torch.float32, offset=2)        # not a multiple of the element size


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_write_inside_the_view_is_not_reported(dtype):
    a = AR.guarded((7, 13), dtype, ld=20)
    a.view.fill_(1)
    a.view[6, 12] = 3
    a.view[0, 0] = 2
    assert a.first_difference() is None
    a.check()
    for r, c in ((0, 0), (6, 12), (3, 5)):
        _poke(a, r, c)
    a.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where,row,col", [("one element before the view", -1, 19), ("one element after the view", 6, 13),
                                           ("a pad column", 2, 17), ("a pad column", 0, 13), ("past the last row", 7, 0),
                                           ("past the last row", 7, 5), ("a whole tile row block past the end", 7 + 255, 12),
                                           ("a whole tile row block in front", -256, 0)])
def test_a_write_outside_the_view_is_reported_at_its_offset(dtype, where, row, col):
    a = AR.guarded((7, 13), dtype, ld=20)
    a.view.fill_(1)
    _poke(a, row, col)
    d = a.first_difference()
    assert d is not None, where
    assert d[:2] == (row, col), (where, d)
    assert d[3] == row * a.row_bytes + col * a.esz + d[2]
    with pytest.raises(AssertionError, match=rf"row {row}, column {col} "):
        a.check(where)


def test_the_first_of_several_writes_is_the_one_named():
    a = AR.guarded((7, 13), torch.float32, ld=20)
    _poke(a, 9, 1)
    _poke(a, 3, 15)
    _poke(a, 5, 19)
    assert a.first_difference()[:2] == (3, 15)


def test_a_constant_store_cannot_hide_in_the_random_fill():
    """a kernel that stores one value (0, NaN bits, anything) over a 16-byte run of guard or pad is seen whatever the value is"""
    for value in (0x00, 0xFF, 0x7F, 0x3C):
        a = AR.guarded((4, 8), torch.bfloat16, ld=24)
        at = a.start + 1 * a.row_bytes + 8 * a.esz
        a.buf[at:at + 16] = value
        d = a.first_difference()
        assert d is not None and d[0] == 1 and 8 <= d[1] < 16, (value, d)


def test_repoison_keeps_the_view_and_changes_everything_else():
    t = torch.arange(35, dtype=torch.int32).view(5, 7)
    a = AR.hold(t, ld=12, fill=0x11)
    assert torch.equal(a.view, t) and a.view.stride() == (12, 1)
    assert bool((a.buf[:a.start] == 0x11).all()) and int(a.buf[a.start + 7 * 4]) == 0x11
    a.repoison(0xEE)
    assert torch.equal(a.view, t)
    assert bool((a.buf[:a.start] == 0xEE).all()) and int(a.buf[a.start + 7 * 4]) == 0xEE
    a.check()
    _poke(a, 4, 7)
    assert a.first_difference()[:2] == (4, 7)


def test_element_fill_for_index_operands():
    t = torch.tensor([5, 6, 7], dtype=torch.int32)
    a = AR.hold(t, fill=("elem", 3))
    around = a.buf[a.start - 16:a.start + 12 + 16].view(torch.int32)
    assert around.tolist() == [3, 3, 3, 3, 5, 6, 7, 3, 3, 3, 3]
    a.repoison(("elem", 1))
    assert a.buf[a.start - 16:a.start + 12 + 16].view(torch.int32).tolist() == [1, 1, 1, 1, 5, 6, 7, 1, 1, 1, 1]
    b = AR.hold(torch.tensor([9], dtype=torch.int64), fill=("elem", 2))
    assert b.buf[b.start - 8:b.start + 16].view(torch.int64).tolist() == [2, 9, 2]
    a.check()
    _poke(a, 1, 0)                                         # one element behind the vector: "row 1" of a one-row grid
    assert a.first_difference()[:2] == (1, 0)


def test_a_vector_is_guarded_by_its_own_length():
    a = AR.guarded(10_000_000, torch.uint8)
    assert a.guard_bytes == AR.MAX_VECTOR_GUARD and a.view.shape == (10_000_000,) and a.view.data_ptr() % 256 == 0
    assert AR.guarded(100, torch.float32).guard_bytes == AR.MIN_GUARD_BYTES


def test_shapes_beyond_two_dimensions_are_contiguous_views():
    a = AR.guarded((2, 3, 8), torch.float16, fill=AR.NAN_BYTE)
    assert a.view.shape == (2, 3, 8) and a.view.is_contiguous() and (a.rows, a.cols, a.ld) == (6, 8, 8)
    a.view.zero_()
    a.check()
    _poke(a, 6, 0)
    assert a.first_difference()[:2] == (6, 0)
    b = AR.guarded(9, torch.int64)
    assert b.view.shape == (9,) and (b.rows, b.cols) == (1, 9)
    with pytest.raises(AssertionError):
        AR.guarded((2, 3, 8), torch.float16, ld=16)
