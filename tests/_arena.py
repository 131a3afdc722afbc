"""Guarded operands for the containment tests: a tensor carved from the MIDDLE of one larger uint8 buffer, so that what a kernel writes
outside the extents its arguments describe lands in memory the test owns and can be seen, and what it reads there is poison.

    a = guarded((M, Nc), torch.bfloat16, ld=Nc + 4, device="cuda")     # an output: random bytes around and between the rows
    kernel(..., a.view.data_ptr(), ldc=a.ld)
    a.check()                                                          # AssertionError naming the first changed byte as (row, column)

Layout of the buffer:  [ guard | row 0: cols, pad | row 1: cols, pad | ... | row rows-1: cols, pad | guard ].  `view` is the strided
[rows, cols] window (row stride ld elements); everything else -- both guards and the ld - cols pad columns of every row, the last row's
included -- is "outside".  A guard is at least 256 rows x ld elements (one whole row block of the largest GEMM tile, 256 x 256) and
never less than 64 KiB, so a store that is wrong by a whole tile row block still lands inside the buffer.  (A vector -- a bias, a scale
array, a workspace -- has no rows to be wrong by: its guards are its own length, between 64 KiB and 4 MiB.)

Fills of the outside bytes:
    "random" (outputs)   a seeded pseudo-random byte stream: a kernel that writes a constant (0, NaN, its own result) cannot match it;
    an int 0..255        that byte everywhere.  0xFF for inputs of every float type: all-ones bytes are a NaN in fp32, bf16, fp16, e4m3
                         and e8m0 alike, so an over-read that reaches an accumulator shows in the result.  Inputs with no NaN encoding
                         (u8 pixels, MXFP4 code bytes, integer indices) run twice on two different fills (`repoison`) and the outputs
                         must be bit-identical;
    ("elem", v)          every element outside is the value v: for integer INDEX operands, whose two fills must both be valid indices
                         (an over-read index must show as a different result, never as a wild access).
A pristine clone of the buffer is kept; `check` compares the outside bytes with it, bit for bit (torch.equal on uint8).

A plain helper module (not a conftest); works on CPU and CUDA tensors alike (tests/test_arena_host.py runs it on the CPU)."""
import math

import torch

MIN_GUARD_BYTES = 64 * 1024
GUARD_ROWS = 256
MAX_VECTOR_GUARD = 4 * 1024 * 1024
ALIGN = 256
NAN_BYTE = 0xFF


def _numel(shape):
    return int(math.prod(shape))


class Guarded:
    def __init__(self, shape, dtype, ld=None, fill="random", device="cpu", offset=0, seed=0):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s >= 1 for s in shape), shape
        self.shape, self.dtype = shape, dtype
        self.cols = shape[-1]
        self.rows = _numel(shape[:-1])
        self.ld = int(ld) if ld is not None else self.cols
        assert self.ld >= self.cols, (self.ld, self.cols)
        assert len(shape) <= 2 or self.ld == self.cols, "a padded row stride needs a [rows, cols] shape"
        self.esz = torch.empty(0, dtype=dtype).element_size()
        assert offset >= 0 and offset % self.esz == 0, offset
        self.row_bytes = self.ld * self.esz
        self.body_bytes = self.rows * self.row_bytes
        # a vector (one "row": a bias, a scale array, a workspace) has no tile rows to spill by: its own length, at most MAX_VECTOR_GUARD
        spill = GUARD_ROWS * self.row_bytes if len(shape) > 1 else min(self.row_bytes, MAX_VECTOR_GUARD)
        guard = max(spill, MIN_GUARD_BYTES)
        self.guard_bytes = (guard + ALIGN - 1) // ALIGN * ALIGN
        total = self.guard_bytes + ALIGN + offset + self.body_bytes + self.guard_bytes
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        # first byte of the view: 256-byte aligned (the strictest alignment an entry point asks for), plus the explicit misalignment
        self.start = self.guard_bytes + (-(self.buf.data_ptr() + self.guard_bytes)) % ALIGN + offset
        assert (self.buf.data_ptr() + self.start - offset) % ALIGN == 0
        self.seed = seed
        self.view = self._window(self.buf)
        self.pristine = None
        self.repoison(fill, keep=False)

    def _window(self, buf):
        typed = buf[self.start:self.start + self.body_bytes].view(self.dtype)
        if self.ld == self.cols:
            return typed.view(self.shape)
        return typed.as_strided((self.rows, self.cols), (self.ld, 1))

    def _bytes_window(self, buf):
        """the view's bytes as a uint8 [rows, cols * esz] window of `buf`"""
        return buf[self.start:self.start + self.body_bytes].as_strided((self.rows, self.cols * self.esz), (self.row_bytes, 1))

    def repoison(self, fill, keep=True):
        """Refill everything outside the view (guards and pad columns) and take a new pristine clone; the view's content stays
        (keep = False: the view is poisoned with the same fill)."""
        inside = self._bytes_window(self.buf).clone() if keep else None
        if isinstance(fill, str):
            assert fill == "random", fill
            g = torch.Generator().manual_seed(0x5EED + self.seed)
            self.buf.copy_(torch.randint(0, 256, (self.buf.numel(),), dtype=torch.uint8, generator=g))
        elif isinstance(fill, tuple):
            # ("elem", v): every ELEMENT outside is the value v -- for index operands, where an arbitrary byte pattern would decode as an
            # index far outside the table it selects from and an over-read would turn into a wild access instead of a visible difference
            assert len(fill) == 2 and fill[0] == "elem", fill
            self.buf.fill_(0)
            lead = self.start % self.esz
            n = (self.buf.numel() - lead) // self.esz
            self.buf[lead:lead + n * self.esz].view(self.dtype).fill_(fill[1])
        else:
            assert 0 <= int(fill) <= 255, fill
            self.buf.fill_(int(fill))
        if keep:
            self._bytes_window(self.buf).copy_(inside)
        self.fill = fill
        self.pristine = self.buf.clone()
        return self

    def set(self, t):
        """copy `t` (same shape, or [rows, cols]) into the view"""
        self.view.copy_(t.reshape(self.view.shape).to(self.view.device))
        return self

    def first_difference(self):
        """None when every outside byte equals the pristine clone, else (row, column, byte in the element, buffer offset from the view's
        first byte) of the first one that differs.  Rows < 0 / >= rows are the guards, columns >= cols the pad."""
        want = self.pristine.clone()
        self._bytes_window(want).copy_(self._bytes_window(self.buf))
        if torch.equal(want, self.buf):
            return None
        at = int((want != self.buf).nonzero()[0, 0]) - self.start
        row = at // self.row_bytes                              # floor: negative in front of the view
        inrow = at - row * self.row_bytes
        return row, inrow // self.esz, inrow % self.esz, at

    def check(self, what=""):
        d = self.first_difference()
        assert d is None, (f"{what or 'arena'}: a byte outside the [{self.rows}, {self.cols}] view (ld {self.ld}, {self.dtype}) changed: "
                           f"first at row {d[0]}, column {d[1]} (byte {d[2]} of the element; {d[3]:+d} bytes from the view's first byte)")

    def ptr(self):
        return self.view.data_ptr()


def guarded(shape, dtype, ld=None, fill="random", device="cpu", offset=0, seed=0):
    """A [rows, cols] (or [..., cols] when ld is the natural width) tensor with row stride ld >= cols carved from the middle of a larger
    uint8 buffer.  Returns a handle with .view, .check() and .repoison(fill); `offset` shifts the first byte off its 256-byte alignment
    (a multiple of the element size) for the misalignment tests."""
    return Guarded(shape, dtype, ld=ld, fill=fill, device=device, offset=offset, seed=seed)


def hold(t, ld=None, fill=NAN_BYTE, offset=0):
    """An INPUT: `t` copied into a guarded arena on its own device whose outside bytes are `fill` (default all-ones: NaN in every float
    format)."""
    return guarded(tuple(t.shape), t.dtype, ld=ld, fill=fill, device=t.device, offset=offset).set(t)
