"""Canvases for the tests of the stride contract (tests/test_gpu_strides.py, tests/test_strides_cpu.py): every score entry
point of the C ABI takes a leading dimension and an arbitrary base pointer, and must write the rows x cols window it is
asked for and nothing else.

A canvas is a flat buffer of front + rows * ld + back elements in host memory (numpy) or device memory (a torch CUDA
tensor), every element a quiet NaN with a recognisable payload.  The block handed to the library starts at element
`front` (front = 1 moves the base off 16-byte alignment: allocations are at least 64-byte aligned) and has leading
dimension ld; for a column-major block the caller swaps the roles of rows and columns (rows = the block's columns,
cols = its rows, ld >= cols).  `check` compares integer views of the bits, because NaN != NaN: the window must be the
expected block bit for bit and every other element must still hold the sentinel.  What that catches, and that it
catches it, is shown without a device in tests/test_strides_cpu.py:
  * an index computed with cols where ld belongs       (rows land in the wrong place, padding is written)
  * a vector store that runs past the last column      (padding is written)
  * a first chunk that adds into the destination       (NaN + x is NaN: the window is not the expected block)
  * a read of an operand's padding                     (the sentinel is a NaN: it poisons every sum it enters)

Nothing here needs a device; torch is imported only for device canvases."""
import numpy as np

HOST, DEVICE = 0, 1
SENTINEL = {np.dtype(np.float32): 0x7FC0BEEF, np.dtype(np.float64): 0x7FF80000DEADBEEF}
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits_of(value, dtype):
    """The bit pattern of `value` in dtype, as a Python integer."""
    dt = np.dtype(dtype)
    return int(np.array([value], dtype=dt).view(BITS[dt])[0])


class Canvas:
    """buf: the flat buffer (numpy array or torch CUDA tensor), ptr: the address of element `front`, fill: the bits every
    element outside the window holds."""

    def __init__(self, buf, ptr, rows, cols, ld, front, back, dtype, mem, fill):
        self.buf, self.ptr = buf, ptr
        self.rows, self.cols, self.ld, self.front, self.back = rows, cols, ld, front, back
        self.dtype, self.mem, self.fill = np.dtype(dtype), mem, fill
        self.size = front + rows * ld + back

    @property
    def aligned(self):
        return self.ptr % 16 == 0

    def host(self):
        """The whole buffer as a numpy array (a copy for a device canvas; the caller has drained the library's stream)."""
        if self.mem == HOST:
            return self.buf
        return self.buf.cpu().numpy()

    def window(self, flat):
        """The rows x cols window of a flat host copy of the buffer (a view)."""
        body = flat[self.front:self.front + self.rows * self.ld].reshape(self.rows, self.ld)
        return body[:, :self.cols]

    def put(self, block):
        """Write an input block into the window (before the library call); the padding keeps its fill."""
        block = np.ascontiguousarray(block, dtype=self.dtype)
        assert block.shape == (self.rows, self.cols), (block.shape, self.rows, self.cols)
        if self.mem == HOST:
            self.window(self.buf)[...] = block
            return self
        import torch
        flat = self.buf.cpu().numpy()
        self.window(flat)[...] = block
        self.buf.copy_(torch.from_numpy(flat))
        return self


def canvas(rows, cols, ld, front, back, dtype, mem, fill=None):
    """A Canvas of front + rows * ld + back elements of `dtype` in `mem`, every element the NaN sentinel (or, for the
    score blocks handed to consumers, the value `fill`: +inf or a finite number above every score)."""
    dt = np.dtype(dtype)
    assert ld >= cols and front >= 0 and back >= 0 and rows >= 0
    bits = SENTINEL[dt] if fill is None else bits_of(fill, dt)
    n = front + rows * ld + back
    if mem == HOST:
        buf = np.full(n, bits, dtype=BITS[dt]).view(dt)
        assert buf.ctypes.data % 16 == 0
        return Canvas(buf, buf.ctypes.data + front * dt.itemsize, rows, cols, ld, front, back, dt, mem, bits)
    import torch
    it, ft = (torch.int32, torch.float32) if dt == np.float32 else (torch.int64, torch.float64)
    width = 8 * dt.itemsize
    signed = bits - (1 << width) if bits >> (width - 1) else bits
    buf = torch.full((max(n, 1),), signed, dtype=it, device="cuda").view(ft)[:n]
    assert buf.data_ptr() % 16 == 0
    return Canvas(buf, buf.data_ptr() + front * dt.itemsize, rows, cols, ld, front, back, dt, mem, bits)


def check(cv, got, want, label=""):
    """got: a flat host copy of the canvas after the call (cv.host()).  The window equals `want` (rows x cols) bit for
    bit, and every other element of the buffer still holds the canvas's fill."""
    dt = cv.dtype
    got = np.asarray(got)
    assert got.dtype == dt and got.shape == (cv.size,), (got.dtype, got.shape, cv.size)
    want = np.ascontiguousarray(want)
    assert want.dtype == dt and want.shape == (cv.rows, cv.cols), (want.dtype, want.shape, cv.rows, cv.cols)
    gb = got.view(BITS[dt])
    outside = np.ones(cv.size, dtype=bool)
    cv.window(outside)[...] = False
    touched = outside & (gb != BITS[dt](cv.fill))
    if touched.any():
        at = np.flatnonzero(touched) - cv.front
        where = [(int(i // cv.ld), int(i % cv.ld)) if 0 <= i < cv.rows * cv.ld else int(i) for i in at[:8]]
        raise AssertionError(f"{label}: {int(touched.sum())} elements outside the {cv.rows} x {cv.cols} window (ld "
                             f"{cv.ld}, front {cv.front}) were written; first at (row, column) / offset {where}")
    wb = np.ascontiguousarray(cv.window(gb))
    bad = wb != want.view(BITS[dt])
    if bad.any():
        idx = np.argwhere(bad)
        nan = int(np.isnan(np.ascontiguousarray(cv.window(got))[bad]).sum())
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements of the window differ from the expected "
                             f"bits ({nan} of them NaN); first at {idx[:8].tolist()} (ld {cv.ld}, front {cv.front})")


# ----------------------------------------------------------------------------- writers (models of a kernel's stores)
DEFECTS = ("row stride cols instead of ld", "four-wide store past the last column", "adds into the destination")


def write_block(flat, cv, block, defect=None):
    """Store `block` (rows x cols) into the flat host buffer of canvas cv the way a kernel would, row by row in order;
    defect: None or one of DEFECTS.  The four-wide store writes whole groups of four elements, the columns past the
    block as zeros (what a vector store of a zero-padded accumulator leaves)."""
    rows, cols = block.shape
    for r in range(rows):
        stride = cols if defect == DEFECTS[0] else cv.ld
        o = cv.front + r * stride
        if defect == DEFECTS[1]:
            w = -(-cols // 4) * 4
            row = np.zeros(w, dtype=block.dtype)
            row[:cols] = block[r]
            flat[o:o + w] = row
        elif defect == DEFECTS[2]:
            flat[o:o + cols] += block[r]
        else:
            flat[o:o + cols] = block[r]
