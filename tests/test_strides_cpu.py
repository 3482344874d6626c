"""The checker of the stride tests can fail (no device): the reference block is written into host canvases by a correct
writer and by three deliberately defective ones (tests/stride_ref.py); `check` accepts the first and rejects each of the
others, at every padding and base offset the GPU tests use -- and with a tight leading dimension two of the three pass,
which is why the GPU suite needed padded canvases to see them."""
import numpy as np
import pytest

import stride_ref as R

DTYPES = [np.float32, np.float64]
PADS = (1, 3, 4)
FRONTS = (0, 1)
BACK = 8


def _block(rows, cols, dtype, seed=0):
    rng = np.random.default_rng(seed)
    b = (rng.integers(-64, 65, size=(rows, cols)) / 16.0).astype(dtype)
    b[0, 0] = dtype(-0.0)            # the comparison is on bits: -0.0 is not +0.0
    return b


def _written(cv, block, defect):
    flat = cv.host()
    R.write_block(flat, cv, block, defect)
    return flat


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_sentinel_is_a_quiet_nan_with_its_payload(dtype):
    cv = R.canvas(3, 5, 9, 1, 2, dtype, R.HOST)
    assert cv.buf.shape == (1 + 3 * 9 + 2,) and cv.buf.dtype == np.dtype(dtype)
    assert np.isnan(cv.buf).all()
    bits = cv.buf.view(R.BITS[np.dtype(dtype)])
    assert (bits == (0x7FC0BEEF if dtype == np.float32 else 0x7FF80000DEADBEEF)).all()
    assert cv.ptr == cv.buf.ctypes.data + np.dtype(dtype).itemsize and not cv.aligned
    assert R.canvas(3, 5, 9, 0, 2, dtype, R.HOST).aligned
    R.check(cv, cv.host(), cv.window(cv.host()).copy())       # an untouched canvas: the window holds the sentinel too


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("cols", [3, 5, 6, 7, 64, 65])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_check_accepts_the_correct_writer_and_rejects_each_defect(dtype, cols, pad, front):
    rows = 6
    block = _block(rows, cols, dtype)
    cv = R.canvas(rows, cols, cols + pad, front, BACK, dtype, R.HOST)
    R.check(cv, _written(cv, block, None), block, "correct writer")
    for defect in R.DEFECTS:
        if defect == R.DEFECTS[1] and cols % 4 == 0:
            continue                                        # a four-wide store of a multiple of four overruns nothing
        cv = R.canvas(rows, cols, cols + pad, front, BACK, dtype, R.HOST)
        with pytest.raises(AssertionError):
            R.check(cv, _written(cv, block, defect), block, defect)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_overrun_is_one_to_three_elements(dtype):
    """cols = 5, 6, 7: the four-wide store writes 3, 2, 1 elements of padding per row, and nothing else is wrong."""
    for cols, over in ((5, 3), (6, 2), (7, 1)):
        block = _block(4, cols, dtype)
        cv = R.canvas(4, cols, cols + 4, 0, BACK, dtype, R.HOST)
        flat = _written(cv, block, R.DEFECTS[1])
        body = flat[:4 * cv.ld].reshape(4, cv.ld).view(R.BITS[np.dtype(dtype)])
        assert ((body != cv.fill).sum(axis=1) == cols + over).all()
        assert np.array_equal(np.ascontiguousarray(cv.window(flat)).view(np.uint8), block.view(np.uint8))
        with pytest.raises(AssertionError, match="outside"):
            R.check(cv, flat, block)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_tight_leading_dimension_hides_the_first_two_defects(dtype):
    """ld == cols: the wrong stride is the right one, and an overrun lands on the next row, which is rewritten later (the
    last row's lands behind the block, where only a canvas with `back` looks)."""
    block = _block(6, 7, dtype)
    for defect in R.DEFECTS[:2]:
        cv = R.canvas(6, 7, 7, 0, BACK, dtype, R.HOST)
        flat = _written(cv, block, defect)
        assert np.array_equal(np.ascontiguousarray(cv.window(flat)).view(np.uint8), block.view(np.uint8))
    cv = R.canvas(6, 7, 7, 0, BACK, dtype, R.HOST)
    R.check(cv, _written(cv, block, R.DEFECTS[0]), block)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_padding_of_another_fill_and_wrong_values(dtype):
    """Consumer canvases hold +inf or a finite value instead of the sentinel; a single wrong bit in the window, or a
    padding element set to the sentinel there, is rejected."""
    block = _block(5, 9, dtype)
    for fill in (np.inf, 1000.0):
        cv = R.canvas(5, 9, 12, 1, 3, dtype, R.HOST, fill=fill)
        assert (cv.buf == dtype(fill)).all()
        cv.put(block)
        R.check(cv, cv.host(), block)
        flat = cv.host().copy()
        flat[cv.front + 9] = np.nan
        with pytest.raises(AssertionError, match="outside"):
            R.check(cv, flat, block)
    cv = R.canvas(5, 9, 12, 1, 3, dtype, R.HOST)
    cv.put(block)
    wrong = block.copy()
    wrong[4, 8] = np.nextafter(wrong[4, 8], dtype(100))
    with pytest.raises(AssertionError, match="differ"):
        R.check(cv, cv.host(), wrong)
    plus_zero = block.copy()
    plus_zero[0, 0] = dtype(0.0)
    with pytest.raises(AssertionError, match="differ"):
        R.check(cv, cv.host(), plus_zero)
    for where in (0, cv.size - 1):                       # the elements before the base and behind the block count too
        flat = cv.host().copy()
        flat[where] = 0.0
        with pytest.raises(AssertionError, match="outside"):
            R.check(cv, flat, block)
