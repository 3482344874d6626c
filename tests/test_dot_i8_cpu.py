"""Host side of the int8 route of the inner-product producer (include/simspread_hip_int8.h), no GPU: quantize_i8, the
exact conversion of the accepted inputs, and the argument checks that must not need a device."""
import numpy as np
import pytest
import torch

import simspread_jl_amd as ss
from simspread_jl_amd import engine


def test_quantize_i8_properties():
    rng = np.random.default_rng(8)
    X = rng.standard_normal((50, 37)) * 3
    Q, scale = ss.quantize_i8(X)
    top = np.abs(X).max()
    assert Q.dtype == np.int8 and Q.shape == X.shape and scale == top / 127
    assert np.abs(Q).max() == 127 and Q.min() >= -127                     # symmetric: -128 is never produced
    assert np.array_equal(Q, np.rint(X * (127.0 / top)).astype(np.int8))
    assert np.abs(Q * scale - X).max() <= scale / 2 * (1 + 1e-12)          # round to nearest
    # ties go to even: 0.5, 1.5, 2.5, -0.5, -1.5 steps of the grid
    T = np.array([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5])
    q, s = ss.quantize_i8(T)
    assert s == 1.0 and q.tolist() == [127, 0, 2, 2, 0, -2, -2, 64]
    # an all-zero tensor (and an empty one): zeros, scale 1
    q, s = ss.quantize_i8(np.zeros((3, 4)))
    assert s == 1.0 and q.dtype == np.int8 and not q.any() and q.shape == (3, 4)
    q, s = ss.quantize_i8(np.zeros((0, 4)))
    assert s == 1.0 and q.shape == (0, 4)
    # a common scale of the input changes nothing: that is why the three metrics may use Q in place of X
    assert np.array_equal(ss.quantize_i8(X * 4)[0], Q) and np.array_equal(ss.quantize_i8(-X)[0], -Q)
    assert np.array_equal(ss.quantize_i8(X.astype(np.float32))[0], ss.quantize_i8(X.astype(np.float32).astype(np.float64))[0])
    assert ss.quantize_i8(np.arange(-5, 6))[0].tolist() == np.rint(np.arange(-5, 6) * 25.4).astype(int).tolist()
    for bad in (np.array([1.0, np.nan]), np.array([np.inf, 1.0])):
        with pytest.raises(ValueError):
            ss.quantize_i8(bad)
    with pytest.raises(TypeError):
        ss.quantize_i8(np.array(["a"]))
    assert "invariant" in ss.quantize_i8.__doc__


def test_host_inputs_are_taken_as_they_are_or_converted_exactly():
    keep = []
    A = np.arange(-128, 128, dtype=np.int8).reshape(16, 16)
    ptr, n, d, ld = engine._features_i8(A, False, keep)
    assert (ptr, n, d, ld) == (A.ctypes.data, 16, 16, 16)                  # numpy int8: no copy
    for other in (A.astype(np.int64), A.astype(np.float32), A.astype(np.float64), A.astype(np.int16)):
        keep = []
        ptr, n, d, ld = engine._features_i8(other, False, keep)
        assert keep[0].dtype == np.int8 and np.array_equal(keep[0], A) and ptr == keep[0].ctypes.data
    keep = []
    engine._features_i8((A.astype(np.int64) & 127).astype(np.uint8), False, keep)
    assert np.array_equal(keep[0], A & 127)
    F = np.asfortranarray(A)                                               # rows are made contiguous
    keep = []
    engine._features_i8(F, False, keep)
    assert keep[0].flags.c_contiguous and np.array_equal(keep[0], A)
    assert engine._features_i8(np.zeros((5, 0), np.int8), False, [])[1:] == (5, 0, 1)
    assert engine._features_i8(None, False, []) == (None, 0, 0, 1)
    # no silent rounding, no wrap-around
    for bad in (np.array([[0.5]]), np.array([[128]]), np.array([[-129]]), np.array([[np.nan]]), np.array([[np.inf]]),
                np.array([[200]], np.uint8), np.array([[1e10]]), np.array([[True]]), np.array([["1"]]),
                np.array([[1 + 0j]]), np.array([[2 ** 40]], np.uint64)):
        with pytest.raises(ValueError):
            engine._features_i8(bad, False, [])
    with pytest.raises(ValueError):
        engine._features_i8(np.zeros(4, np.int8), False, [])               # not a matrix


def test_argument_validation_needs_no_device():
    X = np.zeros((4, 3), np.int8)
    Y = np.eye(4, 2)
    with pytest.raises(ValueError, match="storage"):
        ss.dot_csr(X, alpha=0.5, storage="i4")
    with pytest.raises(TypeError, match="float32"):
        ss.dot_csr(X, alpha=0.5, storage="i8", dtype=np.float64)
    with pytest.raises(TypeError, match="float32"):
        ss.DeviceGraph.from_vectors(None, X, Y, alpha=0.5, storage="i8", dtype=np.float64)
    with pytest.raises(TypeError, match="alpha"):
        ss.dot_csr(X, storage="i8")
    with pytest.raises(TypeError, match="k"):
        ss.dot_kth_i8(X)
    for k in (65, -1, 2.5):
        with pytest.raises(ValueError, match="outside"):
            ss.dot_csr(X, alpha=0.5, storage="i8", min_neighbours=k)
        with pytest.raises(ValueError, match="outside"):
            ss.DeviceGraph.from_vectors(None, X, Y, alpha=0.5, storage="i8", min_neighbours=k)
    for k in (0, 65):
        with pytest.raises(ValueError, match="outside"):
            ss.dot_kth_i8(X, k=k)
    with pytest.raises(ValueError, match="metric"):
        ss.dot_csr(X, alpha=0.5, storage="i8", metric="l2")
    with pytest.raises(ValueError, match="integers"):
        ss.dot_csr(X + 0.5, alpha=0.5, storage="i8")
    with pytest.raises(ValueError, match="integers"):
        ss.dot_kth_i8(X.astype(np.int32) + 300, k=2)
    with pytest.raises(ValueError, match="metric"):
        ss.dot_kth_i8(X, k=2, metric="l2")
    with pytest.raises(ValueError, match="integers"):
        ss.DeviceGraph.from_vectors(X + 0.25, X, Y, alpha=0.5, storage="i8")
    with pytest.raises(ValueError, match="features"):
        ss.dot_csr(X, np.zeros((2, 5), np.int8), alpha=0.5, storage="i8")
    # mixed host / device inputs (a torch tensor stands for the device side; nothing touches a device)
    T = torch.zeros(2, 3, dtype=torch.int8)
    with pytest.raises(TypeError, match="host"):
        ss.dot_csr(X, T, alpha=0.5, storage="i8")
    with pytest.raises(TypeError, match="host"):
        ss.DeviceGraph.from_vectors(T, X, Y, alpha=0.5, storage="i8")


def test_the_route_is_taken_only_when_named():
    """int8 arrays without `storage` go where they always went (widened exactly to the graph precision); the selection of
    the 16-bit route does not know them."""
    from simspread_jl_amd.engine import _h16_storage, _i8_storage
    B = np.zeros((4, 3), np.int8)
    assert _h16_storage(None, (B, None), np.float32) is None
    assert _h16_storage(None, (torch.zeros(2, 3, dtype=torch.int8), None), np.float32) is None
    assert _i8_storage(None, (B, None), np.float32) is False
    assert _i8_storage("bf16", (B, None), np.float32) is False
    assert _i8_storage("i8", (B, None), np.float32, 64) is True
    assert _i8_storage("i8", (B, B), np.float32, 1, k_min=1) is True
    with pytest.raises(ValueError, match="storage"):                       # still no storage of that name there
        ss.dot_profile(B, cuts=[0.5], storage="i8")
