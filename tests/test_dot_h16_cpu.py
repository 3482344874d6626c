"""Host side of the 16-bit route of the inner-product producer (include/simspread_hip_half.h), no GPU: the bf16 rounding
helper against torch's, and the argument checks that must not need a device."""
import numpy as np
import pytest
import torch

import simspread_jl_amd as ss


def _torch_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _same(a):
    got, want = ss.to_bf16_bits(a), _torch_bits(a)
    assert got.dtype == np.uint16 and got.shape == np.shape(a)
    nan = np.isnan(np.asarray(a, np.float32))
    assert np.array_equal(got[~nan], want[~nan])
    # a NaN stays a NaN: exponent all ones, mantissa not zero
    assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x007F) != 0).all()
    return got


def test_to_bf16_bits_rounds_like_torch():
    f = np.float32
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, -1 - 3 * 2.0 ** -8,     # exact ties: down, up
                     1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23], f)               # just above, just below
    got = _same(ties)
    assert list(got[:4]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82] and list(got[4:]) == [0x3F81, 0x3F80]
    assert list(_same(np.array([0.0, -0.0], f))) == [0x0000, 0x8000]
    sub = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.17549421e-38, 9.1835e-41, 4.6e-41], f)   # fp32 / bf16 subnormals
    _same(sub)
    big = np.array([np.finfo(f).max, -np.finfo(f).max, 3.3895314e38, 3.3961775e38, 3.4e38], f)
    got = _same(big)
    assert got[0] == 0x7F80 and got[1] == 0xFF80 and got[2] == 0x7F7F         # largest fp32 -> inf, largest bf16 stays
    got = _same(np.array([np.inf, -np.inf, np.nan, -np.nan], f))
    assert got[0] == 0x7F80 and got[1] == 0xFF80
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)               # every exponent, NaNs too
    _same(bits.view(f))
    _same((rng.standard_normal((100, 37)) * 3).astype(f))
    # fp64 input is rounded once: 1 + 2^-8 + 2^-30 lies above the tie, although fp32 would round it onto the tie
    assert list(ss.to_bf16_bits(np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8 - 2.0 ** -30, 1e300, -1e300]))) == \
        [0x3F81, 0x3F80, 0x7F80, 0xFF80]
    assert ss.to_bf16_bits(np.arange(-3, 4)).tolist() == _torch_bits(np.arange(-3, 4)).tolist()
    with pytest.raises(TypeError):
        ss.to_bf16_bits(np.array(["a"]))


def test_argument_validation_needs_no_device():
    X = np.zeros((4, 3))
    Y = np.eye(4, 2)
    with pytest.raises(ValueError, match="storage"):
        ss.dot_csr(X, alpha=0.5, storage="fp8")
    with pytest.raises(ValueError, match="storage"):
        ss.DeviceGraph.from_vectors(None, X, Y, alpha=0.5, storage="half")
    with pytest.raises(TypeError, match="float32"):
        ss.dot_csr(X, alpha=0.5, storage="bf16", dtype=np.float64)
    with pytest.raises(TypeError, match="float32"):
        ss.DeviceGraph.from_vectors(None, X, Y, alpha=0.5, storage="f16", dtype=np.float64)
    with pytest.raises(NotImplementedError, match="min_neighbours"):
        ss.dot_csr(X, alpha=0.5, storage="f16", min_neighbours=1)
    with pytest.raises(NotImplementedError, match="min_neighbours"):
        ss.DeviceGraph.from_vectors(None, X.astype(np.float16), Y, alpha=0.5, min_neighbours=1, storage="f16")
    # mixed host / device inputs (a torch tensor stands for the device side; nothing touches a device)
    T = torch.zeros(2, 3, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="host"):
        ss.dot_csr(X, T, alpha=0.5, storage="bf16")
    with pytest.raises(TypeError, match="host"):
        ss.dot_csr(T, X, alpha=0.5)
    with pytest.raises(TypeError, match="host"):
        ss.DeviceGraph.from_vectors(T, X, Y, alpha=0.5, storage="bf16")
    with pytest.raises(ValueError, match="metric"):
        ss.dot_csr(X, alpha=0.5, storage="bf16", metric="l2")
    with pytest.raises(NotImplementedError, match="16-bit"):
        ss.butina_clusters(vectors=T, cutoff=0.5)


def test_implicit_selection_changes_no_call_that_worked_before():
    """numpy float16 rows were always accepted and widened exactly.  Without `storage` they take the 16-bit route only
    where the result is the same graph: all inputs float16, a float32 graph, no neighbour floor."""
    from simspread_jl_amd.engine import _h16_storage
    H, D = np.zeros((4, 3), np.float16), np.zeros((2, 3))
    assert _h16_storage(None, (H, None), np.float32) == 1
    assert _h16_storage(None, (H, H), np.float32) == 1
    assert _h16_storage(None, (H, D), np.float32) is None          # the fp64 side must not be rounded silently
    assert _h16_storage(None, (D, H), np.float32) is None
    assert _h16_storage(None, (H, None), np.float32, min_neighbours=3) is None     # the floor keeps the fp32 route
    assert _h16_storage(None, (H, None), np.float64) is None
    assert _h16_storage(None, (D, None), np.float32) is None
    assert _h16_storage("bf16", (H, D), np.float32) == 0           # named: both sides are rounded to it
    T = torch.zeros(2, 3, dtype=torch.bfloat16)
    assert _h16_storage(None, (T, None), np.float32) == 0
    assert _h16_storage(None, (torch.zeros(2, 3), T), np.float32) == 0            # refused later: one dtype per call
    assert _h16_storage(None, (T, None), np.float32, auto_tensor=False) is None
    with pytest.raises(NotImplementedError):
        _h16_storage(None, (T, None), np.float32, min_neighbours=1)
