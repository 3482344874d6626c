"""The raw W*R SpMM at the shape bench.py's spmm_sweep measures (W 100k x 100k, 1 %, nnz ~1e8), every row of every
width against scipy in fp64.  Default routing (no chunk overrides): the compact sliced-ELL builder cuts dozens of
K-chunks with 16-bit local indices near their limit, the partial-sum pass and the slice tails run at full size, and
every width lands on the route api.hip's table gives it, which each case asserts."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

M = K = 100_000
BMAX = 65
TOL = {np.float32: 1e-5, np.float64: 1e-13}   # element-wise, relative to (|W| @ |R|) of the same entry

NARROW, CSELL, SELL = "spmm_chunked_narrow", "spmm_csell", "spmm_sell"


def expected_route(dtype, B, binary, colmajor=False):
    """ss_spmm's routing (api.hip, 'Routing by width'): row-major B <= 4 -> narrow kernel, except fp64 B = 2 and
    B = 3, 4 which take the lane-per-row kernel on the compact sliced-ELL operand; 5 <= B with B * sizeof <= 256 bytes
    -> that same kernel, unless W is pattern-only and B * sizeof > 128 bytes; everything wider, and column-major
    operands, -> the SELL kernel."""
    vb = np.dtype(dtype).itemsize
    if colmajor:
        return SELL
    if B <= 4:
        return CSELL if (B >= 3 or (B == 2 and vb == 8)) else NARROW
    if B * vb <= 256 and not (binary and B * vb > 128):
        return CSELL
    return SELL


def _rows_product(W, R, threads=16):
    """W @ R in fp64 over row blocks in threads (scipy releases the GIL in its sparse-dense product)."""
    step = (W.shape[0] + threads - 1) // threads
    with ThreadPoolExecutor(threads) as ex:
        return np.vstack(list(ex.map(lambda a: W[a:a + step] @ R, range(0, W.shape[0], step))))


@pytest.fixture(scope="module")
def sweep():
    """W as bench.py's spmm_sweep draws it (seed, sorted unique keys, values U[0.5, 1.5) in fp32), built once on the
    device; R standard normal, rounded to fp32 so one fp64 reference serves both precisions."""
    import torch
    ss.init(0)
    ss.use_torch_stream()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(20250222 + 3)
    n_draw = int(M * K * 0.01)
    rows = torch.randint(0, M, (n_draw,), device=dev, generator=g, dtype=torch.int64)
    cols = torch.randint(0, K, (n_draw,), device=dev, generator=g, dtype=torch.int64)
    keys = torch.unique(rows * K + cols)
    del rows, cols
    r = torch.div(keys, K, rounding_mode="floor")
    idx = (keys - r * K).to(torch.int32)
    ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(r, minlength=M), 0)
    del keys, r
    val = torch.rand(idx.numel(), device=dev, dtype=torch.float32, generator=g) + 0.5
    ones = torch.ones_like(val)
    assert idx.numel() > 9.9e7
    hp, hi, hv = ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    Wv = sp.csr_matrix((hv, hi, hp), shape=(M, K))
    Wp = sp.csr_matrix((np.ones_like(hv), hi, hp), shape=(M, K))
    assert Wv.has_sorted_indices and (np.diff(hp) > 0).all()
    rng = np.random.default_rng(20250222)
    R = rng.standard_normal((K, BMAX)).astype(np.float32).astype(np.float64)
    ref = {False: (_rows_product(Wv, R), _rows_product(Wv, np.abs(R))),
           True: (_rows_product(Wp, R), _rows_product(Wp, np.abs(R)))}
    del Wv, Wp
    mats = {}
    for dt in (np.float32, np.float64):
        tv = val if dt == np.float32 else val.double()
        to = ones if dt == np.float32 else ones.double()
        mats[(dt, False)] = ss.DeviceSpMat.from_device_csr(M, K, ptr, idx, tv, dtype=dt)
        mats[(dt, True)] = ss.DeviceSpMat.from_device_csr(M, K, ptr, idx, to, dtype=dt)
    Rd = {dt: torch.from_numpy(R.astype(dt)).to(dev) for dt in (np.float32, np.float64)}
    yield mats, Rd, ref
    for m in mats.values():
        m.close()


def _check(got, want, scale, dtype, label):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, label
    err = np.abs(got - want)
    assert np.isfinite(got).all(), label
    bound = TOL[dtype] * scale
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{label}: {len(bad)} entries out of bound, first {bad[0].tolist()} "
                           f"(want {want[tuple(bad[0])]!r}, got {got[tuple(bad[0])]!r}, |W||R| {scale[tuple(bad[0])]!r})")
    worst = float((err / scale).max())
    print(f"[spmm_at_size] {label}: route {','.join(ss.path_last())}, all {got.shape[0]} rows, "
          f"worst |err| / (|W||R|) {worst:.3e}")
    return worst


CASES = ([(np.float32, B, False) for B in (1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65)]
         + [(np.float32, B, True) for B in (1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65)]
         + [(np.float64, B, False) for B in (1, 2, 4, 8, 16, 32, 33)]
         + [(np.float64, 32, True)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B,binary", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_spmm_100k_every_row(sweep, dtype, B, binary):
    import torch
    mats, Rd, ref = sweep
    w = mats[(dtype, binary)]
    R = Rd[dtype][:, :B].contiguous()
    F = w.spmm(R)
    torch.cuda.synchronize()
    route = expected_route(dtype, B, binary)
    path = ss.path_last()
    assert route in path or (route == SELL and "spmm_sell_sorted" in path), (route, path)
    want, scale = ref[binary][0][:, :B], ref[binary][1][:, :B]
    _check(F.cpu().numpy(), want, scale, dtype, f"{np.dtype(dtype).name} B={B} {'pattern' if binary else 'values'}")


@pytest.mark.gpu
def test_spmm_100k_column_major(sweep):
    import torch
    mats, Rd, ref = sweep
    B = 16
    w = mats[(np.float32, False)]
    F = w.spmm(Rd[np.float32][:, :B].T.contiguous(), colmajor=True)
    torch.cuda.synchronize()
    path = ss.path_last()
    assert SELL in path or "spmm_sell_sorted" in path, path
    _check(F.cpu().numpy().T, ref[False][0][:, :B], ref[False][1][:, :B], np.float32, "float32 B=16 column-major")


def test_expected_route_table():
    """The route table this file asserts, written out (it must agree with api.hip's comment and code)."""
    assert [expected_route(np.float32, B, False) for B in (1, 2, 3, 4, 5, 64, 65)] == \
        [NARROW, NARROW, CSELL, CSELL, CSELL, CSELL, SELL]
    assert [expected_route(np.float32, B, True) for B in (2, 32, 33, 64)] == [NARROW, CSELL, SELL, SELL]
    assert [expected_route(np.float64, B, False) for B in (1, 2, 4, 8, 32, 33)] == [NARROW, CSELL, CSELL, CSELL, CSELL, SELL]
    assert expected_route(np.float64, 32, True) == SELL and expected_route(np.float32, 16, False, colmajor=True) == SELL
