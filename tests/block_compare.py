"""One comparison of a score block from the device with its fp64 oracle, shared by the at-size GPU tests.

Every term of a SimSpread score is >= 0, so a score block is checked element by element, not only against its
largest entry:
  * -99 (clean!, src/core.jl:478-484) sits at exactly the same positions in both blocks;
  * want > 0 <=> got > 0 and want == 0 => got == 0 (a dropped or an invented contribution shows);
  * |got - want| <= tol_e * want on every positive entry;
  * max |got - want| <= tol_block * (largest positive want), the block-relative bound the suite used before.
Returns the two observed error measures so a test can report its margin."""
import numpy as np

# element-wise / block-relative bounds by result precision
TOL = {np.dtype(np.float32): (1e-4, 1e-5), np.dtype(np.float64): (1e-11, 1e-12)}


def compare_block(got, want, dtype, label="", tol_e=None, tol_block=None):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    te, tb = TOL[np.dtype(dtype)]
    te = te if tol_e is None else tol_e
    tb = tb if tol_block is None else tol_block
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.isfinite(want).all(), label
    w99, g99 = want == -99.0, got == -99.0
    bad = np.argwhere(w99 != g99)
    assert bad.size == 0, f"{label}: -99 differs at {len(bad)} positions, first {bad[0].tolist()}"
    pos, gpos = want > 0, got > 0
    bad = np.argwhere(pos != gpos)
    assert bad.size == 0, (f"{label}: sign pattern differs at {len(bad)} positions, first {bad[0].tolist()} "
                           f"(want {want[tuple(bad[0])]!r}, got {got[tuple(bad[0])]!r})")
    zero = want == 0
    bad = np.argwhere(zero & (got != 0))
    assert bad.size == 0, f"{label}: {len(bad)} structural zeros became non-zero, first {bad[0].tolist()}"
    elem = float((np.abs(got[pos] - want[pos]) / want[pos]).max()) if pos.any() else 0.0
    scale = float(want[pos].max()) if pos.any() else 1.0
    keep = ~w99
    block = float(np.abs(got[keep] - want[keep]).max() / scale) if keep.any() else 0.0
    if not elem <= te:
        rel = np.where(pos, np.abs(got - want) / np.where(pos, want, 1.0), 0.0)
        at = np.unravel_index(int(np.argmax(rel)), rel.shape)
        raise AssertionError(f"{label}: element-wise error {elem:.3e} > {te:.0e} at {list(at)} "
                             f"(want {want[at]!r}, got {got[at]!r})")
    assert block <= tb, f"{label}: error {block:.3e} relative to the largest score > {tb:.0e}"
    print(f"[compare_block] {label}: {want.shape[0]} rows x {want.shape[1]}, element-wise {elem:.3e}, "
          f"block-relative {block:.3e}, -99 entries {int(w99.sum())}")
    return {"elem": elem, "block": block}
