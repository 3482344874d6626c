"""CPU-side checks of the fingerprint route (no GPU): the packed layout of pack_fingerprints is Julia's BitVector.chunks
layout, and the four Tanimoto entry points exist, are bound, and refuse to run without ss_init (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

import simspread_jl_amd as ss
from simspread_jl_amd import _lib


def _chunks(bits):
    """BitVector(bits).chunks written out by hand: bit k is bit k % 64 of word k ÷ 64, unused high bits zero."""
    d = len(bits)
    words = [0] * max((d + 63) // 64, 1)
    for k, b in enumerate(bits):
        if b:
            words[k // 64] |= 1 << (k % 64)
    return words


@pytest.mark.parametrize("d", [1, 63, 64, 65, 130, 2048])
def test_pack_fingerprints_is_the_bitvector_chunks_layout(d):
    rng = np.random.default_rng(d)
    bits = rng.random((5, d)) < 0.4
    bits[0] = True                       # a full row: trailing bits past d must still be zero
    bits[1] = False
    F = ss.pack_fingerprints(bits)
    assert F.dtype == np.uint64 and F.shape == (5, (d + 63) // 64) and F.flags.c_contiguous
    for i in range(5):
        assert [int(w) for w in F[i]] == _chunks(list(bits[i])), i
    # bits past d are zero, and the popcount is the number of set bits
    if d % 64:
        assert int(F[0, -1]) >> (d % 64) == 0
    assert [sum(bin(int(w)).count("1") for w in row) for row in F] == list(bits.sum(axis=1))


def test_pack_fingerprints_accepts_0_1_integers_and_rejects_vectors():
    bits = np.array([[0, 1, 0, 0, 1], [1, 1, 1, 1, 1]], dtype=np.int8)
    F = ss.pack_fingerprints(bits)
    assert [int(F[0, 0]), int(F[1, 0])] == [0b10010, 0b11111]
    with pytest.raises(ValueError):
        ss.pack_fingerprints(np.ones(8))


def test_tanimoto_symbols_are_declared_and_bound():
    names = {"ss_similarity_tanimoto_csr_f32", "ss_similarity_tanimoto_csr_f64",
             "ss_graph_create_fingerprint_f32", "ss_graph_create_fingerprint_f64"}
    assert names <= set(_lib.header_symbols())
    assert names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)


def test_entry_points_need_ss_init():
    """Without ss_init every fingerprint entry point returns SS_ENODEV (no CPU fallback), and nothing is written."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    F = ss.pack_fingerprints(np.eye(4, 70, dtype=bool))
    ptr = np.full(5, -7, np.int64)
    nnz = C.c_int64(-7)
    for suf, ft in (("f32", C.c_float), ("f64", C.c_double)):
        rc = getattr(lib, f"ss_similarity_tanimoto_csr_{suf}")(F.ctypes.data, 4, None, 4, F.shape[1], ft(0.5), 1,
                                                               ptr.ctypes.data, None, None, 0, C.byref(nnz), 0)
        assert rc == -4, (suf, rc)
        assert "ss_init" in lib.ss_last_error().decode()
        h = C.c_void_p()
        yp, yi, yv = np.array([0, 1, 1, 2, 2], np.int64), np.array([0, 1], np.int32), None
        rc = getattr(lib, f"ss_graph_create_fingerprint_{suf}")(0, 4, 2, F.shape[1], None, F.ctypes.data,
                                                                yp.ctypes.data, yi.ctypes.data, yv, 0, ft(0.5), 1, 0,
                                                                C.byref(h))
        assert rc == -4, (suf, rc)
        assert h.value is None
    assert nnz.value == -7 and (ptr == -7).all()
    # the Python mirror raises instead of falling back
    with pytest.raises(ss.SimSpreadError) as e:
        ss.tanimoto_csr(F, alpha=0.5)
    assert e.value.code == -4
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_fingerprints(None, F, np.eye(4, 2), alpha=0.5)
    assert e.value.code == -4
