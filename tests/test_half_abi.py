"""The 16-bit entry points (include/simspread_hip_half.h: the inner-product producer on bf16 / fp16 rows): the library
exports every declared symbol, and the three descriptions of each signature -- C header, ctypes table
(_lib.HALF_SIGNATURES), Julia `ccall` (julia/SimSpreadHalf.jl) -- agree type class by type class, as
tests/test_screening_abi.py holds the screening header's.  The main header includes the new one and keeps its own 117
declarations."""
import os
import re

from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_similarity_dot_csr_h16", "ss_graph_create_vectors_h16", "ss_queries_create_vectors_h16"}


def _header_signatures():
    with open(_lib.HALF_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_half_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.half_header_symbols()
    assert set(declared) == NAMES and len(declared) == 3
    assert sorted(_lib.HALF_SIGNATURES) == declared
    assert not set(declared) & set(_lib.SIGNATURES)
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    assert len(_lib.header_symbols()) == 117
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_half.h"' in main
    with open(_lib.HALF_HEADER_PATH) as f:
        half = f.read()
    assert "SS_H16_BF16 = 0, SS_H16_F16 = 1" in half and "ROW-MAJOR" in half
    assert (_lib.SS_H16_BF16, _lib.SS_H16_F16) == (0, 1)
    # the whole ABI: the main header and its six companions
    total = sum(len(_lib.header_symbols(p)) for p in (
        _lib.HEADER_PATH, _lib.SCREENING_HEADER_PATH, _lib.NEIGHBOURS_HEADER_PATH, _lib.REAL_NEIGHBOURS_HEADER_PATH,
        _lib.CLUSTERS_HEADER_PATH, _lib.TARGET_RANK_HEADER_PATH, _lib.HALF_HEADER_PATH))
    assert total == 188


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.HALF_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadHalf.jl"))
    assert {c[0] for c in calls} == NAMES
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_mirror_exposes_the_route():
    import inspect

    import simspread_jl_amd as ss
    assert "to_bf16_bits" in ss.__all__ and callable(ss.to_bf16_bits)
    for fn in (ss.dot_csr, ss.DeviceGraph.from_vectors, ss.DeviceQueries.from_vectors):
        assert inspect.signature(fn).parameters["storage"].default is None
