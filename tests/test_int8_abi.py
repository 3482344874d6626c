"""The int8 entry points (include/simspread_hip_int8.h: the inner-product producer and its neighbour floor on int8 rows):
the library exports every declared symbol, and the three descriptions of each signature -- C header, ctypes table
(_lib.INT8_SIGNATURES), Julia `ccall` (julia/SimSpreadInt8.jl) -- agree type class by type class, as
tests/test_half_abi.py holds the 16-bit header's.  The main header includes the new one and keeps its own 117
declarations."""
import os
import re

from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_similarity_dot_csr_i8", "ss_similarity_dot_kth_i8", "ss_graph_create_vectors_i8",
         "ss_queries_create_vectors_i8"}


def _header_signatures():
    with open(_lib.INT8_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_int8_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.int8_header_symbols()
    assert set(declared) == NAMES and len(declared) == 4
    assert sorted(_lib.INT8_SIGNATURES) == declared
    others = (set(_lib.SIGNATURES) | set(_lib.SCREENING_SIGNATURES) | set(_lib.NEIGHBOUR_SIGNATURES)
              | set(_lib.REAL_NEIGHBOUR_SIGNATURES) | set(_lib.CLUSTER_SIGNATURES) | set(_lib.TARGET_RANK_SIGNATURES)
              | set(_lib.HALF_SIGNATURES) | set(_lib.PROFILE_SIGNATURES))
    assert not set(declared) & others
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    assert len(_lib.header_symbols()) == 117
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_int8.h"' in main
    with open(_lib.INT8_HEADER_PATH) as f:
        text = f.read()
    for word in ("ROW-MAJOR", "131071", "round-to-nearest-even", "s(j, i) agree bit for bit"):
        assert word in text, word
    # the companions that came before keep their counts
    assert len(_lib.half_header_symbols()) == 3 and len(_lib.real_neighbours_header_symbols()) > 0


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.INT8_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadInt8.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 4
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_mirror_exposes_the_route():
    import inspect

    import simspread_jl_amd as ss
    for name in ("quantize_i8", "dot_kth_i8"):
        assert name in ss.__all__ and callable(getattr(ss, name))
    for fn in (ss.dot_csr, ss.DeviceGraph.from_vectors, ss.DeviceQueries.from_vectors):
        assert inspect.signature(fn).parameters["storage"].default is None
    # dot_kth keeps its parameter list (tests/test_real_floor_cpu.py pins it): the int8 selection is dot_kth_i8
    assert list(inspect.signature(ss.dot_kth_i8).parameters) == ["Fa", "Fb", "metric", "k"]
    assert inspect.signature(ss.dot_kth_i8).parameters["k"].default is None
