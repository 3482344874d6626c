"""The screening entry points (include/simspread_hip_screening.h: query sets, support lists): the library exports every
declared symbol, and the three descriptions of each signature -- C header, ctypes table (_lib.SCREENING_SIGNATURES), Julia
`ccall` (julia/SimSpreadScreening.jl) -- agree type class by type class, as tests/test_julia_binding.py holds the main
header's.  The main header includes the screening header, so a C caller sees one ABI."""
import os
import re

from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_queries_destroy", "ss_queries_info", "ss_queries_degrees"} | {
    f"{n}_{suf}" for suf in ("f32", "f64")
    for n in ("ss_queries_create_csr", "ss_queries_create_fingerprint", "ss_queries_create_features",
              "ss_queries_create_vectors", "ss_predict_queries", "ss_support")}


def _header_signatures():
    with open(_lib.SCREENING_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_screening_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.screening_header_symbols()
    assert set(declared) == NAMES and len(declared) == 15
    assert sorted(_lib.SCREENING_SIGNATURES) == declared
    assert not set(declared) & set(_lib.SIGNATURES)
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    assert len(_lib.header_symbols()) + len(declared) == 132
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_screening.h"' in main
    assert "SS_ROWS_LOO = 2" in main and "typedef struct ss_queries ss_queries;" in main
    assert _lib.SS_ROWS_LOO == 2


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.SCREENING_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadScreening.jl"))
    assert {c[0] for c in calls} == NAMES
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_mirror_exposes_the_handles():
    import simspread_jl_amd as ss
    assert "DeviceQueries" in ss.__all__
    for m in ("from_sparse", "from_fingerprints", "from_features", "from_vectors", "degrees", "close"):
        assert callable(getattr(ss.DeviceQueries, m))
    assert callable(ss.DeviceGraph.support)
