"""The cutoff-profile entry points (include/simspread_hip_profile.h): the library exports every declared symbol, and the
three descriptions of each signature -- C header, ctypes table (_lib.PROFILE_SIGNATURES), Julia `ccall`
(julia/SimSpreadProfile.jl) -- agree type class by type class, as tests/test_half_abi.py holds the 16-bit header's.  The
main header includes the new one and keeps its own 117 declarations."""
import os
import re

from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ({f"ss_similarity_{p}_profile_{s}" for p in ("tanimoto", "jaccard", "dot") for s in ("f32", "f64")}
         | {"ss_similarity_dot_profile_h16"})


def _header_signatures():
    with open(_lib.PROFILE_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_profile_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.profile_header_symbols()
    assert set(declared) == NAMES and len(declared) == 7
    assert sorted(_lib.PROFILE_SIGNATURES) == declared
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    # the new exports live in the new header only
    others = (_lib.HEADER_PATH, _lib.SCREENING_HEADER_PATH, _lib.NEIGHBOURS_HEADER_PATH, _lib.REAL_NEIGHBOURS_HEADER_PATH,
              _lib.CLUSTERS_HEADER_PATH, _lib.TARGET_RANK_HEADER_PATH, _lib.HALF_HEADER_PATH)
    for p in others:
        assert not set(declared) & set(_lib.header_symbols(p)), p
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.HALF_SIGNATURES))
    assert len(_lib.header_symbols()) == 117
    with open(_lib.HEADER_PATH) as f:
        assert '#include "simspread_hip_profile.h"' in f.read()
    # the whole ABI: the main header and its seven companions
    assert sum(len(_lib.header_symbols(p)) for p in others) + len(declared) == 195


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.PROFILE_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadProfile.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 7
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_rule_is_in_the_header_and_the_python_mirror_exposes_the_profiles():
    import inspect

    import simspread_jl_amd as ss
    with open(_lib.PROFILE_HEADER_PATH) as f:
        text = f.read()
    for phrase in ("Pair (i, j) counts for cut b iff `s >= cuts[b] and v != 0`", "A NaN `s` counts for none",
                   "There is no 2^31 refusal here", "`1 <= ncuts <= 32`", '"dot_h16_profile"'):
        assert phrase in text, phrase
    for name in ("CutoffProfile", "tanimoto_profile", "jaccard_profile", "dot_profile"):
        assert name in ss.__all__ and callable(getattr(ss, name)), name
    p = inspect.signature(ss.dot_profile).parameters
    assert p["metric"].default == "cosine" and p["storage"].default is None and p["weighted"].default is True
    for fn in (ss.tanimoto_profile, ss.jaccard_profile, ss.dot_profile):
        assert list(inspect.signature(fn).parameters)[:2] == ["Fa", "Fb"]
        assert "cuts" in inspect.signature(fn).parameters
