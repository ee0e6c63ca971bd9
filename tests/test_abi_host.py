"""The C ABI as one table (sketchedit_amd/_lib.py ABI) against the headers of include/ and the built library: names, order, counts,
signatures, exports and the #define'd constants, for all headers at once.  CPU only."""
import ctypes
import os
import re

import abi_util
from sketchedit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# entries per header, in the order the features arrived: the one literal that holds every list's length
COUNTS = {"sketchedit_hip.h": 54, "sketchedit_png.h": 3, "sketchedit_jpg.h": 3, "sketchedit_jpg2.h": 5, "sketchedit_feather.h": 1,
          "sketchedit_fill.h": 4, "sketchedit_select.h": 3, "sketchedit_lasso.h": 2, "sketchedit_outline.h": 2, "sketchedit_move.h": 2,
          "sketchedit_warp.h": 2, "sketchedit_filter.h": 2, "sketchedit_adjust.h": 4, "sketchedit_modify.h": 1, "sketchedit_blend.h": 2,
          "sketchedit_canvas.h": 1}

SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def _code(name):
    """a header's text without its comments"""
    text = open(os.path.join(INCLUDE, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _prototypes(name):
    """[(entry, return type, [parameter, ..])] of one header in declaration order: the statements that begin a line with a return
    type of int, size_t, void or const char*"""
    found = re.findall(r"^(int|size_t|void|const char\s*\*)\s*(\w+)\s*\(([^)]*)\)\s*;", _code(name), re.M)
    protos = []
    for ret, entry, params in found:
        params = [" ".join(p.split()) for p in params.split(",")]
        protos.append((entry, re.sub(r"\s*\*", "*", ret), [] if params in ([""], ["void"]) else params))
    return protos


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _param_matches(param, t):
    if "*" in param or "[" in param:
        return _is_pointer(t)
    ctype = " ".join(param.split()[:-1])          # without the parameter's name
    return ctype in SCALARS and t is SCALARS[ctype]


def test_headers_and_table_agree():
    assert set(os.listdir(INCLUDE)) == set(_lib.ABI)
    for header, rows in _lib.ABI.items():
        assert [p[0] for p in _prototypes(header)] == [r[0] for r in rows] == _lib.abi_names(header), header
    assert _lib.abi_names() == [r[0] for rows in _lib.ABI.values() for r in rows]


def test_counts_are_pinned_once():
    assert {h: len(rows) for h, rows in _lib.ABI.items()} == COUNTS and list(_lib.ABI) == list(COUNTS)
    names = _lib.abi_names()
    assert len(names) == 91 == len(set(names)) and all(n.startswith("se_") for n in names)
    assert _lib.ABI_OPTIONAL == {"se_debug_gconv_form"} and _lib.ABI_OPTIONAL <= set(names)


def _signature_mismatches():
    bad = []
    for header, rows in _lib.ABI.items():
        for (entry, ret, params), (name, restype, argtypes) in zip(_prototypes(header), rows):
            if entry != name or restype is not RETURNS[ret] or len(params) != len(argtypes):
                bad.append((header, name, "return type or parameter count"))
            else:
                bad += [(header, name, p) for p, t in zip(params, argtypes) if not _param_matches(p, t)]
    return bad


def test_signatures_match_the_prototypes():
    assert sum(len(_prototypes(h)) for h in _lib.ABI) == 91
    assert _signature_mismatches() == []


def test_exports_match_the_table():
    names = _lib.abi_names()
    exported = abi_util.exported_names(("se_", "sk"))          # "sk": no entry under the library's own name, whole or shortened
    assert exported == set(names), exported ^ set(names)
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert getattr(raw, n) is not None
    lib = _lib.load_library()
    for rows in _lib.ABI.values():
        for name, restype, argtypes in rows:
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def _defines():
    """[(header, macro, value text or None)] of every #define in include/"""
    return [(h, m, v.strip() or None) for h in sorted(os.listdir(INCLUDE))
            for m, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", _code(h), re.M)]


def _define_mismatches(defines):
    bad = []
    for header, macro, value in defines:
        if value is None:                     # only a header's own include guard has no value
            if macro != header.upper().replace(".", "_"):
                bad.append((header, macro, "no value"))
            continue
        if not macro.startswith("SE_") or not re.fullmatch(r"[0-9()<\-l \t]+", value):
            bad.append((header, macro, value))
            continue
        want = eval(value.replace("l", ""), {"__builtins__": {}})          # digits, brackets, << and - alone (checked above)
        short = macro[len("SE_"):]
        got = getattr(_lib, short) if hasattr(_lib, short) else getattr(_lib, macro, None)
        if got is None or got != want:
            bad.append((header, macro, value, got))
    return bad


def test_every_define_has_its_python_mirror():
    defines = _defines()
    valued = [d for d in defines if d[2] is not None]
    assert len(valued) == 51 and len(defines) == 51 + len(_lib.ABI)
    assert _define_mismatches(defines) == []
    assert [m for _, m, v in valued if not hasattr(_lib, m[3:])] == ["SE_JPG_420", "SE_JPG_OPTIMIZE"]
    assert ("sketchedit_warp.h", "SE_WARP_MAX_TRANSLATION", "(1ll << 40)") in valued and _lib.WARP_MAX_TRANSLATION == 1 << 40


def test_the_checks_fail_when_broken(monkeypatch):
    """a row one int short, a pointer bound as an int, a mirror of another value, a define without a mirror and a macro under
    another prefix are each found"""
    rows = _lib.ABI["sketchedit_png.h"]
    name, restype, argtypes = rows[0]
    monkeypatch.setitem(_lib.ABI, "sketchedit_png.h", [(name, restype, argtypes[:-1])] + rows[1:])
    assert _signature_mismatches() == [("sketchedit_png.h", "se_png_bound", "return type or parameter count")]
    monkeypatch.setitem(_lib.ABI, "sketchedit_png.h", rows[:2] + [(rows[2][0], rows[2][1], [ctypes.c_int] + rows[2][2][1:])])
    assert _signature_mismatches() == [("sketchedit_png.h", "se_png_encode_u8_workspace_bytes", "se_ctx* ctx")]
    monkeypatch.setitem(_lib.ABI, "sketchedit_png.h", rows)
    monkeypatch.setattr(_lib, "FEATHER_MAX_RADIUS", 17)
    assert _define_mismatches(_defines()) == [("sketchedit_feather.h", "SE_FEATHER_MAX_RADIUS", "16", 17)]
    assert _define_mismatches([("sketchedit_x.h", "SE_NO_MIRROR", "1")]) == [("sketchedit_x.h", "SE_NO_MIRROR", "1", None)]
    assert _define_mismatches([("sketchedit_x.h", "SX_FEATHER_MAX_RADIUS", "16")]) == [("sketchedit_x.h", "SX_FEATHER_MAX_RADIUS", "16")]
