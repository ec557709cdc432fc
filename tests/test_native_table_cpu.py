"""The ctypes binding's parameter table (_native.ENTRIES) against include/gsrast.h, its by-name
argument ordering, and the derived SIGNATURES against the values recorded before the table was named
(tests/golden/native_signatures.json).  No GPU."""
import ctypes
import json
import os
import re

import pytest

from diff_gaussian_rasterization import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "void": None}


def prototypes():
    """[(name, return type, [(type, parameter name)])] of every function include/gsrast.h declares."""
    with open(os.path.join(ROOT, "include", "gsrast.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    text = re.sub(r"typedef\s+struct[^{]*\{.*?\}[^;]*;", " ", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    out = []
    for m in re.finditer(r"([\w\s*]+?)\b(gs_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                t, name = re.match(r"^(.*?)(\w+)$", p.strip(), flags=re.S).groups()
                params.append((" ".join(t.split()), name))
        out.append((m.group(2), " ".join(m.group(1).split()), params))
    return out


def matches(c_type, ct):
    """Is the ctypes object `ct` a binding of the C type?  Pointers (and the allocator callback) are
    c_void_p or a POINTER(...) of the pointee; char* is c_char_p; scalars are their ctypes, compared as
    objects (c_longlong is c_long on LP64)."""
    t = c_type.replace("const", " ")
    base = " ".join(t.replace("*", " ").split())
    if "*" in t or base == "gs_alloc_fn":
        if base == "char" and t.count("*") == 1:
            return ct is ctypes.c_char_p
        if ct is ctypes.c_void_p:
            return True
        pointee = _native.ViewGrad if base == "gs_view_grad" else _SCALARS.get(base, False)
        return t.count("*") == 1 and pointee not in (False, None) and ct is ctypes.POINTER(pointee)
    return base in _SCALARS and ct is _SCALARS[base]


def test_table_is_the_header():
    protos = prototypes()
    assert len(protos) == len(_native.SIGNATURES) == len(_native.ENTRIES) == 83
    assert len({p[0] for p in protos}) == len(protos)
    for name, ret, params in protos:
        res, table = _native.ENTRIES[name]
        assert matches(ret, res), (name, ret, res)
        assert [n for n, _ in table] == [n for _, n in params], name
        for (c_type, pname), (_, ct) in zip(params, table):
            assert matches(c_type, ct), (name, pname, c_type, ct)
        assert _native.SIGNATURES[name] == (res, [ct for _, ct in table]), name


def test_the_type_rule_tells_types_apart():
    """(what the comparison above can see: a float bound as a double, a pointer as an int, a wrong pointee)"""
    assert matches("float", ctypes.c_float) and not matches("float", ctypes.c_double)
    assert matches("long long", ctypes.c_longlong) and not matches("long long", ctypes.c_int)
    assert matches("unsigned", ctypes.c_uint) and not matches("unsigned", ctypes.c_int)
    assert matches("const float*", ctypes.c_void_p) and not matches("const float*", ctypes.c_int)
    assert matches("long long*", ctypes.POINTER(ctypes.c_longlong))
    assert not matches("long long*", ctypes.POINTER(ctypes.c_double)) and not matches("int", ctypes.c_void_p)
    assert matches("char*", ctypes.c_char_p) and not matches("char*", ctypes.c_void_p)
    assert matches("const char*", ctypes.c_char_p) and matches("void", None) and not matches("int", None)
    assert matches("const gs_view_grad*", ctypes.POINTER(_native.ViewGrad))
    assert matches("gs_alloc_fn", ctypes.c_void_p) and matches("void**", ctypes.c_void_p)
    assert not matches("float* const*", ctypes.POINTER(ctypes.c_float))


def test_ordered():
    x = ctypes.c_void_p(64)
    got = _native.ordered("gs_knn_mean_dist2", stream=None, out=x, P=5, scratch=None, points=x)
    assert got == [5, x, x, None, None] and got[3] is None  # a pointer's None passes through
    assert _native.ordered("gs_abi_version") == []
    wide = {n: k for k, (n, _) in enumerate(_native.ENTRIES["gs_backward_accumulate_absgrad"][1])}
    assert _native.ordered("gs_backward_accumulate_absgrad", **dict(reversed(list(wide.items())))) == list(range(43))
    with pytest.raises(TypeError, match="unknown argument.*'colour'"):
        _native.ordered("gs_knn_mean_dist2", P=5, points=x, out=x, scratch=None, stream=None, colour=None)
    with pytest.raises(TypeError, match="missing argument 'scratch'"):
        _native.ordered("gs_knn_mean_dist2", P=5, points=x, out=x, stream=None)
    with pytest.raises(TypeError):  # a misspelt name: one missing, one unknown
        _native.ordered("gs_knn_mean_dist2", P=5, points=x, out=x, scratch=None, strem=None)


def _canonical(t):
    if t is None:
        return "void"
    if t is _native.ViewGrad:
        return "ViewGrad"
    for name in ("c_void_p", "c_char_p", "c_int", "c_uint", "c_longlong", "c_size_t", "c_float", "c_double"):
        if t is getattr(ctypes, name):
            return name
    return "POINTER(%s)" % _canonical(t._type_)


def test_signatures_are_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "native_signatures.json")) as f:
        recorded = json.load(f)
    assert set(recorded) == set(_native.SIGNATURES)
    for name, (res, args) in _native.SIGNATURES.items():
        assert [_canonical(res), [_canonical(a) for a in args]] == recorded[name], name
