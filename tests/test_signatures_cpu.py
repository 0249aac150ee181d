"""CPU: dcpt_amd._lib.SIGNATURES against include/dcpt_hip.h, argument by argument.  The table is written by hand and every call site of
dcpt_amd/functional.py is written against it; tests/test_abi_cpu.py compares the names only.  Here every declaration of the header is parsed
and every parameter (and the result) mapped to a kind -- any ``*`` or ``dcpt_stream_t`` is a pointer, otherwise int / int64_t / size_t /
float / double / long long -- and compared with the kind of the ctypes type in the same position."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCALARS = ("long long", "int64_t", "size_t", "double", "float", "int")   # ("long long" before "int": the first match names the kind)
_CTYPES = {C.c_int: "int", C.c_int64: "int64_t", C.c_size_t: "size_t", C.c_float: "float", C.c_double: "double", C.c_longlong: "long long"}
# c_int64 and c_longlong (and, on LP64, c_size_t's unsigned twin) are one ctypes class per width: kinds compare by width and signedness
_WIDTH = {"int": (4, True), "int64_t": (8, True), "long long": (8, True), "size_t": (C.sizeof(C.c_size_t), False), "float": "f4", "double": "f8"}


def _c_kind(decl: str) -> str:
    decl = decl.strip()
    if "*" in decl or re.search(r"\bdcpt_stream_t\b", decl) or "[" in decl:
        return "pointer"
    for s in _SCALARS:
        if re.search(rf"\b{s}\b", decl):
            return s
    raise AssertionError(f"dcpt_hip.h: cannot classify {decl!r}")


def _ctypes_kind(t) -> str:
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C.Array))):
        return "pointer"
    if t in _CTYPES:
        return _CTYPES[t]
    if t is C.c_uint64 or t is C.c_ulong:
        return "size_t"
    raise AssertionError(f"_lib.SIGNATURES: cannot classify {t!r}")


def _same(a: str, b: str) -> bool:
    return a == b or (a != "pointer" and b != "pointer" and _WIDTH[a] == _WIDTH[b])


def _header_declarations():
    """{name: (result kind, [parameter kinds])} of every dcpt_* function the header declares"""
    txt = open(os.path.join(ROOT, "include", "dcpt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = "\n".join(ln for ln in txt.splitlines() if not ln.lstrip().startswith("#"))
    txt = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", txt, flags=re.S)   # struct bodies hold no declarations
    decls = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(dcpt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        res, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in decls, f"{name} declared twice"
        kinds = [] if params in ("", "void") else [_c_kind(p) for p in params.split(",")]
        decls[name] = (_c_kind(res), kinds)
    return decls


def test_ctypes_table_matches_header_argument_by_argument():
    from dcpt_amd import _lib

    decls = _header_declarations()
    assert len(decls) >= 150, f"only {len(decls)} declarations parsed"
    assert sorted(decls) == sorted(_lib.SIGNATURES), "ctypes table and header name different entry points"
    bad = []
    for name, (res, kinds) in decls.items():
        cres, cargs = _lib.SIGNATURES[name]
        if not _same(res, _ctypes_kind(cres)):
            bad.append(f"{name}: result {res} in the header, {_ctypes_kind(cres)} in the table")
        if len(kinds) != len(cargs):
            bad.append(f"{name}: {len(kinds)} parameters in the header, {len(cargs)} in the table")
            continue
        for i, (k, t) in enumerate(zip(kinds, cargs)):
            if not _same(k, _ctypes_kind(t)):
                bad.append(f"{name}: parameter {i} is {k} in the header, {_ctypes_kind(t)} in the table")
    assert not bad, "\n".join(bad)


def test_parser_tells_the_kinds_apart():
    assert _c_kind("const float* x") == "pointer" and _c_kind("dcpt_stream_t stream") == "pointer"
    assert _c_kind("const dcpt_nafblock_params* p") == "pointer" and _c_kind("int64_t M") == "int64_t"
    assert _c_kind("size_t ws_bytes") == "size_t" and _c_kind("float eps") == "float" and _c_kind("int C") == "int"
    assert not _same("int", "int64_t") and not _same("float", "int") and not _same("pointer", "size_t") and not _same("float", "double")
