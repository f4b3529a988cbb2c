"""CPU: the ctypes binding against the public headers.  Every row of _capi.SIGNATURES against its prototype (arity, the class of
every parameter, the return class), the five mirrored structs against a C program that prints their layout, and the integer
#defines against the constants of the same name.  The per-feature tests keep what is theirs (the expected names of a header, the
enum orders, package.__all__); what holds for every header alike is asserted here, once."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from reinforcementlearning4meshgeneration_amd import _capi, build

INCLUDE = os.path.join(ROOT, "include")
STRUCTS = ("MeshEnvParams", "MeshEvalBuffers", "MeshKeepEntry", "MeshOptimScalars", "MeshOptimCounted")
SCALARS = {"int": "int", "int32_t": "int", "int64_t": "int64_t", "uint64_t": "uint64_t", "float": "float", "double": "double"}
CTYPES = {C.c_int: "int", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_float: "float", C.c_double: "double", None: "void"}


def _code(header):
    """The header without comments and preprocessor lines."""
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)


def _c_class(decl, header):
    """The class of one parameter or return type as the header spells it: 'pointer', a scalar of SCALARS, or 'void'."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in {**SCALARS, "void": "void"}, f"{header}: cannot classify '{decl}'"
    return {**SCALARS, "void": "void"}[words[0]]


def _prototypes(header):
    """{name: (return class, [parameter classes])} of every `ret name(args);` the header declares, in its order."""
    found = re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(meshenv_\w+)\s*\(([^()]*)\)\s*;", _code(header))
    names = [name for _, name, _ in found]
    assert len(names) == len(set(names)), f"{header} declares a function twice"
    out = {}
    for ret, name, args in found:
        args = args.strip()
        params = [] if args in ("void", "") else [a.strip() for a in args.split(",")]
        for p in params:    # a parameter is a type and a name: a bare `int` would hide a word of the type from _c_class
            assert "*" in p or len([w for w in p.split() if w != "const"]) == 2, f"{header}: {name}: parameter '{p}'"
        out[name] = (_c_class(ret, header), [_c_class(p, header) for p in params])
    return out


def _ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "pointer"
    return CTYPES[t]


PROTOTYPES = {h: _prototypes(h) for h in build.PUBLIC_HEADERS}


def test_the_table_has_the_headers_of_the_build_and_their_names_once():
    assert sorted(_capi.SIGNATURES) == sorted(build.PUBLIC_HEADERS) and len(set(build.PUBLIC_HEADERS)) == len(build.PUBLIC_HEADERS)
    for header, rows in _capi.SIGNATURES.items():
        assert set(rows) == set(PROTOTYPES[header]), (header, set(rows) ^ set(PROTOTYPES[header]))
    every = [name for rows in _capi.SIGNATURES.values() for name in rows]
    assert len(every) == len(set(every)) == 175         # no name twice: the groups are pairwise disjoint over all headers
    assert len(_capi.SIGNATURES["meshenv.h"]) == 82
    headers = list(_capi.SIGNATURES)
    for a in range(len(headers)):
        for b in range(a + 1, len(headers)):
            assert not set(_capi.SIGNATURES[headers[a]]) & set(_capi.SIGNATURES[headers[b]]), (headers[a], headers[b])


def test_the_export_lists_are_the_groups_of_the_table():
    lists = {k: v for k, v in vars(_capi).items() if k.startswith("EXPORTS")}
    assert len(lists) == len(_capi.SIGNATURES) == 16
    for key, names in lists.items():
        header = "meshenv" + key[len("EXPORTS"):].lower() + ".h"
        assert names == list(_capi.SIGNATURES[header]), key


@pytest.mark.parametrize("header", build.PUBLIC_HEADERS)
def test_every_row_agrees_with_its_prototype(header):
    rows = _capi.SIGNATURES[header]
    assert len(PROTOTYPES[header]) >= 1
    for name, (ret, params) in PROTOTYPES[header].items():
        restype, argtypes = rows[name]
        assert _ctypes_class(restype) == ret, f"{name}: returns {ret} in {header}, {restype} in the table"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in {header}, {len(argtypes)} in the table"
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert _ctypes_class(t) == p, f"{name}: parameter {k} is {p} in {header}, {t} in the table"


def test_load_sets_every_row_on_the_library():
    assert os.path.exists(build.LIB_PATH), "run `python -m reinforcementlearning4meshgeneration_amd.build` first"
    L = _capi.load()
    for rows in _capi.SIGNATURES.values():
        for name, (restype, argtypes) in rows.items():
            assert hasattr(L, name), f"{name} is declared but not exported by the library"
            fn = getattr(L, name)
            assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes) and fn.restype is restype, name


def _header_fields(struct):
    """The field names of `typedef struct <struct> { ... }`, in the header's order."""
    for header in build.PUBLIC_HEADERS:
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % struct, _code(header), flags=re.S)
        if body:
            pieces = [p for decl in body.group(1).split(";") for p in decl.split(",") if p.strip()]
            return [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", p).group(1) for p in pieces]
    raise AssertionError(f"no public header defines {struct}")


def test_the_struct_mirrors_have_the_layout_the_c_compiler_gives_the_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler on PATH")
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in build.PUBLIC_HEADERS] + ["int main(void) {"]
    for s in STRUCTS:
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        for field in _header_fields(s):
            lines.append(f'    printf("{s}.{field} %zu %zu\\n", offsetof({s}, {field}), sizeof((({s} *)0)->{field}));')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    done = subprocess.run([cc, "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    printed = [line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    for s in STRUCTS:
        cls = getattr(_capi, s)
        mirror = [[s, str(C.sizeof(cls))]] + [[f"{s}.{name}", str(getattr(cls, name).offset), str(getattr(cls, name).size)]
                                             for name, _ in cls._fields_]
        assert [row for row in printed if row[0].split(".")[0] == s] == mirror, s
    assert [C.sizeof(getattr(_capi, s)) for s in STRUCTS] == [80, 184, 24, 104, 104]


def test_the_integer_defines_equal_the_constants_of_the_same_name():
    pairs = 0
    for header in build.PUBLIC_HEADERS:
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+MESHENV_(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M):
            if isinstance(getattr(_capi, name, None), int):
                assert getattr(_capi, name) == int(value), f"{header}: MESHENV_{name} is {value}, _capi.{name} is {getattr(_capi, name)}"
                pairs += 1
    assert pairs >= 48, pairs
