"""The Python declaration of the C ABI (mpsfm_amd/abi.py) against the two headers, by the compiler and by a parse.

Layout: a C++ program generated from the ctypes classes prints sizeof / offsetof of every struct and field as the host compiler
sees include/mpsfm_hip.h; every number must equal ctypes'.  Signatures: every prototype of the headers against SIGNATURES /
DEBUG_SIGNATURES.  Binding: the loader types every function once, and nothing else in the package assigns a signature."""

import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from mpsfm_amd import abi
from mpsfm_amd.build import _hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PUBLIC, DEBUG = os.path.join(INCLUDE, "mpsfm_hip.h"), os.path.join(INCLUDE, "mpsfm_hip_debug.h")


def _text(path):
    """The header without comments."""
    s = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", s)


def _header_structs():
    """{struct name: [field names in order]} of every `typedef struct ... { ... } name;` of the two headers."""
    out = {}
    for path in (PUBLIC, DEBUG):
        for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", _text(path), flags=re.S):
            assert name not in out, f"{name} is defined twice"
            fields = []
            for decl in body.split(";"):
                decl = re.sub(r"\[[^\]]*\]", "", decl).strip()  # double K[4] -> double K
                if decl:
                    fields += [re.findall(r"\w+", d)[-1] for d in decl.split(",")]  # int32_t H, W -> H, W
            out[name] = fields
    return out


def _mirrors():
    """{C struct name: ctypes class} of abi.py; an alias of a class (CAbsPoseOptions = CRansacOptions) counts once."""
    classes = {id(v): v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    out = {}
    for cls in classes.values():
        name = cls.__dict__.get("_c_name_")
        assert name, f"abi.{cls.__name__} does not name its C struct (_c_name_)"
        assert name not in out, f"{name} has two mirrors: {out.get(name)} and {cls}"
        out[name] = cls
    return out


def _split_params(params):
    """One string per parameter; a function-pointer parameter has commas of its own, inside parentheses."""
    return [" ".join(p.split()) for p in re.sub(r"\([^()]*\)", "(*)", params).split(",")]


def _c_kind(decl):
    """pointer / charp / int32 / int64 / double / float / void of a C return type or parameter declaration."""
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    if "*" in decl or "[" in decl or "(" in decl:  # arrays and function pointers decay to pointers
        return "charp" if words[0] == "char" and "(" not in decl else "pointer"
    kinds = {"int": "int32", "int32_t": "int32", "int64_t": "int64", "double": "double", "float": "float", "void": "void"}
    assert words[0] in kinds, f"unknown C type in {decl!r}"
    return kinds[words[0]]


def _header_prototypes(path):
    """{function: (return kind, [parameter kinds])} of every prototype of one header."""
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?[\s\*])(mpsfm_\w+)\s*\(([^;{]*)\)\s*;", _text(path), flags=re.M):
        if ret.split()[0] == "typedef":
            continue
        assert name not in out, f"{name} is declared twice"
        kinds = [_c_kind(p) for p in _split_params(params)]
        out[name] = (_c_kind(ret), [] if kinds == ["void"] else kinds)
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "charp"
    if t is C.c_void_p or issubclass(t, (C._Pointer, C._CFuncPtr)):
        return "pointer"
    kinds = {C.c_int32: "int32", C.c_int64: "int64", C.c_double: "double", C.c_float: "float"}  # c_int is c_int32: the header's `int`
    assert t in kinds, f"unexpected ctypes type {t}"
    return kinds[t]


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """{struct: size}, {(struct, field): (offset, size)} as the host compiler lays out the headers' structs."""
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "mpsfm_hip_debug.h"', "int main() {"]
    for name, cls in _mirrors().items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        for field, *_ in cls._fields_:
            lines.append(f'  std::printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    lines += ["  return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-I", INCLUDE, str(src), "-o", str(exe)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "the layout probe does not compile against the headers:\n" + r.stdout
    sizes, fields = {}, {}
    for line in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        if "." in key:
            fields[tuple(key.split("."))] = (int(nums[0]), int(nums[1]))
        else:
            sizes[key] = int(nums[0])
    return sizes, fields


def test_every_struct_has_one_mirror_with_the_compilers_layout(compiled_layout):
    declared, mirrors = _header_structs(), _mirrors()
    assert len(declared) >= 36, "the struct parse lost structs (36 when this test was written)"
    assert set(declared) == set(mirrors), f"structs and mirrors differ: {sorted(set(declared) ^ set(mirrors))}"
    sizes, fields = compiled_layout
    checked = 0
    for name, cls in mirrors.items():
        assert [f[0] for f in cls._fields_] == declared[name], f"{name}: field names or order differ from the header"
        assert C.sizeof(cls) == sizes[name], f"sizeof({name})"
        for field, *_ in cls._fields_:
            d = getattr(cls, field)
            assert (d.offset, d.size) == fields[(name, field)], f"{name}.{field}: ctypes (offset, size) against the compiler's"
            checked += 1
    assert checked == len(fields) == sum(len(f) for f in declared.values())  # no field left out on either side
    print(f"{len(mirrors)} structs, {checked} fields agree with the compiler")


def test_every_prototype_agrees_with_its_table_entry():
    total = 0
    for path, table, least in ((PUBLIC, abi.SIGNATURES, 63), (DEBUG, abi.DEBUG_SIGNATURES, 15)):
        protos = _header_prototypes(path)
        assert len(protos) >= least, f"the prototype parse of {os.path.basename(path)} lost functions ({least} when this test was written)"
        assert set(protos) == set(table), f"{os.path.basename(path)} and its table differ: {sorted(set(protos) ^ set(table))}"
        for name, (ret, params) in protos.items():
            restype, argtypes = table[name]
            assert _ctypes_kind(restype) == ret, f"{name}: return type"
            assert [_ctypes_kind(t) for t in argtypes] == params, f"{name}: parameters"
        total += len(protos)
    assert all(name.startswith("mpsfm_debug_") for name in abi.DEBUG_SIGNATURES)
    assert not any(name.startswith("mpsfm_debug_") for name in abi.SIGNATURES)
    print(f"{total} prototypes agree with the tables")


def test_the_loader_binds_every_function_once_and_nothing_else_does():
    L = abi.lib()
    assert abi.lib() is L
    for table in (abi.SIGNATURES, abi.DEBUG_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            assert hasattr(L, name), f"{name} is in the table but not exported"
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    others = [p for p in glob.glob(os.path.join(ROOT, "mpsfm_amd", "**", "*.py"), recursive=True) if not os.path.samefile(p, abi.__file__)]
    offenders = [os.path.relpath(p, ROOT) for p in others if re.search(r"\.(argtypes|restype)\b", open(p).read())]
    assert not offenders, f"signatures are declared in abi.py alone, not in {offenders}"
