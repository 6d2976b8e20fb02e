"""CPU: everything ``semi_detr_amd._lib`` copies from include/semidetr_hip.h (and semidetr_hip_experiments.h) against the header
itself.  Functions: every declaration is parsed and its return and argument types must equal ``SIGNATURES`` /
``EXPERIMENT_SIGNATURES``.  Structures and constants: one generated C file that includes only the header is compiled with the
oracle's C compiler and prints ``sizeof``, every field's ``offsetof`` / ``sizeof`` / kind and every macro of ``CONSTANTS``; a
field the header does not have fails that compile.  The comparison functions are shown to report a wrong mirror."""
import ctypes
import os
import re
import subprocess

import pytest

from semi_detr_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "void": None}
INTEGERS = ("char", "signed char", "unsigned char", "short", "unsigned short", "int", "unsigned", "long", "unsigned long",
            "long long", "unsigned long long")
C_NAME = {cls: name for name, cls in _lib.STRUCTS.items()}


def _source(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def _ctype(text, is_return=False):
    """The ctypes type of a C parameter ``<type> <name>`` or of a return type."""
    text = " ".join(text.replace("*", " * ").split())
    block = re.match(r"const (semidetr_\w+) \*", text)
    if block and block.group(1) in _lib.STRUCTS:
        return ctypes.POINTER(_lib.STRUCTS[block.group(1)])
    if "*" in text or "[" in text:
        return ctypes.c_char_p if is_return and text == "const char *" else ctypes.c_void_p
    return SCALARS[text if is_return else text.rsplit(" ", 1)[0]]


def declarations(header="semidetr_hip.h"):
    """{function: (restype, argtypes)} as the header declares them."""
    found = re.findall(r"^([\w \t]+?[\s*]+)(semidetr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _source(header), flags=re.M)
    return {name: (_ctype(res, True), [_ctype(a) for a in args.split(",") if a.strip() != "void"]) for res, name, args in found}


def header_fields(struct):
    """The member names of ``typedef struct <struct> { ... } <struct>;`` in the header's order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _source("semidetr_hip.h"), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", d).group(1) for line in body.split(";") for d in line.split(",") if d.strip()]


def signature_mismatches(table, declared):
    out = [f"{n}: in the table, not in the header" for n in table.keys() - declared.keys()]
    out += [f"{n}: declared by the header, not in the table" for n in declared.keys() - table.keys()]
    for n in table.keys() & declared.keys():
        (res, args), (hres, hargs) = table[n], declared[n]
        if res is not hres:
            out.append(f"{n}: returns {hres} in the header, {res} in the table")
        if len(args) != len(hargs):
            out.append(f"{n}: {len(hargs)} arguments in the header, {len(args)} in the table")
        out += [f"{n}: argument {i} is {h} in the header, {a} in the table" for i, (a, h) in enumerate(zip(args, hargs)) if a is not h]
    return out


def _kind(ctype):
    while issubclass(ctype, ctypes.Array):
        ctype = ctype._type_
    if ctype in C_NAME:
        return C_NAME[ctype]
    return {"f": "floating", "d": "floating", "P": "pointer"}.get(ctype._type_, "integer")


def struct_mismatches(name, cls, report):
    """``cls`` against what the compiler reported for the header's ``name`` (``report["S"]``, ``report["F"]``)."""
    names = [f[0] for f in cls._fields_]
    out = [] if names == header_fields(name) else [f"{name}: fields {names}, the header has {header_fields(name)}"]
    if ctypes.sizeof(cls) != report["S"][name]:
        out.append(f"{name}: sizeof {report['S'][name]} in the header, {ctypes.sizeof(cls)} in the mirror")
    for field, ctype in cls._fields_:
        got = (getattr(cls, field).offset, ctypes.sizeof(ctype), _kind(ctype))
        if got != report["F"][name, field]:
            out.append(f"{name}.{field}: (offset, size, kind) {report['F'][name, field]} in the header, {got} in the mirror")
    return out


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """What the C compiler says about the header: {"S": {struct: sizeof}, "F": {(struct, field): (offset, size, kind)},
    "C": {macro: value}}."""
    kinds = [f'{t}: "integer"' for t in INTEGERS] + ['float: "floating"', 'double: "floating"'] + \
            [f'{n}: "{n}"' for n in _lib.STRUCTS]
    lines = ['#include "semidetr_hip.h"', "#include <stdio.h>", "#include <stddef.h>",
             '#define KIND(x) _Generic((x), %s, default: "pointer")' % ", ".join(kinds), "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        for field, ctype in cls._fields_:
            elem = field
            while issubclass(ctype, ctypes.Array):
                elem, ctype = elem + "[0]", ctype._type_
            lines.append(f'    printf("F {name} {field} %zu %zu %s\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}), '
                         f'KIND((({name} *)0)->{elem}));')
    lines += [f'    printf("C {macro} %lld\\n", (long long)({macro}));' for macro in _lib.CONSTANTS]
    tmp = tmp_path_factory.mktemp("cabi_mirror")
    (tmp / "mirror.c").write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    cc = subprocess.run([os.environ.get("CC", "gcc"), "-std=c11", "-I", INCLUDE, str(tmp / "mirror.c"), "-o", str(tmp / "mirror")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr             # a field or macro the header does not have ends here
    out = {"S": {}, "F": {}, "C": {}}
    for tag, *w in (line.split() for line in subprocess.run([str(tmp / "mirror")], capture_output=True, text=True,
                                                            check=True).stdout.splitlines()):
        out[tag][w[0] if tag != "F" else (w[0], w[1])] = int(w[1]) if tag != "F" else (int(w[2]), int(w[3]), w[4])
    return out


def test_signatures_equal_the_headers_declarations():
    product, experiments = declarations(), declarations("semidetr_hip_experiments.h")
    assert len(product) >= 59 and len(experiments) == 3
    assert signature_mismatches(_lib.SIGNATURES, product) == []
    assert signature_mismatches(_lib.EXPERIMENT_SIGNATURES, experiments) == []


def test_structures_equal_the_headers_layout(report):
    assert list(_lib.STRUCTS) == re.findall(r"typedef struct (\w+) \{", _source("semidetr_hip.h"))
    for name, cls in _lib.STRUCTS.items():
        assert struct_mismatches(name, cls, report) == []


def test_constants_equal_the_headers_macros(report):
    assert report["C"] == _lib.CONSTANTS and len(_lib.CONSTANTS) == 15


def test_the_comparison_reports_a_wrong_mirror(report):
    fields = list(_lib.SelfAttn._fields_)
    i, j = fields.index(("scale", ctypes.c_float)), fields.index(("q", ctypes.c_void_p))
    fields[i], fields[j] = fields[j], fields[i]
    fields[0] = ("batch", ctypes.c_float)
    wrong = type("Wrong", (ctypes.Structure,), {"_fields_": fields})
    found = "\n".join(struct_mismatches("semidetr_self_attn", wrong, report))
    assert "semidetr_self_attn: fields" in found          # q keeps its offset (alignment padding): only the order shows it
    assert "semidetr_self_attn.scale: (offset, size, kind) (20, 4, 'floating') in the header, (32, 4, 'floating')" in found
    assert "semidetr_self_attn.batch: (offset, size, kind) (0, 4, 'integer') in the header, (0, 4, 'floating')" in found
    res, args = _lib.SIGNATURES["semidetr_qsel_gather_f32"]
    found = signature_mismatches({"semidetr_qsel_gather_f32": (res, args[:-1])},
                                 {"semidetr_qsel_gather_f32": declarations()["semidetr_qsel_gather_f32"]})
    assert "semidetr_qsel_gather_f32: 13 arguments in the header, 12 in the table" in found


def test_a_typed_block_pointer_refuses_other_blocks_before_anything_launches():
    fn = _lib.lib().semidetr_add_norm_forward_f32
    for wrong in (ctypes.byref(_lib.SelfAttn()), ctypes.c_void_p(4096), 4096, (_lib.SelfAttn * 1)()):
        with pytest.raises(ctypes.ArgumentError):
            fn(None, wrong, None, 0)
    assert fn(None, None, None, 0) == -1 and b"null pointer" in _lib.lib().semidetr_last_error()
    for empty in (ctypes.byref(_lib.AddNorm()), (_lib.AddNorm * 1)()):       # accepted by ctypes, refused by the library
        assert fn(None, empty, None, 0) == -1
