"""Reader of include/glowtts_hip.h: the header the library is compiled against is the ONLY description of the C ABI.

`_hip.py` types its ctypes handle from what this module yields, and csrc/gen_fastcall.py generates the FASTCALL wrappers from
the same thing, so neither keeps a copy of a prototype or a struct.  Standard library only (the build runs it before torch
is needed).  The header is plain C in a small vocabulary; whatever falls outside it RAISES with the function's or the struct's
name — a guessed type would hand a kernel shifted arguments:
    anything with `*`, glowtts_stream_t                      -> pointer (c_void_p);  `const char *` -> c_char_p
    int                                                       -> c_int
    float                                                     -> c_float
    long, long long, unsigned long long, int64_t              -> c_int64
    int32_t (struct fields the library writes)                -> c_int32
"""
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                           "include", "glowtts_hip.h")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long": ctypes.c_int64, "long long": ctypes.c_int64,
            "unsigned long long": ctypes.c_int64, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
            "glowtts_stream_t": ctypes.c_void_p}


class HipLibraryMissing(RuntimeError):
    pass


def _ctype(c_type: str, where: str):
    """ctypes code of a C type written without a declarator name ("const float *", "unsigned long long")."""
    words = " ".join(w for w in c_type.replace("*", " * ").split() if w != "const")
    if words == "char *":
        return ctypes.c_char_p
    if "*" in words:
        return ctypes.c_void_p
    if words not in _SCALARS:
        raise ValueError(f"{where}: type {c_type.strip()!r} is outside the vocabulary of the C ABI (glow_tts_train/_cabi.py)")
    return _SCALARS[words]


def _declarator(decl: str, where: str):
    """("const float *", "x") of `const float *x`."""
    m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", decl, flags=re.S)
    if not m:
        raise ValueError(f"{where}: cannot read the declaration {decl.strip()!r}")
    return m.group(1), m.group(2)


def _struct(name: str, body: str):
    fields = []
    for line in filter(str.strip, body.split(";")):
        first, *more = line.split(",")                    # `const float *wf_in, *wb_in, *b_in`
        where = f"struct {name}"
        c_type, field = _declarator(first, where)
        base = c_type.replace("*", " ")
        fields.append((field, _ctype(c_type, f"{where}.{field}")))
        for d in more:
            c_type, field = _declarator(base + d, where)
            fields.append((field, _ctype(c_type, f"{where}.{field}")))
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"struct {name} (include/glowtts_hip.h)"})


def parse(text: str):
    """(functions, structs, constants) of a header's text:
    functions[name] = (restype, [argtypes], streamed) — streamed: returns int and its last parameter is a glowtts_stream_t;
    structs[name]   = the ctypes.Structure of `typedef struct name { .. } name;`, fields in the header's order;
    constants[name] = value of `#define GLOWTTS_NAME integer`."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text).replace("\\\n", " ")
    constants = {m.group(1): int(m.group(2), 0)
                 for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GLOWTTS_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", "", text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)

    structs = {}

    def take_struct(m):
        if m.group(1) != m.group(3):
            raise ValueError(f"struct {m.group(1)}: typedef'd to another name, {m.group(3)}")
        structs[m.group(1)] = _struct(m.group(1), m.group(2))
        return ""

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)
    text = re.sub(r"\btypedef\b[^;{}]*;", "", text)      # typedef void *glowtts_stream_t

    functions = {}
    for stmt in filter(None, map(str.strip, text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise ValueError(f"cannot read the declaration {' '.join(stmt.split())[:80]!r}")
        name = m.group(2)
        restype = _ctype(m.group(1), f"{name}: return")
        params = [] if m.group(3).strip() in ("", "void") else [_declarator(p, name) for p in m.group(3).split(",")]
        args = [_ctype(c_type, f"{name}({arg})") for c_type, arg in params]
        streamed = restype is ctypes.c_int and bool(params) and params[-1][0].strip() == "glowtts_stream_t"
        functions[name] = (restype, args, streamed)
    return functions, structs, constants


def read_header(path: str = HEADER_PATH):
    if not os.path.exists(path):
        raise HipLibraryMissing(f"{path} not found: the C ABI of libglowtts_hip.so is read from this header")
    with open(path) as f:
        return parse(f.read())
