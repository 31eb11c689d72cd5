"""ctypes binding of libtensoir_hip.so, derived at import from include/tensoir_hip.h (the one statement of the C ABI).

There is NO fallback: if the shared library is missing or cannot be loaded the import of any
product entry point raises.  Built in-tree by ``tensoir_amd/csrc/build.sh`` (``__graft_entry__.build``).
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TENSOIR_HIP_LIB", os.path.join(_HERE, "libtensoir_hip.so"))
HEADER_PATH = os.environ.get("TENSOIR_HIP_HEADER", os.path.join(os.path.dirname(_HERE), "include", "tensoir_hip.h"))


class TensoirHipError(RuntimeError):
    pass


# ---- the header parser: exactly the C subset include/tensoir_hip.h uses (its top comment lists it); anything else raises ----
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double}
_POINTEES = {"void", "char", "unsigned", "unsigned long long", "uint8_t", "uint16_t", "uint32_t", *_SCALARS}   # + the structs
_INT, _FLT = r"-?(?:0[xX][0-9a-fA-F]+|[1-9]\d*|0)", r"-?(?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?"
_DEFINE = re.compile(rf"^#\s*define\s+(TIR_\w+)\s+(?:({_INT})|({_FLT})|\(\s*({_FLT})\s*/\s*({_FLT})\s*\))\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)")
_DECL = re.compile(r"\s*(?:const\s+)?(unsigned\s+long\s+long\b|[A-Za-z_]\w*)\s*(.*)", re.S)            # base type, declarators
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\s*)?)*)([A-Za-z_]\w*)\s*(?:\[\s*(\w+)\s*\])?\s*")   # stars, name, [length]


def _declarators(text, structs, const):
    """`const float* a[3], b` -> [("a", "float", 1, 3), ("b", "float", 0, None)]: name, base type, pointer depth, array length."""
    m = _DECL.fullmatch(text)
    base = " ".join(m.group(1).split()) if m else ""
    if base not in _POINTEES and base not in structs:
        raise TensoirHipError(f"{HEADER_PATH}: unknown type in `{text.strip()}`")
    out = []
    for d in m.group(2).split(","):
        m = _DECLARATOR.fullmatch(d)
        if not m:
            raise TensoirHipError(f"{HEADER_PATH}: cannot read the declarator `{d.strip()}` of `{text.strip()}`")
        length = m.group(3)
        if length is not None:
            length = int(length) if length.isdigit() else const.get(length)
            if not isinstance(length, int):
                raise TensoirHipError(f"{HEADER_PATH}: array length of `{text.strip()}` is neither a number nor an integer macro")
        out.append((m.group(2), base, m.group(1).count("*"), length))
    return out


def _value_type(base, text, structs):
    if base in _SCALARS:
        return _SCALARS[base]
    if base in structs:
        return structs[base]
    raise TensoirHipError(f"{HEADER_PATH}: `{base}` cannot be passed or stored by value in `{text.strip()}`")


def parse_header(src):
    """-> (CONST, STRUCTS, SIGNATURES) of a header text.  Raises TensoirHipError on anything outside the subset; never guesses."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S).replace("\\\n", " ")
    src = re.sub(r"^#\s*ifdef __cplusplus\n.*?^#\s*endif[^\n]*$", "", src, flags=re.S | re.M)      # we read the header as C
    const, code = {}, []
    for line in src.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        line = line.strip()
        if not re.match(r"#\s*(define|include|ifndef \w+_H|endif)\b", line):
            raise TensoirHipError(f"{HEADER_PATH}: preprocessor line `{line}` is outside the subset the binding reads")
        m = _DEFINE.match(line)
        if m:                                            # macros of any other shape (brace lists, the include guard) are skipped
            name, i, f, num, den = m.groups()
            const[name] = int(i, 0) if i else float(f) if f else float(num) / float(den)
    code = "\n".join(code)
    structs = {}
    for m in _STRUCT.finditer(code):
        if m.group(1) != m.group(3):
            raise TensoirHipError(f"{HEADER_PATH}: struct {m.group(1)} is typedef'd as {m.group(3)}")
        fields = []
        for decl in filter(str.strip, m.group(2).split(";")):
            for name, base, stars, length in _declarators(decl, structs, const):
                t = C.c_void_p if stars else _value_type(base, decl, structs)
                fields.append((name, t if length is None else t * length))
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
    sigs = {}
    for stmt in filter(str.strip, _STRUCT.sub("", code).split(";")):
        m = _PROTO.fullmatch(stmt.strip())
        if not m:
            raise TensoirHipError(f"{HEADER_PATH}: cannot read `{' '.join(stmt.split())}` as a prototype")
        ret, name, params = m.groups()
        types = []
        for text in [ret + name] + ([] if params.strip() in ("", "void") else params.split(",")):
            (_, base, stars, length), = _declarators(text, structs, const)
            if length is not None:
                raise TensoirHipError(f"{HEADER_PATH}: array parameter `{text.strip()}` of {name}")
            if stars == 1 and base in structs:
                types.append(C.POINTER(structs[base]))   # a TirMlp cannot be passed where a TirField belongs
            elif stars:
                types.append(C.c_char_p if base == "char" and not types else C.c_void_p)
            elif base == "void" and not types:
                types.append(None)
            else:
                types.append(_value_type(base, text, structs))
        sigs[name] = (types[0], types[1:])
    return const, structs, sigs


if not os.path.exists(HEADER_PATH):
    raise TensoirHipError(f"{HEADER_PATH} not found: the ctypes binding is derived from the C header (TENSOIR_HIP_HEADER overrides "
                          "the path)")
with open(HEADER_PATH) as _f:
    CONST, STRUCTS, SIGNATURES = parse_header(_f.read())     # name -> int | float, name -> Structure, name -> (restype, argtypes)
TirField, TirFieldHalf, TirFieldGrad, TirMlp, TirEnvSG = (STRUCTS[n] for n in ("TirField", "TirFieldHalf", "TirFieldGrad", "TirMlp",
                                                                               "TirEnvSG"))

_lib = None


def lib():
    """Load (once) and return the shared library.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TensoirHipError(
            f"{LIB_PATH} not found: the HIP library is not built.  Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or tensoir_amd/csrc/build.sh). "
            "tensoir_amd has no CPU / eager fallback by design.")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().tir_error_string(int(rc))
        raise TensoirHipError(f"{what or 'libtensoir_hip'} failed: rc={rc} ({msg.decode() if msg else '?'})")
