"""The C ABI of libegomi.so, read from include/egomi.h: that header is its only statement.

Parsed once at import (no library, no GPU needed): every prototype, the two descriptor structures and the integer EGOMI_* constants.
From that table come the generated ctypes.Structure classes, `argtypes` / `restype` of every declared symbol (bind) and one converter
per parameter (marshal).  The header's top comment lists the rules this reader relies on; a line it cannot read is an error that names
the line, never a skipped declaration.
"""
import ctypes
import numbers
import os
import re
from ctypes import c_double, c_float, c_int, c_int64, c_size_t, c_void_p
from operator import index

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egomi.h")


class EgomiError(RuntimeError):
    pass


SCALARS = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "float": c_float, "double": c_double}
RETURNS = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "char *": ctypes.c_char_p}
POINTEES = {"void", "float", "double", "int", "int32_t", "int64_t", "uint8_t", "uint64_t", "void *"}   # every such pointer is a c_void_p
STRUCT_NAMES = {"egomi_gemm_desc": "GemmDesc", "egomi_attn_desc": "AttnDesc"}


def _spelling(t):
    return " ".join(re.sub(r"\bconst\b", " ", t).replace("*", " * ").split())


def _ctype(t, what, structs):
    s = _spelling(t)
    if s in SCALARS:
        return SCALARS[s]
    if s == "egomi_stream_t" or (s.endswith(" *") and s[:-2] in POINTEES):
        return c_void_p
    if s.endswith(" *") and s[:-2] in structs:
        return ctypes.POINTER(structs[s[:-2]])
    raise EgomiError(f"egomi.h: {what}: the binder does not know the type '{' '.join(t.split())}'")


def _declarator(d, what):
    m = re.fullmatch(r"(.*[\s*])(\w+)", d.strip(), flags=re.S)
    if not m:
        raise EgomiError(f"egomi.h: {what}: cannot read '{' '.join(d.split())}' as '<type> <name>'")
    return m.group(1), m.group(2)


def _fields(body, cname):
    out = []
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = decl.split(",")
        t, name = _declarator(first, cname)
        for n in [name] + [m.strip() for m in more]:
            if not re.fullmatch(r"\w+", n):
                raise EgomiError(f"egomi.h: {cname}: cannot read the field list '{' '.join(decl.split())}'")
            out.append((n, _ctype(t, f"{cname}.{n}", {})))
    return out


def parse(text):
    """-> (consts {name: int}, structs {C name: ctypes.Structure class}, protos {symbol: (restype, [(parameter, ctype)])})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(EGOMI_\w+)(.*)$", text, flags=re.M):
        if val.strip():                                               # (the include guard has no value)
            if not re.fullmatch(r"-?\d+|\(-?\d+\)", val.strip()):
                raise EgomiError(f"egomi.h: #define {name}: '{val.strip()}' is not an integer")
            consts[name] = int(val.strip().strip("()"))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "", 1)
    structs = {}

    def struct(m):
        cname = m.group(1)
        if m.group(3) != cname or cname not in STRUCT_NAMES:
            raise EgomiError(f"egomi.h: typedef struct {cname}: not one of the descriptors the binder generates")
        structs[cname] = type(STRUCT_NAMES[cname], (ctypes.Structure,), {"_fields_": _fields(m.group(2), cname)})
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    *stmts, tail = text.split(";")
    if tail.strip() != "}":                                           # the closing brace of extern "C"
        raise EgomiError(f"egomi.h: cannot read the end of the header: '{' '.join(tail.split())}'")
    protos = {}
    for stmt in stmts:
        stmt = " ".join(stmt.split())
        if stmt == "typedef void* egomi_stream_t":
            continue
        m = re.fullmatch(r"(.*[\s*])(egomi_\w+) ?\((.*)\)", stmt)
        if not m or "(" in m.group(3):
            raise EgomiError(f"egomi.h: cannot read '{stmt}' as a prototype")
        ret, name, plist = m.groups()
        if _spelling(ret) not in RETURNS:
            raise EgomiError(f"egomi.h: {name}: the binder does not know the return type '{ret.strip()}'")
        params = []
        for d in ([] if plist.strip() == "void" else plist.split(",")):
            t, pname = _declarator(d, name)
            params.append((pname, _ctype(t, f"{name}({pname})", structs)))
        protos[name] = (RETURNS[_spelling(ret)], params)
    return consts, structs, protos


with open(HEADER) as _f:
    CONSTS, STRUCTS, PROTOS = parse(_f.read())
globals().update(CONSTS)                                              # EGOMI_OK, EGOMI_E_*, EGOMI_F32, EGOMI_BF16, EGOMI_EPI_*, ... by name


def bind(lib):
    """argtypes and restype on every symbol the header declares; a declared symbol the library lacks is an error."""
    for name, (ret, params) in PROTOS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise EgomiError(f"{name} is declared in include/egomi.h but the library does not export it") from None
        fn.restype, fn.argtypes = ret, [t for _, t in params]


# -- marshalling: one converter per parameter ----------------------------------------------------------------------------------
def _int_conv(ct):
    bits = 8 * ctypes.sizeof(ct)
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if ct(-1).value < 0 else (0, (1 << bits) - 1)

    def conv(v):
        if type(v) is ct:
            return v
        if hasattr(v, "data_ptr"):                                    # a 0-d integer tensor has __index__ (and would wait for the device)
            raise TypeError(f"a tensor where {ct.__name__} belongs")
        i = v if type(v) is int else index(v)                         # TypeError for a float, None or a ctypes object of another type
        if not lo <= i <= hi:
            raise OverflowError(f"{i} does not fit {ct.__name__}")
        return ct(i)
    return conv


def _real_conv(ct):
    def conv(v):
        if type(v) is ct:
            return v
        if not isinstance(v, numbers.Real):
            raise TypeError(f"{type(v).__name__} where {ct.__name__} belongs")
        return ct(v)                                                  # .value is the value rounded to the C type
    return conv


def _pointer_conv(v):
    """Device pointers, host out-parameters and the stream.  A bare int is refused: a count where a buffer belongs is a transposition."""
    if v is None or type(v) is c_void_p:
        return v
    ptr = getattr(v, "data_ptr", None)
    if ptr is not None:
        if not v.is_cuda:
            raise EgomiError("egoscaler_amd ops need CUDA/HIP tensors (no CPU fallback)")
        return c_void_p(ptr())
    if isinstance(getattr(v, "_obj", v), (ctypes._SimpleCData, ctypes.Array)) and not isinstance(v, ctypes._SimpleCData):
        return v                                                      # byref(scalar) or a ctypes array: a host out-parameter
    raise TypeError(f"{type(v).__name__} where a pointer belongs (None, a device tensor, c_void_p or byref of a scalar)")


def _desc_conv(ptr_type):
    struct = ptr_type._type_

    def conv(v):
        if v is None or type(v) is ptr_type or isinstance(getattr(v, "_obj", None), struct):
            return v
        raise TypeError(f"{type(v).__name__} where byref({struct.__name__}) belongs")
    return conv


def _conv(ct):
    if ct in (c_float, c_double):
        return _real_conv(ct)
    if ct is c_void_p:
        return _pointer_conv
    return _desc_conv(ct) if hasattr(ct, "_type_") and not isinstance(ct._type_, str) else _int_conv(ct)


_CONV = {name: tuple(_conv(t) for _, t in params) for name, (_, params) in PROTOS.items()}


def marshal(name, args):
    """The tuple of ctypes values (None = NULL) that go to entry point `name` for `args`, checked against its prototype."""
    try:
        convs = _CONV[name]
    except KeyError:
        raise EgomiError(f"{name} is not declared in include/egomi.h") from None
    if len(args) != len(convs):
        raise TypeError(f"{name} takes {len(convs)} arguments, {len(args)} given")
    try:
        return tuple([c(a) for c, a in zip(convs, args)])
    except (TypeError, OverflowError, EgomiError) as e:
        for i, (c, a) in enumerate(zip(convs, args)):                 # slow path: name the parameter
            try:
                c(a)
            except type(e):
                raise type(e)(f"{name}: argument {i} ({PROTOS[name][1][i][0]}): {e}") from None
        raise
