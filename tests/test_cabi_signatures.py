"""CPU: the signature table that egoscaler_amd/_abi.py reads from include/egomi.h.

- every declared symbol is bound (argtypes of the header's length on the built library);
- the table agrees with the C++ compiler: one generated translation unit of static_asserts on the header itself (structure sizes and
  field offsets, every prototype's arity, and per parameter / return its size and whether it is a pointer, a floating-point or a signed /
  unsigned integral type), compiled host-only with -fsyntax-only; the same unit generated from a structure that lost a field must fail;
- marshal()'s rules, on host-only entry points;
- an AST sweep: every call site in the package, the tools and bench.py passes the header's number of arguments, and inside the package
  none repeats a C type by hand.
No compute calls (no GPU here)."""
import ast
import ctypes
import os
import subprocess
from ctypes import byref, c_float, c_int, c_int64

import numpy as np
import pytest
import torch

from egoscaler_amd import _abi, _lib, build as B, ops
from tests.test_cabi_symbols import ROOT, declared_symbols

SLABS = "egomi_gemm_w8_slab_count"          # (int M, int N, int K, int64_t workspace_bytes), host-only


@pytest.fixture(scope="module")
def L():
    B.build()
    return _lib.lib()


def test_every_declared_symbol_is_bound(L):
    assert sorted(_abi.PROTOS) == declared_symbols() and len(_abi.PROTOS) >= 97
    for name, (ret, params) in _abi.PROTOS.items():
        fn = getattr(L, name)
        assert fn.restype is ret and list(fn.argtypes) == [t for _, t in params], name
    assert ops.GemmDesc is _abi.STRUCTS["egomi_gemm_desc"] and ops.AttnDesc is _abi.STRUCTS["egomi_attn_desc"]
    assert (ops.F32, ops.BF16, _abi.EGOMI_E_LAUNCH, _abi.EGOMI_EPI_SLABS) == (0, 1, -3, 2)


# -- the table against the compiler ----------------------------------------------------------------------------------------------
def _kind(ct):
    """'p' pointer, 'f' floating point, 'i' / 'u' signed / unsigned integral: what the ctypes type chosen for a parameter claims."""
    if ct in (ctypes.c_float, ctypes.c_double):
        return "f"
    if ct in (ctypes.c_void_p, ctypes.c_char_p) or not isinstance(ct._type_, str):
        return "p"
    return "i" if ct(-1).value < 0 else "u"


PRELUDE = """#include <cstddef>
#include <tuple>
#include <type_traits>
#include "egomi.h"
template <class F> struct sig;
template <class R, class... A> struct sig<R(A...)> {
    using ret = R;
    static constexpr int arity = sizeof...(A);
    template <int I> using arg = std::tuple_element_t<I, std::tuple<A...>>;
};
template <class T> constexpr char kind = std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f'
                                         : std::is_integral_v<T> ? (std::is_signed_v<T> ? 'i' : 'u') : '?';
#define IS(T, size, k, what) static_assert(sizeof(T) == size && kind<T> == k, what)
"""


def translation_unit(structs, protos):
    out = [PRELUDE]
    for cname, cls in structs.items():
        out.append(f'static_assert(sizeof({cname}) == {ctypes.sizeof(cls)}, "sizeof {cname}");')
        for f, ct in cls._fields_:
            out.append(f'static_assert(offsetof({cname}, {f}) == {getattr(cls, f).offset}, "offsetof {cname}.{f}");')
            out.append(f'IS(decltype({cname}::{f}), {ctypes.sizeof(ct)}, \'{_kind(ct)}\', "{cname}.{f}");')
    for name, (ret, params) in protos.items():
        s = f"sig<decltype({name})>"
        out.append(f'static_assert({s}::arity == {len(params)}, "{name}: arity");')
        out.append(f'IS({s}::ret, {ctypes.sizeof(ret)}, \'{_kind(ret)}\', "{name}: return");')
        for i, (p, ct) in enumerate(params):
            out.append(f'IS({s}::arg<{i}>, {ctypes.sizeof(ct)}, \'{_kind(ct)}\', "{name}: {p}");')
    return "\n".join(out) + "\n"


def _syntax_check(text, tmp_path):
    src = tmp_path / "abi_check.cpp"
    src.write_text(text)
    return subprocess.run([B._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True, text=True)


def test_table_agrees_with_the_compiler(tmp_path):
    text = translation_unit(_abi.STRUCTS, _abi.PROTOS)
    assert text.count("static_assert(") + text.count("IS(") > 1100          # 97 prototypes, ~970 parameters, 59 fields
    r = _syntax_check(text, tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("cname,field", [("egomi_gemm_desc", "split_k"), ("egomi_attn_desc", "q_rows")])
def test_compiler_check_catches_a_dropped_field(tmp_path, cname, field):
    """A field missing from the generated structure (a middle one; the last one) moves an offset or the size: the unit must not compile."""
    cls = _abi.STRUCTS[cname]
    short = type("Short", (ctypes.Structure,), {"_fields_": [f for f in cls._fields_ if f[0] != field]})
    r = _syntax_check(translation_unit({cname: short}, {}), tmp_path)
    assert r.returncode != 0 and "static assertion failed" in r.stderr and cname in r.stderr


def test_parser_names_what_it_cannot_read():
    head = '#define EGOMI_OK 0\nextern "C" {\ntypedef void* egomi_stream_t;\n'
    for body, needle in (("int egomi_f(unsigned n);", "unsigned"), ("int egomi_f(int (*cb)(int));", "egomi_f"),
                         ("long egomi_f(int n);", "long"), ("int egomi_f(int);", "egomi_f"), ("int egomi_f(int n)\n int egomi_g(void);", "egomi_f"),
                         ("typedef struct egomi_gemm_desc { short M; } egomi_gemm_desc;", "egomi_gemm_desc.M"), ("#define EGOMI_X 0x10", "EGOMI_X")):
        with pytest.raises(_lib.EgomiError, match=needle):
            _abi.parse(head + body + "\n}\n")
    consts, structs, protos = _abi.parse(head + "#define EGOMI_E_X (-7)\nsize_t egomi_f(const float* x, int64_t n,\n  egomi_stream_t s);\n}\n")
    assert consts == {"EGOMI_OK": 0, "EGOMI_E_X": -7} and not structs
    assert protos == {"egomi_f": (ctypes.c_size_t, [("x", ctypes.c_void_p), ("n", c_int64), ("s", ctypes.c_void_p)])}


# -- marshalling rules -----------------------------------------------------------------------------------------------------------
def test_marshal_argument_count():
    with pytest.raises(TypeError, match=f"{SLABS} takes 4 arguments, 3 given"):
        _lib.marshal(SLABS, (1, 2, 3))
    with pytest.raises(TypeError, match=f"{SLABS} takes 4 arguments, 5 given"):        # ctypes alone lets surplus arguments through
        _lib.marshal(SLABS, (1, 2, 3, 4, 5))


def test_marshal_integers():
    m = _lib.marshal(SLABS, (True, np.int32(7), 2**31 - 1, 2**40))
    assert [type(a) for a in m] == [c_int, c_int, c_int, c_int64] and [a.value for a in m] == [1, 7, 2**31 - 1, 2**40]
    with pytest.raises(OverflowError, match=r"argument 1 \(N\)"):
        _lib.marshal(SLABS, (1, 2**31, 3, 4))
    with pytest.raises(OverflowError):
        _lib.marshal(SLABS, (1, 2, -2**31 - 1, 4))
    with pytest.raises(OverflowError):
        _lib.marshal(SLABS, (1, 2, 3, 2**63))
    for bad in (1.0, None, torch.tensor(3), "3", c_float(3)):
        with pytest.raises(TypeError, match=r"argument 0 \(M\)"):
            _lib.marshal(SLABS, (bad, 2, 3, 4))
    with pytest.raises(TypeError, match=r"argument 3 \(workspace_bytes\)"):             # a c_int object where the header says int64_t
        _lib.marshal(SLABS, (1, 2, 3, c_int(4)))


def test_marshal_passes_typed_ctypes_objects_through(L):
    a, w = c_int(4), c_int64(1 << 24)
    m = _lib.marshal(SLABS, (a, 4096, 4096, w))
    assert m[0] is a and m[3] is w
    n = _lib.query(SLABS, 4, 4096, 4096, 1 << 24)
    assert n >= 1 and n == _lib.query(SLABS, a, c_int(4096), c_int(4096), w) == L.egomi_gemm_w8_slab_count(a, 4096, 4096, w)


def test_marshal_reals():
    m = _lib.marshal("egomi_seq_rank", (None, None, 1, 1, 1e-5, None, None, None))
    assert type(m[4]) is c_float and m[4].value == c_float(1e-5).value != 1e-5         # the rounded value, as the decode trace records it
    assert _lib.marshal("egomi_seq_rank", (None, None, 1, 1, np.float32(2), None, None, None))[4].value == 2.0
    d = _lib.marshal("egomi_depth_to_cloud", (None, 1, 2, 2, None, 2, 2, 0.1, 1, 0.3, None, None, None, None, None))
    assert [type(a) for a in d[7:10]] == [ctypes.c_double] * 3 and d[7].value == 0.1 and d[8].value == 1.0
    for bad in (None, "1", torch.tensor(1.0), c_int(1), ctypes.c_double(1)):
        with pytest.raises(TypeError, match=r"argument 4 \(length_penalty\)"):
            _lib.marshal("egomi_seq_rank", (None, None, 1, 1, bad, None, None, None))


def test_marshal_pointers():
    n, p, arr = c_int(0), ctypes.c_void_p(256), (c_int * 4)()
    ok = (None, p, byref(n), arr)
    for v in ok:
        assert _lib.marshal("egomi_gemm_last_route", (v,))[0] is v
    for bad in (256, 0, 1.0, n, byref(ops.GemmDesc())):                                 # a bare int: a count where a buffer belongs
        with pytest.raises(TypeError, match=r"argument 0 \(out4\)"):
            _lib.marshal("egomi_gemm_last_route", (bad,))
    with pytest.raises(_lib.EgomiError, match="no CPU fallback"):
        _lib.marshal("egomi_pc_norm", (torch.zeros(1, 4, 3, dtype=torch.float64), None, None, 1, 4, None))
    with pytest.raises(TypeError, match=r"argument 3 \(B\)"):                            # tensor and count transposed
        _lib.marshal("egomi_pc_norm", (None, None, None, torch.zeros(1), 4, None))


def test_marshal_descriptors(L):
    d = ops.GemmDesc()
    ref = byref(d)
    assert _lib.marshal("egomi_gemm_kernel_id", (ref,))[0] is ref and _lib.marshal("egomi_gemm_kernel_id", (None,)) == (None,)
    for bad in (byref(ops.AttnDesc()), d, 5, ctypes.c_void_p(256), torch.zeros(4)):
        with pytest.raises(TypeError, match=r"argument 0 \(desc\)"):
            _lib.marshal("egomi_gemm_kernel_id", (bad,))
    assert ops.gemm_kernel_id(5536, 4096, 4096) == 2 and _lib.query("egomi_gemm_kernel_id", None) < 0   # NULL: the library's own BADARG


def test_call_checks_before_the_library_is_entered(L):
    with pytest.raises(_lib.EgomiError, match="not declared"):
        _lib.call("egomi_gemm_stamp_reset")
    for args, exc in (((2**31,), OverflowError), ((4.0,), TypeError), ((torch.tensor(4),), TypeError), ((), TypeError), ((4, 4), TypeError)):
        with pytest.raises(exc, match="egomi_attn_set_fwd_form"):
            _lib.call("egomi_attn_set_fwd_form", *args)
    _lib.call("egomi_attn_set_fwd_form", 4)                                            # the default form (process-wide switch)
    with pytest.raises(_lib.EgomiError, match="egomi_attn_set_fwd_form: egomi error"):
        _lib.call("egomi_attn_set_fwd_form", 99)


# -- the call sites --------------------------------------------------------------------------------------------------------------
WRAPPERS = {"c_i", "c_i64", "c_f", "c_d", "c_sz", "P"}


def _py_files():
    yield os.path.join(ROOT, "bench.py")
    for top in ("egoscaler_amd", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            yield from (os.path.join(d, f) for f in files if f.endswith(".py"))


def _symbols(node):
    """The entry points a call site may name: call("egomi_x", ...), call("a" if c else "b", ...), lib().egomi_x(...) -> names, first argument index."""
    f = node.func
    if isinstance(f, ast.Attribute) and f.attr.startswith("egomi_"):
        return [f.attr], 0
    if (isinstance(f, ast.Name) and f.id in ("call", "query") or isinstance(f, ast.Attribute) and f.attr in ("call", "query")) and node.args:
        a = node.args[0]
        consts = [a] if isinstance(a, ast.Constant) else [a.body, a.orelse] if isinstance(a, ast.IfExp) else []
        return [c.value for c in consts if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("egomi_")], 1
    return [], 0


def _wrapped(node):
    """Wrapper constructions inside an argument, byref(...) out-parameters exempt."""
    if isinstance(node, ast.Call):
        if isinstance(node.func, ast.Attribute) and node.func.attr == "byref" or isinstance(node.func, ast.Name) and node.func.id == "byref":
            return []
        if isinstance(node.func, ast.Name) and node.func.id in WRAPPERS:
            return [node.func.id]
    return [w for ch in ast.iter_child_nodes(node) for w in _wrapped(ch)]


def test_call_sites_match_the_header():
    sites, bad = 0, []
    for path in _py_files():
        rel = os.path.relpath(path, ROOT)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.Call):
                continue
            names, first = _symbols(node)
            args = node.args[first:]
            for name in names:
                if name not in _abi.PROTOS:
                    if "_stamp_" not in name:
                        bad.append(f"{rel}:{node.lineno}: {name} is not declared")
                    continue
                sites += 1
                if any(isinstance(a, ast.Starred) for a in args) or node.keywords:
                    bad.append(f"{rel}:{node.lineno}: {name}: star or keyword arguments")
                elif len(args) != len(_abi.PROTOS[name][1]):
                    bad.append(f"{rel}:{node.lineno}: {name} takes {len(_abi.PROTOS[name][1])} arguments, {len(args)} given")
                if rel.startswith("egoscaler_amd") and any(_wrapped(a) for a in args):
                    bad.append(f"{rel}:{node.lineno}: {name}: a C type repeated by hand ({sorted({w for a in args for w in _wrapped(a)})})")
    assert not bad, "\n".join(bad)
    assert sites >= 90                                                                  # the sweep sees the package's call sites at all


def test_package_sets_no_types_by_hand():
    for f in ("ops.py", "decode.py", "traj.py", "pointbert_train.py", "_lib.py"):
        src = open(os.path.join(ROOT, "egoscaler_amd", f)).read()
        assert ".restype" not in src and ".argtypes" not in src and "ctypes.Structure" not in src, f
