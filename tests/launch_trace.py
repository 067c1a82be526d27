"""Recording the library calls of a block as data: the core shared by tests/decode_trace.py and tests/train_trace.py.

trace() wraps the `call` name bound in every loaded egoscaler_amd module and records each launch as [symbol, argument, ...]: scalars by
value, device pointers as [buffer name, byte offset], NULL as None, a descriptor passed by reference as the list of its fields, a host
out-parameter as "out".  The buffer names come from the caller: Recorder.resolved() takes [(name, tensor)] in resolution order (a pointer
takes the first name whose tensor it lies in), so no raw address ever reaches a file.

trace(keep=True) also names what no object holds after the block.  Every device allocation torch makes inside the block is kept alive
until the trace is resolved, so no two of them share an address; a pointer into none of the named tensors is then written
["tmp[k]", byte offset from the start of the allocation], k counting those allocations in the order in which the trace first points into
them.  The numbering follows the launches alone, not the allocator's addresses and not the order of the allocations.  Without keep=True a
pointer into no named buffer is an error."""
import bisect
import contextlib
import ctypes
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves


def _extent(t):
    """Bytes from t.data_ptr() to the end of t's last element (views included)."""
    return (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0


def _raw(a):
    """A ctypes argument -> a scalar, ("p", address or None), ("s", [fields]) for a structure passed by reference, "out" for byref(scalar)."""
    if a is None or isinstance(a, ctypes.c_void_p):     # a bare None is passed as NULL
        return ("p", getattr(a, "value", None))
    obj = getattr(a, "_obj", None)
    if isinstance(obj, ctypes.Structure):
        return ("s", [("p", getattr(obj, f)) if ty is ctypes.c_void_p else getattr(obj, f) for f, ty in obj._fields_])
    return "out" if obj is not None else a.value


class _KeepAllocations(TorchDispatchMode):
    """Holds the storage of every device tensor an operator returns: nothing allocated under it is freed, so no address is used twice."""

    def __init__(self):
        super().__init__()
        self.storages = {}                               # base address -> storage, in order of allocation

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in tree_leaves(out):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                s = t.untyped_storage()
                if s.nbytes():
                    self.storages.setdefault(s.data_ptr(), s)
        return out


class Recorder:
    def __init__(self, inner, only, kept=None):
        self.inner, self.only, self.raw, self.kept = inner, only, [], kept

    def __call__(self, name, *args):
        if self.only is None or name.startswith(self.only):
            from egoscaler_amd import _lib
            self.raw.append([name] + [_raw(a) for a in _lib.marshal(name, args)])        # the ctypes values the library receives
        return self.inner(name, *args)

    def resolved(self, named):
        """The recorded launches with every pointer named through `named`, [(name, tensor)] in resolution order."""
        by_storage, tmp = {}, {}
        for n, t in named:
            s = t.untyped_storage()
            by_storage.setdefault((s.data_ptr(), s.nbytes()), []).append((n, t.data_ptr(), _extent(t)))
        bases = sorted(by_storage)
        kept = sorted((p, s.nbytes()) for p, s in self.kept.items()) if self.kept is not None else []

        def res(sym, i, v):
            if not isinstance(v, tuple):
                return v
            if v[0] == "s":
                return [res(sym, i, f) for f in v[1]]
            if v[1] is None:
                return None
            j = bisect.bisect_right(bases, (v[1], float("inf"))) - 1
            if j >= 0 and v[1] < bases[j][0] + bases[j][1]:
                for n, p0, nbytes in by_storage[bases[j]]:
                    if p0 <= v[1] < p0 + nbytes:
                        return [n, v[1] - p0]
            j = bisect.bisect_right(kept, (v[1], float("inf"))) - 1
            if j >= 0 and v[1] < kept[j][0] + kept[j][1]:
                return [tmp.setdefault(kept[j][0], f"tmp[{len(tmp)}]"), v[1] - kept[j][0]]
            raise AssertionError(f"{sym}: argument {i} points into no named buffer")
        return [[r[0]] + [res(r[0], i, v) for i, v in enumerate(r[1:])] for r in self.raw]


@contextlib.contextmanager
def trace(only=None, keep=False):
    """Records the library calls of the block; -> the Recorder (resolve with .resolved(named) before the buffers it saw can go away).
    only: a symbol prefix to record, None = every call.  keep: see the module docstring."""
    from egoscaler_amd import _lib
    orig = _lib.call                                    # (_lib is one of the modules patched below: keep the function, not the attribute)
    mode = _KeepAllocations() if keep else contextlib.nullcontext()
    rec = Recorder(orig, only, mode.storages if keep else None)
    mods = [m for n, m in list(sys.modules.items()) if (n == "egoscaler_amd" or n.startswith("egoscaler_amd.")) and getattr(m, "call", None) is orig]
    for m in mods:
        m.call = rec
    try:
        with mode:
            yield rec
    finally:
        for m in mods:
            m.call = orig


def first_difference(got, want):
    """None when equal, else a message naming the first differing launch."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"launch {i}: got {g}, recorded {w}"
    if len(got) != len(want):
        return f"{len(got)} launches, recorded {len(want)}"
    return None
