#!/usr/bin/env python3
"""Compare two versions of pmf_amd/_lib.py (e.g. `git show HEAD~1:pmf_amd/_lib.py > /tmp/old_lib.py`): public names and
values, struct layouts, and the argtypes / restype each gives a library handle.  Needs no library: a stand-in collects them.
usage: python tools/compare_binding.py OLD_LIB_PY [NEW_LIB_PY]     (exit status 1 on any difference)"""
import ctypes as C, importlib.util, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

class Handle:                                   # stands in for the CDLL: every attribute is a function to be typed
    def __getattr__(self, name):
        if name.startswith("__"): raise AttributeError(name)
        fn = types.SimpleNamespace(argtypes=None, restype=C.c_int)
        setattr(self, name, fn)
        return fn

def load(path, tag):
    spec = importlib.util.spec_from_file_location("pmf_lib_" + tag, path)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    h = Handle()
    if hasattr(m, "bind"): m.bind(h)
    else:                                       # a version that types the functions inside lib()
        h.pmf_sizeof = lambda which: C.sizeof((m.Src, m.ConvDesc, m.WgradDesc, m.View, m.SmallArgs, m.Op, m.PackJob)[which])
        exists, cdll = os.path.exists, C.CDLL
        m.os.path.exists, m.C.CDLL = (lambda p: True), (lambda p: h)
        m.lib()
        m.os.path.exists, m.C.CDLL = exists, cdll
    return m, {k: v for k, v in vars(h).items() if v.argtypes is not None or v.restype is not C.c_int}

def kind(t):
    if t is None: return "void"
    if isinstance(t, type) and issubclass(t, C._Pointer) and issubclass(t._type_, (C.Structure, C.Union)):
        return "ptr " + t._type_.__name__       # a typed descriptor pointer: compared by struct name
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C.Array))): return "ptr"
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_double: "f64"}[t]

def layout(st, prefix=""):
    out = []
    for name, t in st._fields_:
        f = getattr(st, name)
        out.append((prefix + name, f.offset, f.size))
        if isinstance(t, type) and issubclass(t, (C.Structure, C.Union)): out += layout(t, prefix + name + ".")
    return out

old, fo = load(sys.argv[1], "old")
new, fn = load(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "pmf_amd", "_lib.py"), "new")
bad, stricter = 0, []
for name, f in fo.items():
    g = fn.get(name)
    a, b = [kind(t) for t in f.argtypes or []], [kind(t) for t in g.argtypes or []] if g else None
    # per parameter the same class; where the old binding names the struct behind a pointer, the new one names the same
    args_ok = g is not None and (f.argtypes is None or (len(a) == len(b) and all(x == y or (x == "ptr" and y.startswith("ptr ")) for x, y in zip(a, b))))
    if not args_ok or kind(f.restype) != kind(g.restype) or (f.restype is C.c_char_p) != (g.restype is C.c_char_p):
        bad += 1; print("FUNCTION %s: old %s -> %s, new %s" % (name, a, kind(f.restype), g and (b, kind(g.restype))))
    elif f.argtypes is not None and a != b: stricter.append(name)
structs = [n for n, v in vars(old).items() if isinstance(v, type) and issubclass(v, C.Structure) and not n.startswith("_")]
for n in structs:
    if not hasattr(new, n) or layout(getattr(old, n)) != layout(getattr(new, n)) or C.sizeof(getattr(old, n)) != C.sizeof(getattr(new, n)):
        bad += 1; print("STRUCT %s differs" % n)
names = [n for n, v in vars(old).items() if not n.startswith("_") and not n.endswith("_PATH") and isinstance(v, (int, str, list, dict, tuple))]
for n in names:
    same = hasattr(new, n) and (sorted(getattr(new, n)) == sorted(getattr(old, n)) if n == "EXPORTS" else getattr(new, n) == getattr(old, n))
    if not same: bad += 1; print("NAME %s: old %r, new %r" % (n, getattr(old, n), getattr(new, n, None)))
print("%d functions typed by the old binding, %d by the new (new only: %s)" % (len(fo), len(fn), ", ".join(sorted(set(fn) - set(fo)))))
print("void pointer in the old, typed descriptor pointer in the new: %s" % (", ".join(stricter) or "none"))
print("%d structs with equal (member, offset, size) lists: %s" % (len(structs), ", ".join(structs)))
print("%d public names with equal values; %d differences" % (len(names), bad))
sys.exit(1 if bad else 0)
