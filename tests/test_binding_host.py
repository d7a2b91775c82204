"""The binding is read from include/pmf_amd.h (pmf_amd/_lib.py read_header / bind): the reader on small header texts, its
refusals, and the real header against counts this file takes itself.  Host only."""
import ctypes as C
import os
import re

import pytest

from pmf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = """
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* t_stream_t; /* a handle; not t_f(x); */
#define T_MAX 5
#define T_TAPS (T_MAX + 2)       /* comment with ; and ( */
#define T_BIT (1 << 24)
#define T_NEG (-1)
#define T_NAME "text"
enum { T_A = 3, T_B, T_C = T_B + 10, T_D };
enum { T_ZERO, T_ONE };
typedef struct {
  const float* x;   // t_g(a; b)
  int32_t H, W;     /* multi-declarator; and t_h( */
  int8_t tdy[T_TAPS + 3], tdx[T_TAPS + 3];
  double s;
} t_in_t;
typedef struct {
  int32_t kind;
  t_in_t src[T_MAX];
  void* p[2];
  union {
    t_in_t one;
    int64_t l[3];
  } u;
} t_op_t;
int t_run(const t_op_t* ops, int32_t n, t_stream_t s,
          int64_t count,
          float a, double b,
          int32_t info[12]);
int64_t t_bytes(const t_in_t* d);
const char* t_version(void);
void t_reset(unsigned long long* cnt, const int64_t* const* lists);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_constants():
    c = L.read_header(SMALL).consts
    assert c == {"T_MAX": 5, "T_TAPS": 7, "T_BIT": 1 << 24, "T_NEG": -1, "T_A": 3, "T_B": 4, "T_C": 14, "T_D": 15,
                 "T_ZERO": 0, "T_ONE": 1}


def test_reader_structs():
    s = L.read_header(SMALL, {"t_in_t": "In"}).structs
    In, Op = s["t_in_t"], s["t_op_t"]
    assert In.__name__ == "In" and Op.__name__ == "t_op_t"
    assert [(n, getattr(In, n).offset, getattr(In, n).size) for n, _ in In._fields_] == \
        [("x", 0, 8), ("H", 8, 4), ("W", 12, 4), ("tdy", 16, 10), ("tdx", 26, 10), ("s", 40, 8)]
    assert C.sizeof(In) == 48
    f = dict(In._fields_)
    assert f["x"] is C.c_void_p and f["H"] is C.c_int32 and f["tdy"]._type_ is C.c_int8 and f["s"] is C.c_double
    assert [(n, getattr(Op, n).offset, getattr(Op, n).size) for n, _ in Op._fields_] == \
        [("kind", 0, 4), ("src", 8, 240), ("p", 248, 16), ("u", 264, 48)]
    o = dict(Op._fields_)
    assert o["src"]._type_ is In and o["src"]._length_ == 5 and o["p"]._type_ is C.c_void_p
    assert issubclass(o["u"], C.Union) and [n for n, _ in o["u"]._fields_] == ["one", "l"]
    assert Op.u.size == 48 and o["u"].l.offset == 0


def test_reader_prototypes():
    p = L.read_header(SMALL).protos
    assert list(p) == ["t_run", "t_bytes", "t_version", "t_reset"]         # the calls inside comments are no declarations
    v = C.c_void_p
    assert p["t_run"] == (C.c_int32, [v, C.c_int32, v, C.c_int64, C.c_float, C.c_double, v])
    assert p["t_bytes"] == (C.c_int64, [v])
    assert p["t_version"] == (C.c_char_p, [])
    assert p["t_reset"] == (None, [v, v])


def test_reader_keeps_descriptor_pointers_typed():
    h = L.read_header("typedef struct { int32_t ldc; } pmf_view_t;\n"
                      "int f(const pmf_view_t* a, pmf_view_t* out, const pmf_view_t* views_dev, const pmf_view_t* v[2]);")
    assert h.protos["f"][1] == [C.POINTER(h.structs["pmf_view_t"]), C.c_void_p, C.c_void_p, C.c_void_p]


@pytest.mark.parametrize("text, named", [
    ("int f(size_t n);", "int f(size_t n)"),                                          # unknown type
    ("typedef struct { int32_t a; } v_t;\nint f(v_t v, int n);", "int f(v_t v, int n)"),    # struct by value
    ("typedef struct { int32_t a : 3; } b_t;", "int32_t a : 3"),                    # bit-field
    ("int f(int (*cb)(int), int n);", "int f(int (*cb)(int), int n)"),                # function pointer parameter
    ("typedef struct { int (*cb)(int); } c_t;", "int (*cb)(int)"),                    # function pointer member
    ("int f(const char* fmt, ...);", "int f(const char* fmt, ...)"),                  # variadic
    ("typedef struct { wchar_t w[4]; } w_t;", "wchar_t w[4]"),                        # unknown member type
    ("typedef struct { int32_t a[N_UNKNOWN]; } n_t;", "int32_t a[N_UNKNOWN]"),        # array bound that is no constant
    ("#if X\nint f(int a);\n#endif", "#if X"),                                        # a section the reader cannot follow
])
def test_reader_refuses(text, named):
    with pytest.raises(L.PMFLibraryError) as e:
        L.read_header(text)
    assert named in str(e.value)


def test_missing_header_is_reported(monkeypatch):
    monkeypatch.setattr(L, "HEADER_PATH", os.path.join(ROOT, "include", "no_such.h"))
    with pytest.raises(L.PMFLibraryError) as e:
        L._read()
    assert "no_such.h not found" in str(e.value)


def test_every_prototype_of_the_header_is_bound():
    text = open(os.path.join(ROOT, "include", "pmf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = re.findall(r"\b(pmf_\w+)\s*\(([^()]*)\)\s*;", text)
    assert len(found) == len(L.EXPORTS) == 117 and [n for n, _ in found] == L.EXPORTS
    lib = L.lib()
    for name, params in found:
        nargs = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert getattr(lib, name).restype is not None


def test_struct_sizes():
    lib = L.lib()
    for which, st in enumerate((L.Src, L.ConvDesc, L.WgradDesc, L.View, L.SmallArgs, L.Op, L.PackJob)):
        assert lib.pmf_sizeof(which) == C.sizeof(st)
    assert C.sizeof(L.ConvDst) == 80
    # sizeof(pmf_bev_extent_t) printed by a host program built with the system C compiler (x86-64): four float, four int32_t
    assert C.sizeof(L.BevExtent) == 32
    assert [n for n, _ in L.BevExtent._fields_] == ["min_x", "min_y", "max_x", "max_y", "h", "w", "flags", "max_count"]


def test_formerly_unbound_entry_point_takes_a_64_bit_stream():
    """pmf_conv_wgrad_partial had no argtypes: an integer stream handle would have been converted as a C int.  Its
    descriptor check comes before any HIP call (wgrad_phases in conv_wgrad.hip), so this runs without a GPU."""
    lib = L.lib()
    assert lib.pmf_conv_wgrad_partial.argtypes[0] is C.POINTER(L.WgradDesc)
    assert lib.pmf_conv_wgrad_partial.argtypes[1] is C.c_void_p
    assert lib.pmf_conv_wgrad_partial(C.byref(L.WgradDesc()), 0x7F0012345678) == L.PMF_E_ARG         # nsrc = 0
    with pytest.raises(C.ArgumentError):
        lib.pmf_conv_wgrad_partial(C.byref(L.ConvDesc()), None)
