"""ctypes binding of libpmf_amd.so, derived from include/pmf_amd.h at import.

The header is the only place a constant, a struct member or a signature is written: read_header() turns its text into the
PMF_* integers, the ctypes structs and the argtypes / restype of every prototype.  The reader is strict -- a declaration it
cannot classify raises PMFLibraryError naming it, it never skips or guesses.  include/pmf_amd_sensat.h (the SensatUrban
training loader) is a second header read the same way on top of the first: EXPORTS_SENSAT, BevSample.  include/pmf_amd_wide.h
(33 to 64 classes in the heads and the fused objective) is a third: EXPORTS_WIDE.  include/pmf_amd_a2d2.h (the A2D2 loader:
undistortion map, remap, per-point pass) is a fourth: EXPORTS_A2D2, LENS_TELECAM / LENS_FISHEYE.  include/pmf_amd_nus.h (the
nuScenes projection chain) is a fifth: EXPORTS_NUS, NUS_BLOCK, NUS_CHAIN, NUS_IMAGE / NUS_YAW.  include/pmf_amd_fov.h (the
SemanticKITTI-FOV filter) is a sixth: EXPORTS_FOV, FOV_BLOCK, FOV_MAX_FRAMES.  include/pmf_amd_full.h (full sweeps from FOV
predictions) is a seventh: EXPORTS_FULL, FULL_WS_PER_BLOCK, FULL_WS_FIXED.

The product path has NO fallback: if the header or the shared library is missing, or the library's struct layout
disagrees with the header, importing a compute entry point raises.
"""
import ctypes as C
import os
import re
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpmf_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd.h")
SENSAT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_sensat.h")
WIDE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_wide.h")
A2D2_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_a2d2.h")
NUS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_nus.h")
FOV_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_fov.h")
FULL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pmf_amd_full.h")


class PMFLibraryError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int32, "int8_t": C.c_int8, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
            "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "unsigned long long": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
# a `const T*` parameter of these keeps its type, so that a byref() of the wrong struct is refused; every other pointer is a
# c_void_p, and so is a `..._dev` parameter: an array in DEVICE memory, handed over as data_ptr()
_TYPED_POINTEES = ("pmf_conv_desc_t", "pmf_wgrad_desc_t", "pmf_view_t")
_DECL = re.compile(r"([A-Za-z_]\w*(?: [A-Za-z_]\w*)*?) ?((?:\* ?)*)(\w+)?((?: ?\[[^\]]*\])*)")


def _split(decl):
    """`const float* x[4]` -> match of _DECL: type words, stars, name (optional), array bounds; None if it is not of that form"""
    return _DECL.fullmatch(" ".join(re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()))


def _statements(text):
    """the pieces of `text` between the `;` outside braces"""
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            out.append(text[start:i].strip())
            start = i + 1
    if depth or text[start:].strip():
        raise PMFLibraryError("pmf_amd.h: unterminated declaration: %r" % text[start:].strip()[:200])
    return out


def _int(expr, consts):
    """value of a C integer expression over literals, known constants and ( ) + - * << >> | & ~ ^ (nothing else reaches eval)"""
    if not re.fullmatch(r"[\w\s()+\-*<>|&~^]+", expr):
        raise ValueError(expr)
    try:
        v = eval(expr, {"__builtins__": {}}, dict(consts))
    except Exception:
        raise ValueError(expr)
    if type(v) is not int:
        raise ValueError(expr)
    return v


class _Reader:
    def __init__(self):
        self.consts, self.structs, self.protos, self.aliases = {}, {}, {}, {}

    def declarator(self, decl, what, member):
        """one `type name` -> (name, ctypes type); `what` is the whole declaration, for the error message"""
        def bad(why):
            return PMFLibraryError("pmf_amd.h: cannot bind `%s`: %s" % (" ".join(what.split()), why))
        m = _split(decl)
        if not m:
            raise bad("not a plain `type name` declaration (bit-field, function pointer, `...`?)")
        base, stars, name, arr = m.group(1), m.group(2).count("*"), m.group(3), m.group(4)
        if base in self.aliases:        # `typedef void* pmf_stream_t;`
            base, stars = self.aliases[base][0], stars + self.aliases[base][1]
        known = _SCALARS.get(base) or self.structs.get(base)
        if known is None and base not in ("void", "char"):
            raise bad("unknown type `%s`" % base)
        if stars or (arr and not member):
            typed = (base in _TYPED_POINTEES and stars == 1 and not arr and "const" in decl.split()
                     and not (name or "").endswith("_dev"))
            t = C.POINTER(known) if typed else C.c_void_p
        elif base in _SCALARS or (member and known is not None):
            t = known
        else:
            raise bad("`%s` by value" % base)
        if member:
            for bound in reversed(re.findall(r"\[([^\]]*)\]", arr)):
                try:
                    t = t * _int(bound, self.consts)
                except ValueError:
                    raise bad("array bound `%s`" % bound)
        return name, t

    def struct(self, kind, body, pyname):
        fields = []
        for st in _statements(body):
            m = re.fullmatch(r"(struct|union)\s*\{(.*)\}\s*(\w+)", st, re.S)
            if m:       # anonymous aggregate with one declarator: `union { ... } u;`
                fields.append((m.group(3), self.struct(m.group(1), m.group(2), "%s_%s" % (pyname, m.group(3)))))
                continue
            first, *more = st.split(",")
            base = _split(first)        # `int32_t H, W;`: the type words go with every declarator, the stars do not
            for piece in [first] + ["%s %s" % (base.group(1) if base else "?", p) for p in more]:
                name, t = self.declarator(piece, st, True)
                if not name:
                    raise PMFLibraryError("pmf_amd.h: member without a name in `%s`" % " ".join(st.split()))
                fields.append((name, t))
        return type(pyname, (C.Union if kind == "union" else C.Structure,), {"_fields_": fields})

    def prototype(self, st):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", st, re.S)
        if not m or not m.group(1).strip():
            raise PMFLibraryError("pmf_amd.h: neither a typedef, an enum nor a prototype: `%s`" % " ".join(st.split()))
        ret, name, params = m.groups()
        if re.fullmatch(r"\s*(const\s+)?char\s*\*\s*", ret):
            restype = C.c_char_p
        else:
            restype = None if ret.split() == ["void"] else self.declarator(ret + " _", st, False)[1]
        params = [] if params.split() in ([], ["void"]) else params.split(",")
        self.protos[name] = (restype, [self.declarator(p, st, False)[1] for p in params])


def read_header(text, struct_names=None, base=None):
    """Parse the text of a C header of pmf_amd.h's kind.  Returns a namespace with
    consts: {name: int} of the `#define NAME <integer expression>` lines and the enumerators,
    structs: {C name: ctypes class} of the `typedef struct { ... } name;` blocks (class name from struct_names),
    protos: {function: (restype, [argtypes])} in declaration order,
    aliases: {name: (base type, stars)} of the `typedef T* name;` lines.
    base: the namespace of a header this one includes (`#include` lines are skipped, not followed): its constants, structs
    and aliases are known while reading, and only what THIS text declares is returned."""
    r, names = _Reader(), struct_names or {}
    inherited = (set(), set())
    if base is not None:
        r.consts.update(base.consts)
        r.structs.update(base.structs)
        r.aliases.update(base.aliases)
        inherited = (set(base.consts), set(base.structs))
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text.replace("\\\n", " "), flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#[^\n]*", text, re.M):
        directive, rest = re.match(r"\s*#\s*(\w*)(.*)", line).groups()
        if directive == "define":
            m = re.fullmatch(r"\s+(\w+)\s+(.*\S)\s*", rest)
            try:
                if m:
                    r.consts[m.group(1)] = _int(m.group(2), r.consts)
            except ValueError:
                pass        # a macro that is no integer expression is no constant of the binding
        elif directive not in ("include", "ifndef", "endif"):
            raise PMFLibraryError("pmf_amd.h: preprocessor directive the reader does not follow: `%s`" % line.strip())
    for st in _statements(re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)):
        m = re.fullmatch(r"(?:typedef\s+)?enum\s*\w*\s*\{(.*)\}\s*\w*", st, re.S)
        if m:
            nxt = 0
            for item in filter(None, (s.strip() for s in m.group(1).split(","))):
                name, _, expr = (s.strip() for s in item.partition("="))
                try:
                    nxt = r.consts[name] = (_int(expr, r.consts) if expr else nxt)
                except ValueError:
                    raise PMFLibraryError("pmf_amd.h: enumerator `%s` is not an integer expression" % item)
                nxt += 1
            continue
        m = re.fullmatch(r"typedef\s+(struct|union)\s*\w*\s*\{(.*)\}\s*(\w+)", st, re.S)
        if m:
            r.structs[m.group(3)] = r.struct(m.group(1), m.group(2), names.get(m.group(3), m.group(3)))
            continue
        m = re.fullmatch(r"typedef\s+([\w\s]+?)\s*((?:\*\s*)*)(\w+)", st)
        if m:           # `typedef void* pmf_stream_t;`
            base = " ".join(re.sub(r"\bconst\b", " ", m.group(1)).split())
            if base not in _SCALARS and base not in r.structs and base != "void":
                raise PMFLibraryError("pmf_amd.h: cannot bind `%s`: unknown type `%s`" % (st, base))
            r.aliases[m.group(3)] = (base, m.group(2).count("*"))
            continue
        r.prototype(st)
    return types.SimpleNamespace(consts={k: v for k, v in r.consts.items() if k not in inherited[0]},
                                 structs={k: v for k, v in r.structs.items() if k not in inherited[1]},
                                 protos=r.protos, aliases=r.aliases)


# header name -> name in this module
_STRUCT_NAMES = {"pmf_src_t": "Src", "pmf_conv_dst_t": "ConvDst", "pmf_conv_desc_t": "ConvDesc",
                 "pmf_wgrad_desc_t": "WgradDesc", "pmf_view_t": "View", "pmf_small_args_t": "SmallArgs", "pmf_op_t": "Op",
                 "pmf_pack_job_t": "PackJob", "pmf_bev_extent_t": "BevExtent"}


_SENSAT_STRUCT_NAMES = {"pmf_bev_sample_t": "BevSample"}


def _read(path=None, struct_names=_STRUCT_NAMES, base=None):
    path = HEADER_PATH if path is None else path
    if not os.path.exists(path):
        raise PMFLibraryError("pmf_amd: %s not found -- the binding is derived from the header, it ships with the package "
                              "tree.  There is no hand-written copy to fall back to." % path)
    with open(path) as f:
        h = read_header(f.read(), struct_names, base)
    lacking = [c for c in struct_names if c not in h.structs]
    if lacking:
        raise PMFLibraryError("pmf_amd: %s does not define %s" % (path, ", ".join(lacking)))
    return h


_H = _read()
# the SensatUrban training loader's part of the ABI (csrc/bev_train.hip): a header of its own on top of the first one
_HS = _read(SENSAT_HEADER_PATH, _SENSAT_STRUCT_NAMES, _H)
# 33..64 classes (csrc/elementwise.hip, csrc/loss.hip): prototypes only, no struct and no constant
_HW = _read(WIDE_HEADER_PATH, {}, _H)
# the A2D2 loader (csrc/undistort.hip, csrc/a2d2.hip): prototypes and the two lens kinds
_HA = _read(A2D2_HEADER_PATH, {}, _H)
# the nuScenes projection chain (csrc/nus_project.hip): one prototype, the block size, the chain length and the two modes
_HN = _read(NUS_HEADER_PATH, {}, _H)
# the SemanticKITTI-FOV filter (csrc/project.hip): one prototype, the block size and the frames per call
_HF = _read(FOV_HEADER_PATH, {}, _H)
# full sweeps from FOV predictions (csrc/project.hip): one prototype and the two workspace constants
_HK = _read(FULL_HEADER_PATH, {}, _H)
# PMF_ACT_RELU -> ACT_RELU, PMF_OP_CONV -> OP_CONV, PMF_MAX_SRC -> MAX_SRC ...; the error codes keep their prefix (PMF_E_ARG)
globals().update((k if k.startswith("PMF_E_") else k[4:], v) for k, v in _H.consts.items() if k.startswith("PMF_"))
globals().update((py, _H.structs[c]) for c, py in _STRUCT_NAMES.items())
WG_STAGED, WG_W8 = 2, 4    # retired with their kernels (docs/rounds/r15.md): never returned, kept so that code naming them imports
OP_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("OP_")}
EXPORTS = list(_H.protos)       # every function the header declares
globals().update((k[4:], v) for k, v in _HS.consts.items() if k.startswith("PMF_"))      # BEV_HFLIP, BEV_VFLIP
globals().update((py, _HS.structs[c]) for c, py in _SENSAT_STRUCT_NAMES.items())
EXPORTS_SENSAT = list(_HS.protos)       # every function pmf_amd_sensat.h declares
EXPORTS_WIDE = list(_HW.protos)         # every function pmf_amd_wide.h declares
EXPORTS_A2D2 = list(_HA.protos)         # every function pmf_amd_a2d2.h declares
globals().update((k[4:], v) for k, v in _HA.consts.items() if k.startswith("PMF_"))      # LENS_TELECAM, LENS_FISHEYE
EXPORTS_NUS = list(_HN.protos)           # every function pmf_amd_nus.h declares
globals().update((k[4:], v) for k, v in _HN.consts.items() if k.startswith("PMF_"))      # NUS_BLOCK, NUS_CHAIN, NUS_IMAGE, NUS_YAW
EXPORTS_FOV = list(_HF.protos)           # every function pmf_amd_fov.h declares
globals().update((k[4:], v) for k, v in _HF.consts.items() if k.startswith("PMF_"))      # FOV_BLOCK, FOV_MAX_FRAMES
EXPORTS_FULL = list(_HK.protos)          # every function pmf_amd_full.h declares
globals().update((k[4:], v) for k, v in _HK.consts.items() if k.startswith("PMF_"))      # FULL_WS_PER_BLOCK, FULL_WS_FIXED
NARROW_CLASSES, WIDE_CLASSES = 32, 64   # class limit of pmf_amd.h's softmax / loss entry points, and of pmf_amd_wide.h's


def bind(handle):
    """Set restype and argtypes of every function of the header that `handle` (a CDLL of this library, or of a private
    build of some of its sources) exports; returns the handle."""
    for name, (restype, argtypes) in list(_H.protos.items()) + list(_HS.protos.items()) + list(_HW.protos.items()) \
            + list(_HA.protos.items()) + list(_HN.protos.items()) + list(_HF.protos.items()) \
            + list(_HK.protos.items()):
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return handle


_lib = None


def lib():
    """Load libpmf_amd.so once; raise loudly (no fallback) if it is absent or ABI-incompatible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PMFLibraryError(
            "pmf_amd: %s not found -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pmf_amd/csrc`).  There is no CPU / PyTorch fallback for the HIP hot path." % LIB_PATH)
    L = bind(C.CDLL(LIB_PATH))
    missing = [name for name in EXPORTS if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_SENSAT if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_sensat.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_WIDE if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_wide.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_A2D2 if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_a2d2.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_NUS if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_nus.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_FOV if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_fov.h declares" % (LIB_PATH, ", ".join(missing)))
    missing = [name for name in EXPORTS_FULL if not hasattr(L, name)]
    if missing:
        raise PMFLibraryError("pmf_amd: %s lacks %s, which include/pmf_amd_full.h declares" % (LIB_PATH, ", ".join(missing)))
    if L.pmf_wide_max_classes() != WIDE_CLASSES:
        raise PMFLibraryError("pmf_amd: %s takes up to %d classes, the binding expects %d"
                              % (LIB_PATH, L.pmf_wide_max_classes(), WIDE_CLASSES))
    for which, st in enumerate((Src, ConvDesc, WgradDesc, View, SmallArgs, Op, PackJob)):    # the order pmf_sizeof documents
        if L.pmf_sizeof(which) != C.sizeof(st):
            raise PMFLibraryError("pmf_amd ABI mismatch for %s: lib %d vs binding %d"
                                  % (st.__name__, L.pmf_sizeof(which), C.sizeof(st)))
    if L.pmf_sizeof_sensat() != C.sizeof(BevSample):
        raise PMFLibraryError("pmf_amd ABI mismatch for BevSample: lib %d vs binding %d"
                              % (L.pmf_sizeof_sensat(), C.sizeof(BevSample)))
    _lib = L
    return L


def check(rc, what="pmf call", failed_at=None):
    if rc != 0:
        extra = "" if failed_at is None else " at op #%d" % failed_at
        raise RuntimeError("%s failed with code %d%s (negative = argument error, positive = hipError_t)"
                           % (what, rc, extra))
