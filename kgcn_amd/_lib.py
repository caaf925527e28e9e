"""ctypes binding of libkgcn_hip.so, derived at import from the C ABI's own text, include/kgcn_hip.h.

The header is the only place an entry point, a structure or a limit is written down: parse_header() turns its prototypes
into SIGNATURES, its structures into the ctypes.Structure classes below and its #define / enum values into K.  A new entry
point is added to the header and the library, and nothing here.

There is no CPU fallback: if the header or the shared library is missing, or the library lacks a symbol, importing this
module raises.  PyTorch is used only for device memory and streams; every call passes raw device pointers and the current
HIP stream.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# Development overrides.  KGCN_HIP_LIB: load another build of the library (tools/variant_bench.py times alternative builds).
# KGCN_GIN_JOIN / KGCN_GIN_DOT: Python-side routing switches.  (The library's own development knobs exist only
# in a -DKGCN_DEV_KNOBS build, make DEV_KNOBS=1; the dense family and the batched SpMM have none left.)  Anything set here is
# reported by active_overrides() (bench.py prints it in its JSON line) and warned about once at import, because a stray
# variable changes summation order / which binary produced the numbers.
DEV_ENV_VARS = ("KGCN_HIP_LIB", "KGCN_GIN_JOIN", "KGCN_GIN_DOT")
LIB_PATH = os.environ.get("KGCN_HIP_LIB") or os.path.join(_HERE, "csrc", "libkgcn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kgcn_hip.h")


def active_overrides():
    """Development environment switches that are set in this process (name -> value); {} in a clean environment."""
    return {k: os.environ[k] for k in DEV_ENV_VARS if os.environ.get(k)}


if active_overrides():
    import warnings
    warnings.warn("kgcn_amd: development overrides active: %r (KGCN_HIP_LIB swaps the native library, the others "
                  "change kernel routing)" % (active_overrides(),), RuntimeWarning, stacklevel=2)


# -- the header's grammar ---------------------------------------------------------------------------
# parse_header accepts what include/kgcn_hip.h uses and nothing wider; text it does not understand raises a ValueError
# that quotes it, so a declaration is never skipped silently.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
_FIELD_SCALARS = ("int32_t", "int64_t", "float")
_POINTEES = tuple(_SCALARS) + ("void", "char", "int8_t", "uint8_t", "double")    # what an untyped pointer may point to
# Structures an entry point takes by typed pointer (ctypes then checks what a caller passes).  Pointers to the other
# structures stay untyped like every pointer to plain data: their callers hand over job arrays or raw addresses.
_TYPED_POINTERS = ("kgcn_csr_batch", "kgcn_stack_layer", "kgcn_assemble_plan", "kgcn_spmm_route")
_PREAMBLE = re.compile(r'\s*#ifndef (\w+)\n#define \1\n\s*#include <stdint\.h>\n\s*#ifdef __cplusplus\nextern "C" \{\n#endif\n')
_EPILOGUE = "#ifdef __cplusplus\n}\n#endif\n#endif"
_DEFINE = re.compile(r"#define[ \t]+(\w+)[ \t]*([^\n]*)\n\s*")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;\s*")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;\s*")
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(kgcn_\w+)\s*\(([^(){};]*)\)\s*;\s*")
_EXPR_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?(?:ll|LL)?)(?!\w)|(<<|[()])|([A-Za-z_]\w*))")
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?$")


def _integer(expr, constants):
    """Value of a constant expression: decimal or hex literals (u / ll / ull suffix), <<, parentheses, earlier constants."""
    tokens, pos = [], 0
    while expr[pos:].strip():
        m = _EXPR_TOKEN.match(expr, pos)
        if not m:
            raise ValueError("kgcn_hip.h: %r is not an integer expression" % expr)
        lit, op, name = m.groups()
        if name is not None and name not in constants:
            raise ValueError("kgcn_hip.h: %r names %r, which is no earlier constant" % (expr, name))
        tokens.append(int(lit, 0) if lit is not None else op if op is not None else constants[name])
        pos = m.end()

    def shifts():
        v = atom()
        while tokens and tokens[0] == "<<":
            tokens.pop(0)
            v <<= atom()
        return v

    def atom():
        if not tokens or tokens[0] in ("<<", ")"):
            raise ValueError("kgcn_hip.h: %r is not an integer expression" % expr)
        t = tokens.pop(0)
        if t != "(":
            return t
        v = shifts()
        if not tokens or tokens.pop(0) != ")":
            raise ValueError("kgcn_hip.h: unbalanced parentheses in %r" % expr)
        return v

    v = shifts()
    if tokens:
        raise ValueError("kgcn_hip.h: %r is not an integer expression" % expr)
    return v


def _pointer(base, stars, structs, what):
    if base not in _POINTEES and base not in structs:
        raise ValueError("kgcn_hip.h: unknown type %r in %r" % (base, what))
    return ctypes.POINTER(ctypes.c_void_p) if stars == 2 else ctypes.c_void_p


def _struct(c_name, body, structs, constants):
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = re.match(r"(\w+)\b\s*(.+)$", re.sub(r"\bconst\b", " ", stmt).strip(), flags=re.S)
        if not m:
            raise ValueError("kgcn_hip.h: cannot type the field %r of %s" % (stmt, c_name))
        base = m.group(1)
        for decl in m.group(2).split(","):
            m = _DECLARATOR.match(decl.strip())
            if not m:
                raise ValueError("kgcn_hip.h: cannot type the field %r of %s" % (stmt, c_name))
            stars, name, extent = len(m.group(1)), m.group(2), m.group(3)
            if stars == 0 and base in _FIELD_SCALARS:
                ctype = _SCALARS[base]
            elif stars == 1 and base in structs:
                ctype = ctypes.POINTER(structs[base])
            elif stars == 1:
                ctype = _pointer(base, 1, structs, stmt)
            else:
                raise ValueError("kgcn_hip.h: cannot type the field %r of %s" % (stmt, c_name))
            fields.append((name, ctype if extent is None else ctype * _integer(extent, constants)))
    cls_name = "".join(w.capitalize() for w in c_name[len("kgcn_"):].split("_"))
    return type(cls_name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "struct %s (include/kgcn_hip.h)." % c_name})


def _prototype(restype, name, params, structs):
    what = "%s %s(%s)" % (restype.strip(), name, " ".join(params.split()))
    restype, params = (re.sub(r"\bconst\b", " ", s).replace("*", " * ") for s in (restype, params))

    def ctype(text, is_return):
        words = text.split()
        stars = words.count("*")
        words = [w for w in words if w != "*"]
        if len(words) != (1 if is_return else 2) or stars > 2:
            raise ValueError("kgcn_hip.h: cannot type %r in %r" % (text.strip(), what))
        base = words[0]
        if stars == 0:
            if base not in _SCALARS:
                raise ValueError("kgcn_hip.h: unknown type %r in %r" % (base, what))
            return _SCALARS[base]
        if is_return:
            if (base, stars) != ("char", 1):
                raise ValueError("kgcn_hip.h: unknown return type %r in %r" % (text.strip(), what))
            return ctypes.c_char_p
        if stars == 1 and base in _TYPED_POINTERS and base in structs:
            return ctypes.POINTER(structs[base])
        return _pointer(base, stars, structs, what)

    args = [] if params.strip() == "void" else [ctype(p, False) for p in params.split(",")]
    return ctype(restype, True), args


def parse_header(text):
    """The text of include/kgcn_hip.h -> (functions, structs, constants):
      functions  name -> (restype, [argtypes]) of every prototype: scalars by name; one * to a structure of _TYPED_POINTERS
                 is a POINTER to its class, two * are POINTER(c_void_p), every other pointer is c_void_p, and a
                 `const char*` return is c_char_p
      structs    C name -> ctypes.Structure class (kgcn_csr_batch -> CsrBatch) with the header's fields in the header's order
      constants  name -> int for every `#define KGCN_*` and every enumerator
    Pure: reads no file and touches no library."""
    functions, structs, constants = {}, {}, {}

    def constant(name, value, what):
        if not name.startswith("KGCN_") or name in constants or not value:
            raise ValueError("kgcn_hip.h: unexpected or repeated name, or no value, in %r" % what)
        constants[name] = _integer(value, constants)

    def define(m):
        constant(m.group(1), m.group(2), m.group(0).strip())

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, value = (s.strip() for s in item.partition("="))
            constant(name, value, item)

    def struct(m):
        if m.group(1) != m.group(3) or m.group(1) in structs or not m.group(1).startswith("kgcn_"):
            raise ValueError("kgcn_hip.h: unexpected or repeated structure name in %r" % " ".join(m.group(0).split()))
        structs[m.group(1)] = _struct(m.group(1), m.group(2), structs, constants)

    def prototype(m):
        if m.group(2) in functions:
            raise ValueError("kgcn_hip.h: %s is declared twice" % m.group(2))
        functions[m.group(2)] = _prototype(m.group(1), m.group(2), m.group(3), structs)

    text = re.sub(r"/\*.*?\*/", lambda c: " " + "\n" * c.group(0).count("\n"), text, flags=re.S)   # a comment ends no line early
    text = "\n".join(line.rstrip() for line in text.split("\n")).rstrip()
    head = _PREAMBLE.match(text)
    if not head or not text.endswith(_EPILOGUE):
        raise ValueError("kgcn_hip.h: include guard / extern \"C\" frame not found")
    body, pos = text[head.end():-len(_EPILOGUE)].strip() + "\n", 0
    while pos < len(body):
        for pattern, read in ((_DEFINE, define), (_ENUM, enum), (_STRUCT, struct), (_PROTOTYPE, prototype)):
            m = pattern.match(body, pos)
            if m:
                read(m)
                pos = m.end()
                break
        else:
            raise ValueError("kgcn_hip.h: cannot read %r" % " ".join(body[pos:body.find(";", pos) + 1 or pos + 120].split()))
    return functions, structs, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise ImportError("kgcn_amd: the C header %s is missing (%s); the binding is derived from it" % (HEADER_PATH, e)) from e


# name -> (restype, argtypes) of every function the header declares; C structure name -> class; K: every constant by name
SIGNATURES, _STRUCTS, K = parse_header(_read_header())

CsrBatch, AssemblePlan, WtableJob, AdamSegment, StackLayer, SpmmRoute, Copy2dJob = (_STRUCTS[s] for s in (
    "kgcn_csr_batch", "kgcn_assemble_plan", "kgcn_wtable_job", "kgcn_adam_segment", "kgcn_stack_layer", "kgcn_spmm_route",
    "kgcn_copy2d_job"))
# the library must report the same version and the same sizeof(kgcn_csr_batch) as the header this binding was read from
ABI_VERSION = K["KGCN_HIP_ABI_VERSION"]
ASSEMBLE_MAX_CSR, ASSEMBLE_MAX_TABLES = K["KGCN_ASSEMBLE_MAX_CSR"], K["KGCN_ASSEMBLE_MAX_TABLES"]
# kgcn_spmm_route.kernel (the KGCN_SPMM_* enumerators) -> the kernel of csrc/spmm.hip without its _kernel suffix; call flags
SPMM_KERNELS = ("none", "spmm_tile", "spmm_tile_dot", "spmm_slices", "spmm_block", "spmm_rows", "spmm_gather", "bconv_loop",
                "bconv_fanout")
SPMM_DACT, SPMM_SELF_SCALE, SPMM_DOT, SPMM_FANOUT = (K[n] for n in (
    "KGCN_SPMM_DACT", "KGCN_SPMM_SELF_SCALE", "KGCN_SPMM_DOT", "KGCN_SPMM_FANOUT"))


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "kgcn_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C kgcn_amd/csrc` (hipcc --offload-arch=gfx950). There is no "
            "CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError("kgcn_amd: %s does not export %s (stale build?)" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.kgcn_abi_version() != ABI_VERSION:
        raise ImportError("kgcn_amd: ABI version mismatch: library %d, binding %d" % (lib.kgcn_abi_version(), ABI_VERSION))
    if lib.kgcn_csr_batch_size() != ctypes.sizeof(CsrBatch):
        raise ImportError("kgcn_amd: kgcn_csr_batch is %d bytes in the library, %d in the binding (stale build?)"
                          % (lib.kgcn_csr_batch_size(), ctypes.sizeof(CsrBatch)))
    return lib


lib = _load()


class KgcnHipError(RuntimeError):
    pass


def check(rc, what=""):
    """Raise on a non-zero status, with the library's message (error convention of the ABI)."""
    if rc != 0:
        msg = lib.kgcn_last_error()
        raise KgcnHipError("%s failed: %s" % (what or "kgcn_hip call",
                                              msg.decode() if msg else "unknown error"))


def spmm_route(descs, num_channels, d, rhs_ld, rhs_gs, channel_stride, out_ld, out_gs, align=16, flags=0):
    """kgcn_spmm_route_query: which kernel of csrc/spmm.hip the call described takes -> (kernel name out of SPMM_KERNELS, its
    template arguments, the filled SpmmRoute).  descs: a kgcn_csr_batch or an array of them (BatchedCSR.desc(),
    BatchedAdjacency.desc_array()); host code, no GPU needed."""
    r = SpmmRoute()
    check(lib.kgcn_spmm_route_query(descs, num_channels, d, rhs_ld, rhs_gs, channel_stride, out_ld, out_gs, align, flags,
                                    ctypes.byref(r)), "kgcn_spmm_route_query")
    return SPMM_KERNELS[r.kernel], list(r.template_args), r


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def workspace(nbytes, device, dtype=None):
    """Scratch tensor for a C call's workspace argument: at least `nbytes` bytes (rounded up to whole elements of `dtype`,
    default float32) and at least one element, so its pointer is never NULL."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    return torch.empty((max(-(-int(nbytes) // dtype.itemsize), 1),), device=device, dtype=dtype)


def require_gpu(t, name):
    if not t.is_cuda:
        raise KgcnHipError(
            "%s must live on the GPU (cuda/HIP device); kgcn_amd has no CPU path" % name)
