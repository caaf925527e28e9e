"""CPU-side checks of the drop-in boundary: libkgcn_hip.so loads (no GPU needed), exports every
symbol include/kgcn_hip.h declares, the Python binding -- derived from that header by _lib.parse_header --
lists exactly those symbols, every structure and every constant, the parser refuses what it does not
understand, shape queries answer, and argument validation fails loudly (no compute launches here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kgcn_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(kgcn_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


STRUCTS = {"kgcn_csr_batch": "CsrBatch", "kgcn_assemble_plan": "AssemblePlan", "kgcn_wtable_job": "WtableJob",
           "kgcn_adam_segment": "AdamSegment", "kgcn_stack_layer": "StackLayer", "kgcn_spmm_route": "SpmmRoute",
           "kgcn_copy2d_job": "Copy2dJob"}


def header_abi_version():
    return int(re.search(r"#define\s+KGCN_HIP_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))


def consumer_binary():
    """tests/abi_consumer.bin, (re)built with plain gcc when it is missing or older than its source / the header."""
    import __graft_entry__ as g
    out = os.path.join(ROOT, "tests", "abi_consumer.bin")
    srcs = (os.path.join(ROOT, "tests", "abi_consumer.c"), HEADER)
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        if not os.path.exists("/usr/bin/gcc"):
            pytest.skip("no gcc and no prebuilt abi_consumer.bin")
        g.build_abi_consumer()
    return out


def run_consumer(mode):
    import subprocess
    p = subprocess.run([consumer_binary(), mode], capture_output=True, text=True, timeout=120)
    facts = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        facts[k] = v
    return p.returncode, facts, p.stdout + p.stderr


def test_c_consumer_sees_the_layout_the_binding_mirrors():
    """A plain-C program compiled against include/kgcn_hip.h: its sizeof / offsetof of kgcn_csr_batch, the library's
    kgcn_csr_batch_size() and the ctypes mirror in kgcn_amd/_lib.py must all agree -- layout drift that a ctypes-only test
    cannot see (the struct grew in ABI version 2)."""
    from kgcn_amd import _lib
    rc, facts, text = run_consumer("layout")
    assert rc == 0 and "OK" in facts, text
    assert int(facts["header_abi_version"]) == int(facts["library_abi_version"]) == _lib.ABI_VERSION
    assert int(facts["sizeof_csr_batch"]) == int(facts["library_csr_batch_size"]) == ctypes.sizeof(_lib.CsrBatch)
    for field in ("nnz", "rowptr", "cv", "slots", "graph_ptr", "block_ptr", "num_blocks", "block_rows_max"):
        assert int(facts["offsetof_" + field]) == getattr(_lib.CsrBatch, field).offset, field
    assert int(facts["sizeof_wtable_job"]) == ctypes.sizeof(_lib.WtableJob)
    assert int(facts["offsetof_wtable_job_table"]) == _lib.WtableJob.table.offset
    assert int(facts["offsetof_wtable_job_extra_row"]) == _lib.WtableJob.extra_row.offset
    assert "NULL" in facts["last_error"]
    for c_name, cls_name in STRUCTS.items():            # all seven: sizeof and the last field, as the C compiler lays them out
        cls = getattr(_lib, cls_name)
        size, last, offset = facts["layout_" + c_name].split()
        assert int(size) == ctypes.sizeof(cls), c_name
        assert last == cls._fields_[-1][0] and int(offset) == getattr(cls, last).offset, c_name


def test_header_declares_the_path():
    names = declared_functions()
    for must in ("kgcn_bspmm_f32", "kgcn_bconv_f32", "kgcn_spmm_values_grad_f32", "kgcn_dense_fwd_f32",
                 "kgcn_dense_wgrad_f32", "kgcn_graphconv_fwd_f32", "kgcn_graphconv_bwd_f32",
                 "kgcn_gin_aggregate_f32", "kgcn_graph_gather_fwd_f32", "kgcn_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from kgcn_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), "libkgcn_hip.so does not export %s" % name
    assert sorted(_lib.SIGNATURES) == declared_functions(), "binding and header disagree"
    assert _lib.lib.kgcn_abi_version() == _lib.ABI_VERSION == header_abi_version()
    assert _lib.lib.kgcn_csr_batch_size() == ctypes.sizeof(_lib.CsrBatch)
    assert _lib.lib.kgcn_build_arch() == b"gfx950"


def test_binding_holds_every_structure_and_constant_of_the_header():
    """A second, independent reader of the header (plain regular expressions here) counts what parse_header must have found:
    a structure or a #define its expressions fail to match would be missing from the binding."""
    from kgcn_amd import _lib
    src = header_without_comments()
    functions, structs, constants = _lib.parse_header(open(HEADER).read())
    assert functions.keys() == _lib.SIGNATURES.keys() and constants == _lib.K
    typedefs = re.findall(r"typedef\s+struct\s+(kgcn_\w+)", src)
    assert len(typedefs) == len(structs) == 7 and sorted(typedefs) == sorted(structs) == sorted(STRUCTS)
    for c_name, cls_name in STRUCTS.items():
        assert structs[c_name].__name__ == cls_name and issubclass(getattr(_lib, cls_name), ctypes.Structure)
        assert [f[0] for f in structs[c_name]._fields_] == [f[0] for f in getattr(_lib, cls_name)._fields_]
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(KGCN_\w+)[ \t]+\S", src, flags=re.M)    # the include guard has no value
    assert len(defines) == len(set(defines)) == 66
    for name in defines:
        assert isinstance(_lib.K[name], int), name
    assert _lib.K["KGCN_ROW_PAD_COMPACT"] == 0x104 and _lib.K["KGCN_LP_MAX_BATCH"] == 1 << 22
    assert _lib.K["KGCN_BINARY_METRICS_MAX_ELEMENTS"] == 1 << 31 and _lib.K["KGCN_IG_STREAM_SEQUENCE"] == 0x100
    # SPMM_KERNELS spells kernel names, not enumerators: it must have one name per enumerator of the route codes
    enum = re.search(r"enum\s*\{(.*?)\}", src, flags=re.S).group(1)
    codes = {n: int(v) for n, v in re.findall(r"(KGCN_SPMM_\w+)\s*=\s*(\d+)", enum)}
    assert codes and all(_lib.K[n] == v for n, v in codes.items())
    assert len(_lib.SPMM_KERNELS) == max(codes.values()) + 1
    assert (_lib.SPMM_DACT, _lib.SPMM_SELF_SCALE, _lib.SPMM_DOT, _lib.SPMM_FANOUT) == (1, 2, 4, 8)


SNIPPET = """/* a header in the grammar of kgcn_hip.h */
#ifndef X_H_
#define X_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define KGCN_N (1 << 2)   /* a limit */
#define KGCN_BIG (1ll << 33)
#define KGCN_MASK 0x10u
typedef struct kgcn_csr_batch {
  int32_t a, b[KGCN_N];   /* two declarators */
  const float* p;
  int64_t n[2];
} kgcn_csr_batch;
typedef struct kgcn_pair {
  const kgcn_csr_batch* src[KGCN_N];
  float eps;
} kgcn_pair;
%s
int kgcn_first(const kgcn_csr_batch* a, const float* x, int64_t ld, float* const* outs, uint64_t seed, float beta,
               const kgcn_pair* pairs, void* stream);
const char* kgcn_second(void);
#ifdef __cplusplus
}
#endif
#endif /* X_H_ */
"""


def test_parse_header_types_a_snippet():
    from kgcn_amd import _lib
    functions, structs, constants = _lib.parse_header(SNIPPET % "")
    assert constants == {"KGCN_N": 4, "KGCN_BIG": 1 << 33, "KGCN_MASK": 16}
    batch, pair = structs["kgcn_csr_batch"], structs["kgcn_pair"]
    assert (batch.__name__, pair.__name__) == ("CsrBatch", "Pair") and list(structs) == ["kgcn_csr_batch", "kgcn_pair"]
    assert [(n, t) for n, t in batch._fields_] == [("a", ctypes.c_int32), ("b", ctypes.c_int32 * 4), ("p", ctypes.c_void_p),
                                                   ("n", ctypes.c_int64 * 2)]
    assert pair._fields_ == [("src", ctypes.POINTER(batch) * 4), ("eps", ctypes.c_float)]
    assert ctypes.sizeof(batch) == 48 and batch.p.offset == 24 and ctypes.sizeof(pair) == 40
    assert list(functions) == ["kgcn_first", "kgcn_second"]
    res, args = functions["kgcn_first"]
    assert res is ctypes.c_int
    # typed pointer for kgcn_csr_batch; a structure outside the typed set, like any data pointer, is c_void_p
    assert args == [ctypes.POINTER(batch), ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64,
                    ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert functions["kgcn_second"] == (ctypes.c_char_p, [])


@pytest.mark.parametrize("bad, quoted", [
    ("int kgcn_third(const float* x, size_t n);", "size_t"),                       # unknown scalar in a prototype
    ("int kgcn_third(const half* x);", "half"),                                    # unknown pointee
    ("double kgcn_third(void);", "double"),                                        # unknown return type
    ("#define KGCN_X 1.5f", "1.5f"),                                               # not an integer
    ("#define KGCN_X (KGCN_LATER << 1)", "KGCN_LATER"),                            # no EARLIER constant
    ("#define KGCN_N 5", "KGCN_N"),                                                # defined twice
    ("typedef struct kgcn_t { int32_t a; double d; } kgcn_t;", "double d"),        # field of unknown type
    ("typedef struct kgcn_t { kgcn_csr_batch inner; } kgcn_t;", "kgcn_csr_batch inner"),   # structure by value
    ("typedef struct kgcn_t { float** pp; } kgcn_t;", "float** pp"),
    ("static inline int kgcn_third(void) { return 0; }", "kgcn_third"),            # not a declaration
    ("typedef int32_t kgcn_index;", "kgcn_index"),
])
def test_parse_header_refuses_what_it_does_not_understand(bad, quoted):
    from kgcn_amd import _lib
    with pytest.raises(ValueError) as e:
        _lib.parse_header(SNIPPET % bad)
    assert quoted in str(e.value), str(e.value)


def test_code_object_is_gfx950_only():
    from kgcn_amd import _lib
    import re
    blob = open(_lib.LIB_PATH, "rb").read()
    # the offload bundle lists one entry id per device code object: "hipv4-amdgcn-amd-amdhsa--<arch>" (bare arch names also
    # occur as strings of rocPRIM's host-side tuning tables -- those are not code)
    targets = set(re.findall(rb"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert targets == {b"gfx950"}, targets
    for other in (b"sm_90", b"nvptx"):
        assert other not in blob


def test_shape_queries_and_validation():
    from kgcn_amd import _lib
    lib = _lib.lib
    assert lib.kgcn_graphconv_fused_supported(32, 64, 64, 100) == 1
    assert lib.kgcn_graphconv_fused_supported(10, 4, 52, 24) == 1
    assert lib.kgcn_graphconv_fused_supported(10, 3, 50, 24) == 1       # any width <= 64 (scalar tile path)
    assert lib.kgcn_graphconv_fused_supported(10, 65, 50, 24) == 0
    assert lib.kgcn_graphconv_fused_supported(50, 64, 64, 160) == 0      # N > 32
    assert lib.kgcn_graphconv_fused_supported(32, 128, 64, 100) == 0
    assert lib.kgcn_dense_wgrad_workspace_bytes(3_200_000, 64, 64) > 0
    assert lib.kgcn_graphconv_bwd_workspace_bytes(100_000, 64, 64) >= 256 * (64 * 64 + 64) * 4   # one partial per CU
    assert lib.kgcn_dot_workspace_bytes(10) > 0
    # validation happens before any launch: NULL descriptor / bad sizes -> status + message
    rc = lib.kgcn_bspmm_f32(None, None, 0, 0, 4, None, 0, 0, 0.0, None)
    assert rc != 0 and b"NULL" in lib.kgcn_last_error()
    d = _lib.CsrBatch(-1, 4, 4, 0, 0, 0, 0, None, None, None, None)
    assert lib.kgcn_bspmm_f32(ctypes.byref(d), None, 4, 16, 4, None, 4, 16, 0.0, None) != 0
    d = _lib.CsrBatch(2, 4, 4, 0, 0, 0, 0, 1, None, None, None)                            # fake non-NULL rowptr
    assert lib.kgcn_bspmm_f32(ctypes.byref(d), None, 4, 16, 4, None, 4, 16, 0.0, None) != 0
    assert b"NULL" in lib.kgcn_last_error()
    assert lib.kgcn_bspmm_f32(ctypes.byref(d), 16, 2, 16, 4, 16, 4, 16, 0.0, None) != 0   # ld < d
    assert lib.kgcn_bspmm_f32(ctypes.byref(d), 16, 4, 16, 4, 16, 4, 16, 0.5, None) != 0   # beta
    pd = _lib.CsrBatch(2, 4, 4, 16, 4, 0, 32, 1, 1, 1, 1)                        # row-padded batch
    assert lib.kgcn_bspmm_f32(ctypes.byref(pd), 16, 4, 16, 4, 16, 4, 16, 0.0, None) != 0
    assert b"row_pad" in lib.kgcn_last_error()                            # plain kernels refuse it
    with pytest.raises(_lib.KgcnHipError):
        _lib.check(lib.kgcn_dense_fwd_f32(None, 10, 0, 0, None, 0, 0, None, None, 4, 4, None), "dense")
    rc = lib.kgcn_graphconv_fwd_f32(ctypes.byref(_lib.CsrBatch(1, 50, 50, 12, 4, 0, 0, 1, None, 1, 1)), None, None,
                                    None, 64, 64, None, None)
    assert rc != 0 and b"not supported" in lib.kgcn_last_error()


def test_product_path_has_no_cpu_fallback():
    import torch
    from kgcn_amd import _lib, layers
    layer = layers.GraphConv(8, 1)
    adjs = [[([[0, 0]], [1.0], [4, 4])] for _ in range(2)]
    with pytest.raises((_lib.KgcnHipError, RuntimeError, AssertionError)):
        layer(torch.zeros((2, 4, 4)), adj=adjs)                          # CPU tensors are refused
    # nothing under kgcn_amd/ imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "kgcn_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "oracle" not in open(os.path.join(dirpath, f)).read(), f
