"""The cases of tests/test_gpu_bn_cases.py: shapes, alignments and inputs for the GraphBatchNormalization kernels
(kgcn_amd/csrc/bn.hip), with their operands, the fp64 reference of oracle/kgcn_oracle.py (graph_bn_fwd / graph_bn_bwd) and its
float32 restatement (the same two functions with dtype=np.float32), computed ONCE per case.  tests/test_bn_cases.py proves on the
CPU that every case reaches the kernel, template instance or grid cap it names -- route() below restates the host rules of
bn_apply_impl, bn_blocks and bn_grid -- so a bad shape fails there and never as a GPU mismatch.

build(name) -> Case: x, enabled (None: every row valid), gamma, beta, the moving statistics mm / mv and the output gradient g, all
float32 (enabled int32); `off`, the element offset at which x is placed in a 16-byte-aligned device buffer; ref[phase] and
f32[phase], the reference and the restatement of learning phase 0 / 1 as Result(y, dx, dgamma, dbeta, mean, var, mm, mv).  A fused
activation is applied to the oracle's output, its derivative is formed at the REFERENCE output (relu pre-activations are nudged at
least 1e-3 away from 0, so the device output need not be read back); `clamped` holds enabled values above N and below 0 and its
reference is the oracle's at clip(enabled, 0, N).

The bounds.  The error figure is max|got - ref| / max|ref|, absolute where the reference is all zero
(family_bounds.error_figure, OVER_REF_OR_ABSOLUTE); a comparison is held to

    bound = max(WRITTEN[q], 4 * E32),

WRITTEN the project's own written forms (2e-6 for y and dx: the rel=2e-6 of test_fused_activation_dense and of the act(bn)
comparison; 1e-5 for the reduced quantities mean, var, dgamma, dbeta and the moving statistics: the rel=1e-5 that test uses for dW
and dbias), E32 the same figure of the float32 restatement against the fp64 reference, and 4 the rule of tests/fused_cases.py: the
written form holds where the restatement stays under a quarter of it.  The restatement sums the rows SEQUENTIALLY in float32
(numpy's reduction over a non-contiguous axis): a longer chain than any in the kernels (about 8 row passes a thread, rpp partials
a workgroup, then the second stage).  Nothing here is measured from a kernel.  tests/test_bn_cases.py asserts 4 * E32 <= 1e-3 for
every case, phase and quantity: no bound is loose enough to hide a dropped row or a single-pass variance (which is off by 5e-3 of
var on the `offset30` data).

E32 as tests/test_bn_cases.py prints it: every (case, phase, quantity) whose 4 * E32 exceeds its written form -- all in the reduced
quantities of the long batches, or downstream of phase-1 statistics -- and the bound that makes.  Every other comparison (292 of 324)
is held to the written form; the largest E32 among those is 4.59e-07 (y, dx) and 2.45e-06 (the reduced quantities).
tests/test_bn_cases.py reads this table back and compares it with what it computes.

    case            phase  q          E32      bound
    cols4_lg8           1  y       6.57e-07  2.63e-06
    vec_wide_grid       1  y       1.05e-06  4.19e-06
    vec_wide_grid       1  dx      8.31e-07  3.32e-06
    vec_wide_grid       1  dgamma  3.05e-06  1.22e-05
    grid_256            1  y       1.48e-06  5.93e-06
    grid_256            1  dx      1.26e-06  5.05e-06
    grid_256            1  dgamma  5.32e-06  2.13e-05
    grid_256            1  var     2.82e-06  1.13e-05
    grid_50             0  dgamma  3.17e-06  1.27e-05
    grid_50             0  dbeta   2.90e-06  1.16e-05
    grid_50             1  y       2.85e-06  1.14e-05
    grid_50             1  dx      2.59e-06  1.04e-05
    grid_50             1  dgamma  5.05e-06  2.02e-05
    grid_50             1  dbeta   2.90e-06  1.16e-05
    grid_50             1  var     5.89e-06  2.36e-05
    grid_3              0  dbeta   4.31e-06  1.73e-05
    grid_3              1  y       1.26e-06  5.04e-06
    grid_3              1  dx      7.07e-07  2.83e-06
    grid_3              1  dgamma  6.21e-06  2.48e-05
    grid_3              1  dbeta   4.31e-06  1.73e-05
    grid_3              1  var     3.10e-06  1.24e-05
    offset30            1  y       1.08e-05  4.31e-05
    offset30            1  dx      8.93e-07  3.57e-06
    offset30            1  dgamma  3.28e-05  1.31e-04
    offset30            1  var     2.61e-06  1.04e-05
    const_cols          1  y       1.04e-05  4.16e-05
    const_cols          1  dgamma  5.74e-05  2.30e-04
    act_sigmoid_3       1  dx      5.74e-07  2.29e-06
    act_tanh_64         1  y       1.24e-06  4.97e-06
    act_tanh_64         1  dx      6.36e-07  2.54e-06
    act_tanh_1028       1  y       1.94e-06  7.75e-06
    act_tanh_1028       1  dx      8.53e-07  3.41e-06

(offset30's dgamma and y are the cancellation of x - mean at mean / std = 30: 30 * 2^-24 of xhat a row, summed over 4,300 rows;
const_cols' are the columns with var == 0, where rstd = 1 / sqrt(eps) = 31.6 multiplies the rounding of the mean of 3.3.)
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import family_bounds
from gpu_helpers import act64, dact64
from oracle import kgcn_oracle as K

# ---- bn.hip's host constants, restated (a comment beside each of them there names this file) ------------------------------------
COL_GROUPS = 256                 # bn_apply_impl: d / V <= 256 column groups -> bn_apply_cols_kernel<V>
BN_BLOCKS = 1024                 # bn_blocks: workgroups of a column reduction, about 8 row passes each
NUM_CU = 256                     # kNumCU (kgcn_common.h): bn_apply_cols_kernel <= 8 workgroups a CU, bn_grid <= 16

WRITTEN = {"y": 2e-6, "dx": 2e-6, "dgamma": 1e-5, "dbeta": 1e-5, "mean": 1e-5, "var": 1e-5, "mm": 1e-5, "mv": 1e-5}
QUANTITIES = {0: ("y", "dx", "dgamma", "dbeta"), 1: ("y", "dx", "dgamma", "dbeta", "mean", "var", "mm", "mv")}
E32_CAP = 1e-3                   # 4 * E32 stays under this
RELU_MARGIN = 1e-3
EPS, MOMENTUM = 1e-3, 0.99       # the layer's defaults


def route(d, x_offset_floats, rows):
    """Where bn.hip sends a [rows, d] batch whose x starts x_offset_floats floats into a 16-byte-aligned buffer (y, dx and every
    other operand are allocations of their own: 16-byte aligned):
      apply            cols4 / cols2 / cols1 (bn_apply_cols_kernel<V>), vec (bn_apply_kernel<true>), scalar (bn_apply_kernel<false>)
      V, dv            floats a column group, column groups a row (bn_apply_impl)
      lg, apply_rpp    cols only: dv rounded up to 1 << lg lanes, 256 >> lg rows a pass
      apply_capped     the apply kernel's grid-stride loop runs more than once (kNumCU * 8 workgroups cols, kNumCU * 16 else)
      cb, reduce_rpp   bn_colreduce_kernel: the widths of its column blocks and the rows a pass of each
      reduce_capped    bn_blocks hits BN_BLOCKS: the reduction's grid-stride loop takes more than its ~8 passes
      dx_capped        bn_bwd_dx_kernel's bn_grid(rows * d) hits kNumCU * 16"""
    align = (4 * x_offset_floats) % 16
    vec = d % 4 == 0 and align == 0
    V = 4 if vec else (2 if d % 2 == 0 and align % 8 == 0 else 1)
    dv = d // V
    r = {"V": V, "dv": dv}
    if dv <= COL_GROUPS:
        lg = 0
        while (1 << lg) < dv:
            lg += 1
        rpp = 256 >> lg
        r.update(apply="cols%d" % V, lg=lg, apply_rpp=rpp, apply_capped=(rows + rpp - 1) // rpp > NUM_CU * 8)
    else:
        work = rows * (d // 4 if vec else d)
        r.update(apply="vec" if vec else "scalar", apply_capped=(work + 255) // 256 > NUM_CU * 16)
    r["cb"] = [min(256, d - c0) for c0 in range(0, d, 256)]
    r["reduce_rpp"] = [256 // cb for cb in r["cb"]]
    rpp0 = 256 // min(d, 256)
    r["reduce_capped"] = (rows + 8 * rpp0 - 1) // (8 * rpp0) > BN_BLOCKS
    r["dx_capped"] = (rows * d + 255) // 256 > NUM_CU * 16
    return r


Spec = namedtuple("Spec", "shape off enabled data act with_dx expect purpose")


def _spec(shape, expect, purpose, off=0, enabled="ragged", data="plain", act=None, with_dx=True):
    return Spec(shape, off, enabled, data, act, with_dx, expect, purpose)


# expect: the entries of route() the case is there for
SPECS = {
    "cols4_lg8": _spec((40, 8, 1024), dict(apply="cols4", dv=256, lg=8, apply_rpp=1), "cols<4> at its last width"),
    "vec_wide": _spec((40, 8, 1028), dict(apply="vec", dv=257, apply_capped=False, cb=[256, 256, 256, 256, 4],
                                          reduce_rpp=[1, 1, 1, 1, 64]),
                      "bn_apply_kernel<true>; reduction over 5 column blocks, the last 4 wide"),
    "vec_wide_grid": _spec((512, 8, 1028), dict(apply="vec", apply_capped=True, dx_capped=True),
                           "bn_apply_kernel<true> past kNumCU * 16 workgroups"),
    "scalar_odd": _spec((30, 9, 257), dict(apply="scalar", V=1, cb=[256, 1], reduce_rpp=[1, 256]),
                        "bn_apply_kernel<false>; second column block 1 wide"),
    "cols1_lg8": _spec((30, 9, 255), dict(apply="cols1", dv=255, lg=8), "cols<1> at 255 column groups"),
    "even_wide": _spec((30, 9, 514), dict(apply="scalar", V=2, dv=257), "V = 2 with 257 groups: bn_apply_kernel<false>"),
    "off1_64": _spec((30, 10, 64), dict(apply="cols1", dv=64), "d % 4 == 0 but x 4-byte aligned: cols<1>", off=1),
    "off2_64": _spec((30, 10, 64), dict(apply="cols2", dv=32), "x 8-byte aligned: cols<2>", off=2),
    "off1_300": _spec((30, 10, 300), dict(apply="scalar", V=1, dv=300, cb=[256, 44], reduce_rpp=[1, 5]),
                      "bn_apply_kernel<false>, ragged; second column block 44 wide", off=1),
    "grid_256": _spec((700, 12, 256), dict(apply="cols4", apply_rpp=4, reduce_rpp=[1], reduce_capped=True, apply_capped=True,
                                           dx_capped=True),
                      "8400 rows: past BN_BLOCKS (rpp = 1), past kNumCU * 8 in cols<4>, past kNumCU * 16 in bn_bwd_dx_kernel"),
    "grid_50": _spec((4200, 10, 50), dict(apply="cols2", dv=25, lg=5, reduce_rpp=[5], reduce_capped=True, apply_capped=True),
                     "42000 rows: past BN_BLOCKS at rpp = 5; cols<2> with idle lanes"),
    "grid_3": _spec((3000, 12, 3), dict(apply="cols1", lg=2, reduce_rpp=[85]), "rpp = 85, cols<1>, lg = 2"),
    "offset30": _spec((700, 12, 64), dict(apply="cols4"), "mean / std = 30: the two-pass statistics", data="offset30"),
    "const_cols": _spec((20, 10, 16), dict(apply="cols4"), "two columns constant at 3.3, one all zero: var == 0", data="const"),
    "clamped": _spec((9, 12, 50), dict(apply="cols2"), "enabled above N and below 0",
                     enabled=[15, -1, 12, 0, 13, 3, -7, 12, 1]),
    "all_empty": _spec((6, 10, 50), dict(apply="cols2"), "no valid row: count == 0", enabled="zero"),
    "no_dx": _spec((30, 10, 64), dict(apply="cols4"), "input needs no gradient: MODE 2 in both phases", with_dx=False),
    "squeezed": _spec((12, 50), dict(apply="cols2"), "2-D input, no enabled: the layer's squeeze path", enabled=None),
}
for _act in ("sigmoid", "relu", "tanh"):
    for _d, _k in ((3, "cols1"), (64, "cols4"), (1028, "vec")):
        SPECS["act_%s_%d" % (_act, _d)] = _spec((25, 10, _d), dict(apply=_k), "fused %s in %s" % (_act, _k), act=_act)
NAMES = list(SPECS)
OFFSET_CASES = [n for n in NAMES if SPECS[n].off]

Result = namedtuple("Result", "y dx dgamma dbeta mean var mm mv")
Case = namedtuple("Case", "name spec T N D off x enabled clipped gamma beta mm mv g ref f32 e32 relu_distance")


def shape3(name):
    s = SPECS[name].shape
    return (1,) + tuple(s) if len(s) == 2 else tuple(s)


def expected_route(name):
    T, N, D = shape3(name)
    return route(D, SPECS[name].off, T * N)


def _clear_of_zero(x, valid, gamma, beta, mm, mv, en):
    """relu: move the x whose pre-activation (of either phase) lies within 2 * RELU_MARGIN of 0; a step of 0.05 moves a
    pre-activation by at least 0.5 * 0.05 / sqrt(18) = 5.9e-3, across the whole band"""
    for _ in range(20):
        bad = np.zeros(x.shape, bool)
        for phase in (0, 1):
            pre = K.graph_bn_fwd(x, gamma, beta, mm, mv, en, eps=EPS, training=bool(phase))[0]
            bad |= (np.abs(pre) < 2 * RELU_MARGIN) & valid
        if not bad.any():
            return x
        x = (x + np.where(bad, np.float32(0.05), np.float32(0))).astype(np.float32)
    raise AssertionError("relu pre-activations do not clear 0")


def _results(c, phase, dtype):
    spec = c["spec"]
    pre, mean, var, nmm, nmv = K.graph_bn_fwd(c["x"], c["gamma"], c["beta"], c["mm"], c["mv"], c["clipped"], eps=EPS,
                                              training=bool(phase), momentum=MOMENTUM, dtype=dtype)
    y = act64(pre, spec.act)
    g = np.asarray(c["g"], dtype)
    if spec.act is not None:
        g = (g * dact64(y, spec.act)).astype(dtype)                  # the derivative at the reference output
    dx, dgamma, dbeta = K.graph_bn_bwd(c["x"], c["gamma"], mean, var, g, c["clipped"], eps=EPS, training=bool(phase), dtype=dtype)
    out = Result(y, dx, dgamma, dbeta, mean, var, nmm, nmv)
    assert all(a.dtype == dtype for a in out), [a.dtype for a in out]
    return out, pre


@functools.lru_cache(maxsize=2)
def build(name):
    spec = SPECS[name]
    T, N, D = shape3(name)
    rng = np.random.default_rng([zlib.crc32(b"bn_cases"), zlib.crc32(name.encode()), 1])
    if spec.data == "offset30":
        col, scale = 30.0 * (1.0 + 0.1 * rng.standard_normal(D)), 1.0
    else:
        col, scale = 5.0 * rng.standard_normal(D), 3.0
    x = (scale * rng.standard_normal((T, N, D)) + col).astype(np.float32)
    if spec.data == "const":
        x[:, :, 2] = 3.3
        x[:, :, 7] = 3.3
        x[:, :, 11] = 0.0
    if spec.enabled is None:
        en = None
    elif isinstance(spec.enabled, list):
        en = np.asarray(spec.enabled, np.int32)
    elif spec.enabled == "zero":
        en = np.zeros(T, np.int32)
    else:
        en = rng.integers(0, N + 1, T).astype(np.int32)
        en[0], en[1] = N, 0                                          # one full graph, one empty graph
    clipped = None if en is None else np.clip(en, 0, N)
    valid = np.ones((T, N, 1), bool) if en is None else (np.arange(N)[None, :] < clipped[:, None])[:, :, None]
    gamma = (rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    beta = rng.standard_normal(D).astype(np.float32)
    mm = (col + 0.3 * rng.standard_normal(D)).astype(np.float32)
    mv = (scale * scale * rng.uniform(0.5, 2.0, D)).astype(np.float32)
    g = rng.standard_normal((T, N, D)).astype(np.float32)
    if spec.act == "relu":
        x = _clear_of_zero(x, valid, gamma, beta, mm, mv, clipped)
    c = dict(spec=spec, x=x, clipped=clipped, gamma=gamma, beta=beta, mm=mm, mv=mv, g=g)
    ref, f32, e32, distance = {}, {}, {}, np.inf
    for phase in (0, 1):
        ref[phase], pre = _results(c, phase, np.float64)
        f32[phase], _ = _results(c, phase, np.float32)
        if valid.any():
            distance = min(distance, float(np.abs(pre)[np.broadcast_to(valid, pre.shape)].min()))
        for q in QUANTITIES[phase]:
            e32[phase, q] = family_bounds.error_figure(getattr(f32[phase], q), getattr(ref[phase], q),
                                                       family_bounds.OVER_REF_OR_ABSOLUTE)
    for a in (x, gamma, beta, mm, mv, g) + tuple(ref[0]) + tuple(ref[1]) + tuple(f32[0]) + tuple(f32[1]):
        a.setflags(write=False)
    return Case(name, spec, T, N, D, spec.off, x, en, clipped, gamma, beta, mm, mv, g, ref, f32, e32, distance)


Facts = namedtuple("Facts", "e32 relu_distance enabled clipped valid_rows")


@functools.lru_cache(maxsize=None)
def facts(name):
    """the small figures of a case (the arrays of build() are held for two cases at a time)"""
    c = build(name)
    rows = c.T * c.N if c.clipped is None else int(c.clipped.sum())
    return Facts(dict(c.e32), c.relu_distance, c.enabled, c.clipped, rows)


def bound(name, phase, q):
    return max(WRITTEN[q], 4.0 * facts(name).e32[phase, q])


def padding(case):
    """[T, N] mask of the padding rows, or None where every row is valid"""
    return None if case.clipped is None else np.arange(case.N)[None, :] >= case.clipped[:, None]
