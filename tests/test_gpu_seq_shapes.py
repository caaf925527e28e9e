"""The sequence-encoder kernels (csrc/seq.hip: conv-pool, LSTM, the integrated-gradients pair) across the shape box declared in
include/kgcn_hip.h, against the fp64 oracles tests/multimodal_oracle.py and tests/multimodal_ig_oracle.py fed the same
fp32-rounded inputs.  Every case checks, for every output and gradient,

  normwise     max |err| / max |ref|  <=  TOL = 1e-5, the family's bound (test_gpu_multimodal.py).  The conv-pool has no
               recurrence: its error grows with the number of routed positions B T' summed into d w / d b / d table, and TOL was
               measured at 717k of them; no case here has more than 71,610, so TOL holds for every conv-pool case whatever its
               T'.  An LSTM run of more than 512 steps gets 4 x the fp32 yardstick below instead.
  elementwise  |err| <= tol (|ref| + m), m the largest |ref| of the element's own row (d table: the symbol; dx, pooled, h: the
               position or sequence), column (d w: the filter; d W_x, d W_h: the gate column) or, for a vector, the vector;
               tol = 4 x the fp32 yardstick of the same figure.  A row whose reference is all zero is exactly zero.
  yardstick    the error against the fp64 oracle of the oracle's own expressions evaluated in fp32 NumPy (dtype=np.float32; the
               conv summed one term at a time as a plain loop does), the largest over N_EVALS = 8 evaluations of the case: as
               given, and with the batch rows, the embedding / input columns and the filters / units permuted, which changes
               nothing but the order of every sum.  One evaluation is one draw of rounding noise and its maximum over a small
               tensor can be far below the typical one; the kernel's figure is held to the largest of eight draws.  The
               yardstick is never below one fp32 eps (1.2e-7): no fp32 result is expected closer to fp64 than a unit in the
               last place, and where all eight evaluations are (single products at E = k = F = 1, a one-step LSTM) that is
               luck.  The lines below and the profile mark with "ulp" every figure whose bound comes from that term.  Nothing
               is taken from what the kernels give, and a derived elementwise bound above 1e-2 fails the case: a yardstick
               that loose measures nothing.
  underflow    rows whose largest |ref| is below 2^-102 (an intermediate 2^-24 smaller leaves the fp32 normal range) are held
               to |err| <= 2^-102 and kept out of the elementwise ratio; the count is printed.  The long LSTM runs are built so
               that there are none: the forget gate stays at 1 (hard sigmoid) or 0.99995 (sigmoid) and the input gate small,
               so h and every gradient depend on all 2,048 / 8,192 steps, and the test asserts on the ORACLE that the dx rows
               of every step are within 1e-4 of the largest.
  structure    (exact) rows of d table of symbols that do not occur are 0.0; every case runs twice, first through the C ABI into
               buffers surrounded by sentinels (outputs, arg-max bytes, stash, workspace), which must all survive, then through
               ops and autograd, bit-identical to the first run.

d pooled is zero at the outputs whose arg-max the oracle itself calls ill-conditioned (two conv values of a window, or the
maximum and 0, closer than 1e-4 of the largest conv value): there fp32 and fp64 may route to different positions and neither
is wrong.  At every other output the kernel's arg-max byte must equal the oracle's.

Measured on an MI355X (profiles/seq_shapes_accuracy.txt has every tensor; here the tensor closest to its bound per case, as
fp32-reference error / bound / kernel error):

  conv B=3 L=130 S=7 E=1 k=1 F=1 p=1 norm d_table 1.3e-07 / 1.0e-05 / 5.1e-08   elem d_table 8.4e-08 / 4.8e-07 / 3.2e-08 ulp
  conv B=5 L=257 S=300 E=32 k=8 F=64 p=8 norm pooled  7.1e-07 / 1.0e-05 / 6.3e-07   elem d_table 1.4e-07 / 5.6e-07 / 1.7e-07
  conv B=5 L=257 S=40 E=32 k=8 F=64 p=8 norm pooled  6.2e-07 / 1.0e-05 / 5.4e-07   elem pooled  4.7e-07 / 1.9e-06 / 4.5e-07
  conv B=2 L=8192 S=1024 E=3 k=5 F=33 p=3 norm pooled  1.6e-07 / 1.0e-05 / 1.4e-07   elem pooled  1.9e-07 / 7.7e-07 / 2.1e-07
  conv B=9 L=100 S=1024 E=32 k=2 F=7 p=5 norm pooled  2.8e-07 / 1.0e-05 / 2.4e-07   elem pooled  3.0e-07 / 1.2e-06 / 2.5e-07
  conv B=4 L=6 S=25 E=25 k=8 F=50 p=2 norm pooled  3.8e-07 / 1.0e-05 / 3.5e-07   elem d_table 1.4e-07 / 5.5e-07 / 2.6e-07
  conv B=4 L=5 S=25 E=25 k=4 F=50 p=8 norm pooled  0.0e+00 / 1.0e-05 / 0.0e+00   elem pooled  0.0e+00 / 4.8e-07 / 0.0e+00 ulp
  conv B=70 L=1023 S=25 E=2 k=7 F=63 p=1 norm d_b     7.1e-06 / 1.0e-05 / 1.5e-07   elem pooled  2.0e-07 / 8.0e-07 / 1.7e-07
  conv B=600 L=264 S=64 E=4 k=3 F=64 p=4 norm pooled  1.9e-07 / 1.0e-05 / 1.6e-07   elem pooled  1.8e-07 / 7.2e-07 / 1.6e-07
  conv B=3 L=68 S=30 E=5 k=4 F=50 p=4 norm pooled  2.2e-07 / 1.0e-05 / 1.7e-07   elem pooled  1.3e-07 / 5.2e-07 / 1.0e-07
  conv B=3 L=93 S=30 E=6 k=6 F=12 p=3 norm pooled  2.0e-07 / 1.0e-05 / 1.4e-07   elem pooled  2.2e-07 / 8.9e-07 / 2.2e-07
  conv B=6 L=200 S=1024 E=8 k=4 F=50 p=4 norm pooled  2.1e-07 / 1.0e-05 / 1.8e-07   elem d_table 1.7e-07 / 6.8e-07 / 1.8e-07
  conv B=7 L=40 S=1024 E=32 k=8 F=1 p=8 norm pooled  4.7e-07 / 1.0e-05 / 4.8e-07   elem d_table 9.2e-08 / 4.8e-07 / 5.1e-08 ulp
  lstm B=1 T=1 D=1 H=1 hard_sigmoid  norm h       1.8e-07 / 1.0e-05 / 5.9e-08   elem d_wx    1.2e-07 / 4.9e-07 / 3.9e-08
  lstm B=1 T=1 D=1 H=1 sigmoid       norm h       4.8e-08 / 1.0e-05 / 4.8e-08   elem d_wx    2.8e-08 / 4.8e-07 / 2.8e-08 ulp
  lstm B=17 T=40 D=64 H=16 hard_sigmoid norm dx      5.2e-07 / 1.0e-05 / 4.3e-07   elem h       4.6e-07 / 1.9e-06 / 4.3e-07
  lstm B=17 T=40 D=64 H=16 sigmoid   norm d_wh    3.1e-07 / 1.0e-05 / 3.0e-07   elem d_wh    6.4e-07 / 2.6e-06 / 6.4e-07
  lstm B=17 T=40 D=64 H=64 hard_sigmoid norm dx      5.3e-07 / 1.0e-05 / 5.8e-07   elem d_wx    8.5e-07 / 3.4e-06 / 9.6e-07
  lstm B=17 T=40 D=64 H=64 sigmoid   norm d_wh    6.0e-07 / 1.0e-05 / 5.1e-07   elem h       3.7e-07 / 1.5e-06 / 4.1e-07
  lstm B=5 T=33 D=1 H=64 hard_sigmoid norm dx      1.7e-07 / 1.0e-05 / 3.9e-07   elem h       1.2e-07 / 4.8e-07 / 2.6e-07 ulp
  lstm B=5 T=33 D=1 H=64 sigmoid     norm dx      4.1e-07 / 1.0e-05 / 3.2e-07   elem h       1.4e-07 / 5.6e-07 / 2.5e-07
  lstm B=33 T=20 D=50 H=17 hard_sigmoid norm d_wx    3.2e-07 / 1.0e-05 / 2.8e-07   elem dx      9.1e-07 / 3.6e-06 / 1.0e-06
  lstm B=33 T=20 D=50 H=17 sigmoid   norm dx      3.4e-07 / 1.0e-05 / 3.6e-07   elem d_bias  1.8e-07 / 7.1e-07 / 2.0e-07
  lstm B=33 T=20 D=3 H=33 hard_sigmoid norm dx      1.8e-07 / 1.0e-05 / 2.7e-07   elem h       3.1e-07 / 1.2e-06 / 3.8e-07
  lstm B=33 T=20 D=3 H=33 sigmoid    norm h       2.7e-07 / 1.0e-05 / 2.7e-07   elem d_wh    6.8e-07 / 2.7e-06 / 7.5e-07
  lstm B=9 T=25 D=7 H=5 hard_sigmoid norm d_wh    3.0e-07 / 1.0e-05 / 2.2e-07   elem d_bias  1.2e-07 / 5.0e-07 / 1.8e-07
  lstm B=9 T=25 D=7 H=5 sigmoid      norm d_wh    2.5e-07 / 1.0e-05 / 2.5e-07   elem d_wh    5.3e-07 / 2.1e-06 / 8.1e-07
  lstm B=4 T=2048 D=50 H=32 hard_sigmoid norm h       8.5e-07 / 3.4e-06 / 8.7e-07   elem h       4.9e-07 / 1.9e-06 / 6.2e-07
  lstm B=4 T=2048 D=50 H=32 sigmoid  norm h       1.1e-06 / 4.5e-06 / 7.2e-07   elem d_wx    9.5e-04 / 3.8e-03 / 9.5e-04
  lstm B=4 T=8192 D=8 H=16 hard_sigmoid norm d_bias  2.9e-04 / 1.2e-03 / 5.0e-05   elem dx      1.4e-03 / 5.8e-03 / 1.4e-03
  lstm B=4 T=8192 D=8 H=16 sigmoid   norm d_wx    2.3e-05 / 9.2e-05 / 2.8e-05   elem d_wh    1.0e-04 / 4.1e-04 / 1.5e-04
  lstm B=6 T=12 D=7 H=8 hard_sigmoid norm d_wh    2.7e-07 / 1.0e-05 / 1.8e-07   elem dx      3.7e-07 / 1.5e-06 / 4.2e-07
  lstm B=6 T=12 D=7 H=8 sigmoid      norm dx      1.5e-07 / 1.0e-05 / 2.3e-07   elem dx      3.2e-07 / 1.3e-06 / 2.5e-07
  lstm B=6 T=12 D=8 H=8 hard_sigmoid norm d_wh    3.7e-07 / 1.0e-05 / 2.7e-07   elem dx      5.7e-07 / 2.3e-06 / 5.4e-07
  lstm B=6 T=12 D=8 H=8 sigmoid      norm d_wh    3.6e-07 / 1.0e-05 / 2.2e-07   elem d_wh    9.0e-07 / 3.6e-06 / 6.1e-07
  lstm B=6 T=12 D=12 H=8 hard_sigmoid norm d_wh    2.6e-07 / 1.0e-05 / 2.8e-07   elem dx      3.5e-07 / 1.4e-06 / 2.9e-07
  lstm B=6 T=12 D=12 H=8 sigmoid     norm d_wx    3.2e-07 / 1.0e-05 / 2.4e-07   elem dx      4.5e-07 / 1.8e-06 / 3.9e-07
  lstm B=15 T=12 D=10 H=9 hard_sigmoid norm d_bias  2.9e-07 / 1.0e-05 / 4.0e-07   elem d_wh    4.4e-07 / 1.8e-06 / 4.0e-07
  lstm B=15 T=12 D=10 H=9 sigmoid    norm d_bias  1.5e-07 / 1.0e-05 / 2.2e-07   elem d_bias  9.1e-08 / 4.8e-07 / 1.8e-07 ulp
  lstm B=17 T=12 D=10 H=9 hard_sigmoid norm h       2.5e-07 / 1.0e-05 / 1.7e-07   elem h       2.2e-07 / 8.8e-07 / 2.4e-07
  lstm B=17 T=12 D=10 H=9 sigmoid    norm h       2.0e-07 / 1.0e-05 / 1.6e-07   elem h       1.9e-07 / 7.8e-07 / 2.2e-07
  lstm B=7 T=12 D=21 H=20 hard_sigmoid norm dx      2.4e-07 / 1.0e-05 / 2.3e-07   elem dx      3.5e-07 / 1.4e-06 / 3.8e-07
  lstm B=7 T=12 D=21 H=20 sigmoid    norm dx      3.1e-07 / 1.0e-05 / 3.7e-07   elem d_wh    5.2e-07 / 2.1e-06 / 7.3e-07
  lstm B=9 T=12 D=21 H=20 hard_sigmoid norm dx      4.5e-07 / 1.0e-05 / 3.8e-07   elem d_wh    4.6e-07 / 1.9e-06 / 4.1e-07
  lstm B=9 T=12 D=21 H=20 sigmoid    norm dx      3.8e-07 / 1.0e-05 / 3.5e-07   elem d_bias  1.2e-07 / 5.0e-07 / 1.5e-07
  lstm B=3 T=12 D=30 H=40 hard_sigmoid norm dx      3.8e-07 / 1.0e-05 / 3.2e-07   elem dx      4.8e-07 / 1.9e-06 / 4.7e-07
  lstm B=3 T=12 D=30 H=40 sigmoid    norm dx      4.5e-07 / 1.0e-05 / 3.3e-07   elem dx      4.0e-07 / 1.6e-06 / 4.0e-07
  lstm B=5 T=12 D=30 H=40 hard_sigmoid norm h       2.1e-07 / 1.0e-05 / 3.1e-07   elem dx      5.7e-07 / 2.3e-06 / 7.5e-07
  lstm B=5 T=12 D=30 H=40 sigmoid    norm dx      4.3e-07 / 1.0e-05 / 3.3e-07   elem dx      5.4e-07 / 2.2e-06 / 7.8e-07
  lstm out= H=64 wide=131 col=50     norm d_wx    4.8e-07 / 1.0e-05 / 6.7e-07   elem d_wh    5.0e-07 / 2.0e-06 / 7.4e-07
  lstm out= H=5 wide=23 col=7        norm d_bias  2.4e-07 / 1.0e-05 / 1.5e-07   elem d_wx    3.0e-07 / 1.2e-06 / 2.7e-07
  lstm out= H=5 wide=5 col=0         norm d_wh    2.5e-07 / 1.0e-05 / 1.6e-07   elem h       3.1e-07 / 1.3e-06 / 2.8e-07
  lstm hard-sigmoid edges            norm d_wx    1.3e-01 / 1.0e-05 / 2.2e-07   elem dx      3.2e-07 / 1.3e-06 / 3.2e-07
  ig k=1 p=1 F=1 E=1 L=45 rep=1      norm pooled  6.2e-08 / 1.0e-05 / 6.2e-08   elem dx_sum  4.5e-08 / 4.8e-07 / 4.5e-08 ulp
  ig k=1 p=1 F=1 E=1 L=45 rep=5      norm dx_sum  5.6e-08 / 1.0e-05 / 5.6e-08   elem dx_sum  8.0e-07 / 3.2e-06 / 2.8e-06
  ig k=8 p=8 F=64 E=32 L=70 rep=1    norm pooled  5.4e-07 / 1.0e-05 / 5.4e-07   elem dx_sum  1.7e-07 / 6.7e-07 / 2.8e-07
  ig k=8 p=8 F=64 E=32 L=70 rep=5    norm pooled  6.7e-07 / 1.0e-05 / 4.9e-07   elem dx_row  1.6e-07 / 6.6e-07 / 3.1e-07
  ig k=5 p=3 F=33 E=3 L=129 rep=1    norm dx_row  1.4e-07 / 1.0e-05 / 2.0e-07   elem dx_row  5.0e-07 / 2.0e-06 / 6.2e-07
  ig k=5 p=3 F=33 E=3 L=129 rep=5    norm dx_row  1.2e-07 / 1.0e-05 / 1.7e-07   elem dx_row  8.0e-07 / 3.2e-06 / 1.7e-06
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_ig_oracle as IG  # noqa: E402
import multimodal_oracle as M  # noqa: E402
from gpu_helpers import to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
F32 = np.float32
EPS = float(np.finfo(np.float32).eps)
REF_FACTOR = 4.0            # the kernel's allowance over the fp32 yardstick: another summation order
N_EVALS = 8                 # fp32 NumPy evaluations per case (the first as given, the others with permuted summation orders)
TINY = 2.0 ** -102          # rows of a reference below this are out of fp32's reach
LOOSE = 1e-2                # a derived elementwise bound above 1 % of an element's own row checks nothing
LONG_RUN = 512              # LSTM steps up to which TOL was measured
K_TILE, K_IG_POS = 16, 32   # kTile, kIgPos of seq.hip
GUARD = 256                 # sentinel elements on either side of a guarded buffer
SENTINEL = 1.2345e30


def _lds_limit():
    src = open(os.path.join(ROOT, "kgcn_amd", "csrc", "kgcn_common.h")).read()
    m = re.search(r"constexpr\s+int\s+kLdsBytes\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", src)
    assert m, "kLdsBytes not found in kgcn_common.h"
    return int(m.group(1)) * int(m.group(2))


def _round4(x):
    return (x + 3) & ~3


def convpool_bwd_lds_bytes(S, E, k, F, p, table_in_lds):
    """convpool_bwd_lds of seq.hip restated: W [k][E][F4p], G [kTile p][F4p], window [nrows][E4], v [nrows][32], the window's
    tokens, and the [S][E] table when it is kept in LDS."""
    nrows, F4p = K_TILE * p + k - 1, _round4(F) + 4
    return 4 * (k * E * F4p + K_TILE * p * F4p + nrows * _round4(E) + nrows * 32 + _round4(nrows) + (S * E if table_in_lds else 0))


# ---- comparison --------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def add(self, name, out, ref, refs32, axis, norm_tol, elementwise=True):
        """refs32: the fp32 NumPy evaluations of this tensor; axis: the axes over which an element's own row / column magnitude
        is taken (None = the whole tensor); elementwise=False: the elementwise figure is printed and not asserted."""
        out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
        refs32 = [np.asarray(r, np.float64) for r in refs32]
        assert all(out.shape == ref.shape == r.shape for r in refs32), (self.tag, name, out.shape, ref.shape)
        err = np.abs(out - ref)
        e32 = np.max([np.abs(r - ref) for r in refs32], axis=0) if ref.size else np.zeros(ref.shape)
        top = max(1e-30, np.abs(ref).max(initial=0.0))
        norm, norm32 = err.max(initial=0.0) / top, e32.max(initial=0.0) / top
        marks = ""
        if norm_tol is None:
            norm_tol = REF_FACTOR * max(norm32, EPS)
            marks += " norm-ulp" if norm32 < EPS else ""
        scale = np.abs(ref).max(axis=axis, keepdims=True) if ref.size else np.zeros(ref.shape)
        den = np.abs(ref) + scale
        tiny = np.broadcast_to((scale > 0) & (scale < TINY), ref.shape)
        pos = (den > 0) & ~tiny
        q = float((err[pos] / den[pos]).max(initial=0.0))
        q32 = float((e32[pos] / den[pos]).max(initial=0.0))
        elem_tol = REF_FACTOR * max(q32, EPS)
        marks += " elem-ulp" if q32 < EPS else ""
        marks += " underflow:%d" % int(tiny.sum()) if tiny.any() else ""
        marks += " elem-not-asserted" if not elementwise else ""
        zero_rows_exact = not np.any(out[den == 0])
        tiny_ok = bool(np.all(err[tiny] <= TINY))
        self.rows.append((name, norm32, norm_tol, norm, q32, elem_tol, q, marks))
        bad = []
        if not norm <= norm_tol:
            bad.append("norm %.2e > %.2e" % (norm, norm_tol))
        if elementwise and not q <= elem_tol:
            bad.append("elem %.2e > %.2e" % (q, elem_tol))
        if elementwise and not elem_tol <= LOOSE:
            bad.append("elementwise bound %.2e measures nothing" % elem_tol)
        if not zero_rows_exact:
            bad.append("non-zero where the reference row is all zero")
        if not tiny_ok:
            bad.append("rows below fp32's reach are not")
        if bad:
            self.bad.append((name,) + tuple(bad))

    def finish(self):
        print()
        for name, n32, nt, n, q32, qt, q, marks in self.rows:
            print("ACC %-34s %-7s norm: fp32-ref %.2e bound %.2e kernel %.2e | elem: fp32-ref %.2e bound %.2e kernel %.2e%s"
                  % (self.tag, name, n32, nt, n, q32, qt, q, marks))
        if self.rows:
            wn = max(self.rows, key=lambda r: r[3] / r[2])
            we = max(self.rows, key=lambda r: r[6] / r[5])
            print("SUMMARY %-34s norm %-7s %.1e / %.1e / %.1e   elem %-7s %.1e / %.1e / %.1e%s"
                  % (self.tag, wn[0], wn[1], wn[2], wn[3], we[0], we[4], we[5], we[6], " ulp" if "elem-ulp" in we[7] else ""))
        assert not self.bad, (self.tag, self.bad)


class Guarded:
    """A contiguous device buffer of n elements inside a larger allocation filled with a sentinel."""

    def __init__(self, n, dtype=None):
        import torch
        self.dtype = dtype or torch.float32
        self.fill = 0xA5 if self.dtype == torch.uint8 else SENTINEL
        self.n = int(n)
        self.big = torch.full((self.n + 2 * GUARD,), self.fill, device="cuda", dtype=self.dtype)
        self.view = self.big[GUARD:GUARD + self.n]

    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.view.data_ptr())

    def intact(self):
        import torch
        edge = torch.full((GUARD,), self.fill, device="cuda", dtype=self.dtype)
        return torch.equal(self.big[:GUARD], edge) and torch.equal(self.big[GUARD + self.n:], edge)

    def same_bits(self, t):
        import torch
        return torch.equal(self.view.view(torch.uint8), t.contiguous().reshape(-1).view(torch.uint8))


# ---- conv-pool -------------------------------------------------------------------------------------------------------------
def _conv_params(rng, S, E, k, F):
    lim = np.sqrt(6.0 / (k * E + k * F))
    return (rng.uniform(-0.5, 0.5, (S, E)).astype(F32), rng.uniform(-lim, lim, (k, E, F)).astype(F32),
            rng.uniform(-0.1, 0.1, F).astype(F32))


def _conv_tokens(rng, B, L, S, kind):
    if kind == "zipf":                      # a few symbols take nearly every position: most of the S rows of d table stay empty
        return np.minimum(rng.zipf(1.3, size=(B, L)) - 1, S - 1).astype(np.int32)
    return rng.integers(0, S, size=(B, L)).astype(np.int32)


def _well_conditioned(conv, T, p):
    """-> (safe, alive, arg) [B, T, F]: outputs whose arg-max and relu decision do not hang on the last bits of the conv."""
    B, L, F = conv.shape
    y = conv[:, :T * p].reshape(B, T, p, F)
    thr = 1e-4 * max(1.0, np.abs(conv).max(initial=0.0))
    srt = np.sort(y, axis=2)
    m1 = srt[:, :, -1]
    gap = m1 - srt[:, :, -2] if p > 1 else np.full(m1.shape, np.inf)
    alive, dead = m1 > thr, m1 < -thr
    return dead | (alive & (gap > thr)), alive, y.argmax(axis=2)


def _conv_fp32_evals(rng, tok, table, w, b, p, gp):
    """N_EVALS fp32 evaluations of (pooled, d table, d w, d b): as given, then with batch rows, embedding columns and filters
    permuted and the results put back -> one list of evaluations per tensor."""
    B, (k, E, F) = tok.shape[0], w.shape
    evals = []
    for i in range(N_EVALS):
        pb, pe, pf = (np.arange(n) if i == 0 else rng.permutation(n) for n in (B, E, F))
        ib, ie, jf = np.argsort(pb), np.argsort(pe), np.argsort(pf)
        tk, tb_, w_, b_ = tok[pb], table[:, pe], w[:, pe][:, :, pf], b[pf]
        pooled = M.conv_pool_fwd(tk, tb_, w_, b_, p, F32)[0]
        dt, dw, db = M.conv_pool_bwd(tk, tb_, w_, b_, p, gp[pb][:, :, pf], F32)
        evals.append((pooled[ib][:, :, jf], dt[:, ie], dw[:, ie][:, :, jf], db[jf]))
    return list(zip(*evals))


CONV_CASES = [  # (B, L, S, E, k, F, p, tokens, route of the backward table)
    (3, 130, 7, 1, 1, 1, 1, "uniform", None),          # all minima
    (5, 257, 300, 32, 8, 64, 8, "uniform", "global"),  # all maxima; the table does not fit LDS: convpool_bwd_kernel<false>
    (5, 257, 40, 32, 8, 64, 8, "uniform", "lds"),      # the same shape with the table in LDS
    (2, 8192, 1024, 3, 5, 33, 3, "uniform", None),     # the longest sequence, E4 and F4p padding
    (9, 100, 1024, 32, 2, 7, 5, "uniform", None),      # 900 tokens over 1,024 symbols
    (4, 6, 25, 25, 8, 50, 2, "uniform", None),         # k > L: every window mostly padding
    (4, 5, 25, 25, 4, 50, 8, "uniform", None),         # p > L: T' = 0
    (70, 1023, 25, 2, 7, 63, 1, "uniform", None),      # p = 1: no pooling
    (600, 264, 64, 4, 3, 64, 4, "uniform", None),      # 3,000 tiles: more than kConvGridFwd and kConvGridBwd
    (3, 68, 30, 5, 4, 50, 4, "uniform", None),         # T' = 17 = kTile + 1
    (3, 93, 30, 6, 6, 12, 3, "uniform", None),         # T' = 31 = 2 kTile - 1
    (6, 200, 1024, 8, 4, 50, 4, "zipf", None),         # skewed tokens: most symbols never occur
    (7, 40, 1024, 32, 8, 1, 8, "zipf", "global"),      # F = 1 on the global-table route
]


@pytest.mark.parametrize("B,L,S,E,k,F,p,kind,route", CONV_CASES)
def test_conv_pool_shape_sweep(B, L, S, E, k, F, p, kind, route):
    import torch
    from kgcn_amd import _lib, ops
    lib, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    tag = "conv B=%d L=%d S=%d E=%d k=%d F=%d p=%d" % (B, L, S, E, k, F, p)
    limit = _lds_limit()
    assert convpool_bwd_lds_bytes(S, E, k, F, p, False) <= limit, "the backward needs more LDS than there is without the table"
    in_lds = convpool_bwd_lds_bytes(S, E, k, F, p, True) <= limit
    if route is not None:                   # the route this case is here for: fails when the formula or the limit moves
        assert in_lds == (route == "lds"), (tag, convpool_bwd_lds_bytes(S, E, k, F, p, True), limit)
    rng = np.random.default_rng([B, L, S, E, k, F, p])
    table, w, b = _conv_params(rng, S, E, k, F)
    tok = _conv_tokens(rng, B, L, S, kind)
    used = np.zeros(S, bool)
    used[tok.reshape(-1)] = True
    if kind == "zipf":
        assert used.sum() < S // 2
    T = L // p
    ref_pooled, _, conv = M.conv_pool_fwd(tok, table, w, b, p)
    safe, alive, ref_arg = _well_conditioned(conv, T, p)
    gp = ((rng.standard_normal((B, T, F)) + 1.0) * safe).astype(F32)       # non-zero mean, as in test_gpu_multimodal.py
    refs = (ref_pooled,) + M.conv_pool_bwd(tok, table, w, b, p, gp)
    refs32 = _conv_fp32_evals(rng, tok, table, w, b, p, gp)

    # first through the C ABI into buffers surrounded by sentinels: a write outside any output, or outside the workspace, shows
    # here before anything runs on plain allocations
    ttok = torch.as_tensor(tok, device="cuda")
    tt, tw, tb, tgp = _t(table), _t(w), _t(b), _t(gp)
    n = B * T * F
    g_out, g_arg = Guarded(n), Guarded(n, torch.uint8)
    g_dt, g_dw, g_db = Guarded(S * E), Guarded(k * E * F), Guarded(F)
    wsb = lib.kgcn_seq_convpool_workspace_bytes(B, L, S, E, k, F, p)
    assert wsb > 0 and wsb % 4 == 0
    g_ws = Guarded(wsb // 4)
    _lib.check(lib.kgcn_seq_convpool_fwd_f32(ptr(ttok), B, L, ptr(tt), S, E, ptr(tw), ptr(tb), k, F, p, g_out.ptr(), g_arg.ptr(),
                                             stream()), "kgcn_seq_convpool_fwd_f32")
    _lib.check(lib.kgcn_seq_convpool_bwd_f32(ptr(ttok), B, L, ptr(tt), S, E, ptr(tw), k, F, p, ptr(tgp), g_arg.ptr(), g_dt.ptr(),
                                             g_dw.ptr(), g_db.ptr(), g_ws.ptr(), wsb, stream()), "kgcn_seq_convpool_bwd_f32")
    torch.cuda.synchronize()
    for name, g in (("pooled", g_out), ("arg-max", g_arg), ("d_table", g_dt), ("d_w", g_dw), ("d_b", g_db), ("workspace", g_ws)):
        assert g.intact(), (tag, name, "wrote outside its buffer")

    # then through ops.seq_conv_pool and autograd: the second launch of both kernels, bit-identical to the first
    tp = [t.clone().requires_grad_(True) for t in (tt, tw, tb)]
    pooled = ops.seq_conv_pool(ttok, tp[0], tp[1], tp[2], p)
    assert tuple(pooled.shape) == (B, T, F)
    pooled.backward(tgp)
    torch.cuda.synchronize()
    outs = (pooled.detach(), tp[0].grad, tp[1].grad, tp[2].grad)
    for name, g, t in (("pooled", g_out, outs[0]), ("d_table", g_dt, outs[1]), ("d_w", g_dw, outs[2]), ("d_b", g_db, outs[3])):
        assert g.same_bits(t), (tag, name, "differs between two launches")

    # arg-max bytes: the oracle's position wherever it is well conditioned, 0xFF where relu is dead, never another value
    arg = g_arg.view.cpu().numpy().reshape(B, T, F)
    assert np.all((arg < p) | (arg == 0xFF))
    assert np.array_equal(arg[safe & alive], ref_arg[safe & alive]) and np.all(arg[safe & ~alive] == 0xFF)
    if p == 1:
        assert np.all((arg == 0) | (arg == 0xFF))

    got_dtab = _np(outs[1])
    assert not np.any(got_dtab[~used]), (tag, "d table rows of symbols that do not occur")
    rep = Report(tag)
    for name, out, ref, ref32, axis in zip(("pooled", "d_table", "d_w", "d_b"), outs, refs, refs32, (-1, 1, (0, 1), None)):
        rep.add(name, _np(out), ref, ref32, axis, TOL)
    rep.finish()
    if T == 0:
        assert not any(np.any(_np(o)) for o in outs[1:])


# ---- LSTM ------------------------------------------------------------------------------------------------------------------
def _lstm_params(rng, D, H):
    wx = rng.uniform(-0.3, 0.3, (D, 4 * H))
    wh = np.linalg.qr(rng.standard_normal((4 * H, H)))[0].T
    bias = np.concatenate([np.zeros(H), np.ones(H), np.zeros(2 * H)]) + rng.uniform(-0.1, 0.1, 4 * H)
    return wx.astype(F32), wh.astype(F32), bias.astype(F32)


def _lstm_params_long(rng, D, H, act):
    """Parameters under which a run of thousands of steps forgets nothing: forget pre-activations in 4 +- 1 (hard sigmoid: f = 1)
    or 10 +- 1 (sigmoid: f = 0.99995), input pre-activations around -2 (i about 0.1) and a small g, so c sums small terms over the run."""
    wx, wh, bias = _lstm_params(rng, D, H)
    for gate, f in ((0, 0.05), (1, 0.15), (2, 0.3)):     # i stays inside its clip, g small: c sums 8,192 terms and stays below 1
        wx[:, gate * H:(gate + 1) * H] *= F32(f)
        wh[:, gate * H:(gate + 1) * H] *= F32(f)
    wh *= F32(0.3)                           # a calm recurrence: fp32 rounding is not amplified step after step
    bias[:H] = F32(-2.0)
    bias[H:2 * H] = F32(4.0 if act == "hard_sigmoid" else 10.0)
    return wx, wh, bias


def _lstm_fp32_evals(rng, x, wx, wh, bias, act, gh):
    """N_EVALS fp32 evaluations of (h, dx, d wx, d wh, d bias): as given, then with sequences, input columns and units permuted."""
    B, T, D = x.shape
    H = wh.shape[0]
    evals = []
    for i in range(N_EVALS):
        pb, pd, pu = (np.arange(n) if i == 0 else rng.permutation(n) for n in (B, D, H))
        ib, id_, iu = np.argsort(pb), np.argsort(pd), np.argsort(pu)
        cols = np.concatenate([g * H + pu for g in range(4)])
        ic = np.argsort(cols)
        h, cache = M.lstm_fwd(x[pb][:, :, pd], wx[pd][:, cols], wh[pu][:, cols], bias[cols], act, F32)
        dx, dwx, dwh, db = M.lstm_bwd(cache, gh[pb][:, pu])
        evals.append((h[ib][:, iu], dx[ib][:, :, id_], dwx[id_][:, ic], dwh[iu][:, ic], db[ic]))
    return list(zip(*evals))


def _lstm_geometry(D, H):
    """lstm_args of seq.hip: (Hp, sequences per workgroup, KA4, whether KA4 / 4 is odd)."""
    Hp = 16 if H <= 16 else (32 if H <= 32 else 64)
    KA4 = _round4(D + H)
    return Hp, 256 // Hp, KA4, (KA4 // 4) & 1


LSTM_CASES = [  # (B, T, D, H)
    (1, 1, 1, 1),          # all minima: Hp = 16, wgrad block 64, D + H + 1 = 3
    (17, 40, 64, 16),      # x staging at exactly 1,024 elements per step
    (17, 40, 64, 64),      # both maxima: D + H + 1 = 129, wgrad block 256
    (5, 33, 1, 64),        # D minimum at full units
    (33, 20, 50, 17),      # padding lanes u >= H at Hp = 32, wgrad block 128
    (33, 20, 3, 33),       # padding lanes at Hp = 64, D + H not a multiple of 4
    (9, 25, 7, 5),         # D + H not a multiple of 4 at Hp = 16
    (4, 2048, 50, 32),     # long run
    (4, 8192, 8, 16),      # longest run
    (6, 12, 7, 8),         # KA4 / 4 = 4 even; D + H + 1 = 16: one whole wgrad k tile
    (6, 12, 8, 8),         # KA4 / 4 = 4 even; D + H + 1 = 17: one element into the second k tile
    (6, 12, 12, 8),        # KA4 / 4 = 5 odd
    (15, 12, 10, 9),       # Hp = 16: one below 16 sequences per workgroup
    (17, 12, 10, 9),       # and one above
    (7, 12, 21, 20),       # Hp = 32: one below 8
    (9, 12, 21, 20),       # and one above
    (3, 12, 30, 40),       # Hp = 64: one below 4
    (5, 12, 30, 40),       # and one above
]


def test_lstm_cases_cover_both_parities_and_every_thread_mapping():
    geo = [_lstm_geometry(D, H) + (B,) for B, T, D, H in LSTM_CASES]
    assert {g[3] for g in geo} == {0, 1}
    for Hp in (16, 32, 64):
        seqs = 256 // Hp
        assert {g[4] % seqs for g in geo if g[0] == Hp} >= {1, seqs - 1}
    assert any(D * _lstm_geometry(D, H)[1] == 1024 for B, T, D, H in LSTM_CASES)


def _run_lstm(x, wx, wh, bias, act, gh, tag, rep, rng, elementwise=True):
    """Forward and backward through the C ABI into guarded buffers, again through ops.seq_lstm, compared with the oracle."""
    import torch
    from kgcn_amd import _lib, ops
    lib, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    B, T, D = x.shape
    H = wh.shape[0]
    norm_tol = TOL if T <= LONG_RUN else None
    ref_h, cache = M.lstm_fwd(x, wx, wh, bias, act)
    refs = (ref_h,) + M.lstm_bwd(cache, gh)
    refs32 = _lstm_fp32_evals(rng, x, wx, wh, bias, act, gh)
    if T > LONG_RUN:                        # on the oracle: the gradient reaches every step of the run
        rows = np.abs(refs[1]).max(axis=(0, 2))
        assert rows.min() >= 1e-4 * rows.max(), (tag, "the long run forgets its first steps", rows.min(), rows.max())
    # first through the C ABI into buffers surrounded by sentinels (the stash and the workspace too), then through ops.seq_lstm
    code = ops.RECURRENT_ACTIVATIONS[act]
    rx, rwx, rwh, rb, tgh = _t(x), _t(wx), _t(wh), _t(bias), _t(gh)
    g_h, g_stash = Guarded(B * H), Guarded(lib.kgcn_seq_lstm_stash_floats(B, T, H))
    g_dx, g_dwx, g_dwh, g_db = Guarded(B * T * D), Guarded(D * 4 * H), Guarded(H * 4 * H), Guarded(4 * H)
    wsb = lib.kgcn_seq_lstm_workspace_bytes(B, T, D, H)
    assert wsb > 0 and wsb % 4 == 0
    g_ws = Guarded(wsb // 4)
    guards = (("h", g_h), ("stash", g_stash), ("dx", g_dx), ("d_wx", g_dwx), ("d_wh", g_dwh), ("d_bias", g_db), ("workspace", g_ws))
    _lib.check(lib.kgcn_seq_lstm_fwd_f32(ptr(rx), B, T, D, ptr(rwx), ptr(rwh), ptr(rb), H, code, g_h.ptr(), H, g_stash.ptr(),
                                         stream()), "kgcn_seq_lstm_fwd_f32")
    torch.cuda.synchronize()
    for name, g in guards:
        assert g.intact(), (tag, name, "the forward wrote outside its buffer")
    _lib.check(lib.kgcn_seq_lstm_bwd_f32(ptr(rx), B, T, D, ptr(rwx), ptr(rwh), ptr(rb), H, code, ptr(tgh), H, g_stash.ptr(),
                                         g_dx.ptr(), g_dwx.ptr(), g_dwh.ptr(), g_db.ptr(), g_ws.ptr(), wsb, stream()),
               "kgcn_seq_lstm_bwd_f32")
    torch.cuda.synchronize()
    for name, g in guards:
        assert g.intact(), (tag, name, "wrote outside its buffer")
    tx, twx, twh, tb = (t.clone().requires_grad_(True) for t in (rx, rwx, rwh, rb))
    h = ops.seq_lstm(tx, twx, twh, tb, act)
    h.backward(tgh)
    torch.cuda.synchronize()
    outs = (h.detach(), tx.grad, twx.grad, twh.grad, tb.grad)
    for name, g, t in zip(("h", "dx", "d_wx", "d_wh", "d_bias"), (g_h, g_dx, g_dwx, g_dwh, g_db), outs):
        assert g.same_bits(t), (tag, name, "differs between two launches")
    for name, out, ref, ref32, axis in zip(("h", "dx", "d_wx", "d_wh", "d_bias"), outs, refs, refs32, (-1, -1, 0, 0, None)):
        rep.add(name, _np(out), ref, ref32, axis, norm_tol, elementwise)
    return outs, refs


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("B,T,D,H", LSTM_CASES)
def test_lstm_shape_sweep(B, T, D, H, act):
    rng = np.random.default_rng([B, T, D, H, len(act)])
    wx, wh, bias = _lstm_params_long(rng, D, H, act) if T > LONG_RUN else _lstm_params(rng, D, H)
    x = rng.standard_normal((B, T, D)).astype(F32)
    gh = rng.standard_normal((B, H)).astype(F32)
    tag = "lstm B=%d T=%d D=%d H=%d %s" % (B, T, D, H, act)
    rep = Report(tag)
    _run_lstm(x, wx, wh, bias, act, gh, tag, rep, rng)
    rep.finish()


@pytest.mark.parametrize("H,wide,col", [(64, 131, 50), (5, 23, 7), (5, 5, 0)])
def test_lstm_output_into_a_column_block(H, wide, col):
    """out= / out_col=: h lands in columns col .. col + H of a wider buffer, every other byte of which stays as it was; the
    values and the gradients are those of the plain call, bit for bit."""
    import torch
    from kgcn_amd import ops
    B, T, D = 11, 9, 13
    rng = np.random.default_rng([H, wide, col])
    wx, wh, bias = _lstm_params(rng, D, H)
    x = rng.standard_normal((B, T, D)).astype(F32)
    gh = rng.standard_normal((B, H)).astype(F32)
    res = []
    for into in (False, True):
        tx, twx, twh, tb = (_t(v).requires_grad_(True) for v in (x, wx, wh, bias))
        g = Guarded(B * wide)
        buf = g.view.view(B, wide)
        buf.fill_(7.0)
        h = ops.seq_lstm(tx, twx, twh, tb, out=buf, out_col=col) if into else ops.seq_lstm(tx, twx, twh, tb)
        h.backward(_t(gh))
        torch.cuda.synchronize()
        if into:
            assert h.data_ptr() == buf.data_ptr() + 4 * col and g.intact()
            bb = buf.cpu().numpy()
            assert np.all(bb[:, :col] == 7.0) and np.all(bb[:, col + H:] == 7.0)
        res.append([h.detach().clone(), tx.grad, twx.grad, twh.grad, tb.grad])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    ref_h, cache = M.lstm_fwd(x, wx, wh, bias)
    refs = (ref_h,) + M.lstm_bwd(cache, gh)
    rep = Report("lstm out= H=%d wide=%d col=%d" % (H, wide, col))
    for name, out, ref, ref32, axis in zip(("h", "dx", "d_wx", "d_wh", "d_bias"), res[1], refs,
                                           _lstm_fp32_evals(rng, x, wx, wh, bias, "hard_sigmoid", gh), (-1, -1, 0, 0, None)):
        rep.add(name, _np(out), ref, ref32, axis, TOL)
    rep.finish()


# ---- the hard-sigmoid clip edges ---------------------------------------------------------------------------------------------
EDGE_KINDS = ("upper", "lower", "above", "below", "under_upper", "over_lower")


def _edge_values():
    up, lo = F32(2.5), F32(-2.5)
    return {"upper": up, "lower": lo, "above": np.nextafter(up, F32(3)), "below": np.nextafter(lo, F32(-3)),
            "under_upper": np.nextafter(up, F32(0)), "over_lower": np.nextafter(lo, F32(0))}


def test_hard_sigmoid_clip_edges_on_the_device():
    """Gate columns whose weights are zero and whose bias is exactly +-2.5, or its float neighbour on either side: z is the bias
    bit for bit.  tf.clip_by_value passes the gradient at y == 0 and y == 1 and nowhere beyond.  The exact assertions on d bias
    and the zero columns and the normwise TOL carry this test.  Its elementwise figures are printed and not asserted: the fp32
    NumPy yardstick rounds y = 1 at the float above 2.5 itself and is off by 1e-1 there, and the gate columns at the float inside
    -2.5 have y = 3e-8, a difference of two numbers near 0.5 that fp32 resolves to a few per cent (elementwise 8e-2)."""
    vals = _edge_values()
    # fp32 (the kernel's forward, __fmul_rn / __fadd_rn) and fp64 (the oracle) put the two edges on the clip values exactly
    for z, y in ((vals["upper"], 1.0), (vals["lower"], 0.0)):
        assert float(F32(0.2) * z + F32(0.5)) == y and 0.2 * float(z) + 0.5 == y
    assert 0.2 * float(vals["above"]) + 0.5 > 1.0 and 0.2 * float(vals["below"]) + 0.5 < 0.0
    B, T, D, H = 9, 7, 6, 24
    rng = np.random.default_rng(11)
    wx, wh, bias = _lstm_params(rng, D, H)
    cols = {}
    for gi, gate in enumerate((0, 1, 3)):                  # the three hard-sigmoid gates i, f, o; one gate of a unit at a time
        for ki, kind in enumerate(EDGE_KINDS):
            n = gate * H + gi * len(EDGE_KINDS) + ki
            wx[:, n], wh[:, n], bias[n] = 0.0, 0.0, vals[kind]
            cols[(gate, kind)] = n
    x = rng.standard_normal((B, T, D)).astype(F32)
    gh = rng.standard_normal((B, H)).astype(F32)
    rep = Report("lstm hard-sigmoid edges")
    outs, refs = _run_lstm(x, wx, wh, bias, "hard_sigmoid", gh, rep.tag, rep, rng, elementwise=False)
    d_bias, ref_bias = _np(outs[4]), refs[4]
    d_wx, d_wh = _np(outs[2]), _np(outs[3])
    for (gate, kind), n in cols.items():
        print("edge gate %d %-11s bias %.9g: d bias kernel %+.6e oracle %+.6e" % (gate, kind, bias[n], d_bias[n], ref_bias[n]))
    for (gate, kind), n in cols.items():
        if kind in ("above", "below"):
            assert ref_bias[n] == 0.0
            assert d_bias[n] == 0.0 and not np.any(d_wx[:, n]) and not np.any(d_wh[:, n]), (gate, kind, d_bias[n])
        else:
            assert ref_bias[n] != 0.0
            assert d_bias[n] != 0.0, (gate, kind)
    rep.finish()


# ---- the integrated-gradients pair ---------------------------------------------------------------------------------------------
IG_CASES = [  # (k, p, F, E, S, L, rep)
    (1, 1, 1, 1, 7, 45, 1),
    (1, 1, 1, 1, 7, 45, 5),
    (8, 8, 64, 32, 300, 70, 1),
    (8, 8, 64, 32, 300, 70, 5),
    (5, 3, 33, 3, 30, 129, 1),
    (5, 3, 33, 3, 30, 129, 5),
]


@pytest.mark.parametrize("k,p,F,E,S,L,rep", IG_CASES)
def test_ig_kernels_shape_sweep(k, p, F, E, S, L, rep):
    import torch
    from kgcn_amd import _lib, ops
    lib, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    assert L % K_IG_POS
    C = 3
    Bc = C * rep
    T = L // p
    tag = "ig k=%d p=%d F=%d E=%d L=%d rep=%d" % (k, p, F, E, L, rep)
    rng = np.random.default_rng([k, p, F, E, S, L, rep])
    table, w, b = _conv_params(rng, S, E, k, F)
    b = np.abs(b) if F == 1 else b                         # the single filter is alive at scale 0 too
    tok = _conv_tokens(rng, C, L, S, "uniform")
    scale = np.tile(np.array([1.0] if rep == 1 else [0.0, 0.25, 0.5, 1.0, 0.8], F32), C)
    ttok = torch.as_tensor(tok, device="cuda")
    tt, tw, tb, ts = _t(table), _t(w), _t(b), _t(scale)
    pooled, arg = ops.seq_conv_pool_scaled(ttok, tt, tw, tb, p, ts, rep, argmax=True)
    emb = table[np.repeat(tok, rep, 0)].astype(np.float64) * scale.astype(np.float64)[:, None, None]
    emb32 = table[np.repeat(tok, rep, 0)] * scale[:, None, None]                    # the fp32 product the kernel forms
    ref_pooled, _, conv = IG.conv_pool_fwd_emb(emb, w, b, p)
    safe, alive, ref_arg = _well_conditioned(conv, T, p)
    a = arg.cpu().numpy()
    assert np.array_equal(a[safe & alive], ref_arg[safe & alive]) and np.all(a[safe & ~alive] == 0xFF)
    # scale 1, one copy: bit for bit the training-path kernel
    one, _ = ops.seq_conv_pool_scaled(ttok, tt, tw, tb, p, torch.ones(C, device="cuda"), 1)
    assert torch.equal(one, ops.seq_conv_pool(ttok, tt, tw, tb, p))

    g = (rng.standard_normal((Bc, T, F)) * safe).astype(F32)
    wt = rng.uniform(0.1, 1.0, Bc).astype(F32)
    if rep > 1:
        wt[::rep] = 0.0
    tg, twt = _t(g), _t(wt)
    per_row = ops.seq_conv_pool_input_grad(tg, arg, ttok.repeat_interleave(rep, 0), tt, tw, p, 1)
    summed = ops.seq_conv_pool_input_grad(tg, arg, ttok, tt, tw, p, rep, row_weight=twt)
    attr = ops.seq_conv_pool_input_grad(tg, arg, ttok, tt, tw, p, rep, row_weight=twt, times_table=True)
    torch.cuda.synchronize()

    def refs_in(dtype, pe=np.arange(E), pf=np.arange(F)):
        """in dtype, the embedding columns and the filters in the given order; results in the original order"""
        ie, jf = np.argsort(pe), np.argsort(pf)
        e = (emb if dtype is np.float64 else emb32)[:, :, pe]
        w_ = w[:, pe][:, :, pf]
        pl, ag, cv = IG.conv_pool_fwd_emb(e, w_, b[pf], p, dtype)
        rows = IG.conv_pool_input_grad(cv, ref_arg[:, :, pf], w_, p, g[:, :, pf], dtype)[:, :, ie]   # routed by the fp64 oracle
        sm = (rows * wt.astype(dtype)[:, None, None]).reshape(C, rep, L, E).sum(1, dtype=dtype)
        return pl[:, :, jf], rows, sm, sm * table[tok].astype(dtype)

    evals = [refs_in(F32)] + [refs_in(F32, rng.permutation(E), rng.permutation(F)) for _ in range(N_EVALS - 1)]

    r = Report(tag)
    for name, out, ref, ref32 in zip(("pooled", "dx_row", "dx_sum", "dx_attr"), (pooled, per_row, summed, attr), refs_in(np.float64),
                                     zip(*evals)):
        r.add(name, _np(out), ref, ref32, -1, TOL)

    # the same launches through the C ABI into guarded buffers
    n = Bc * T * F
    g_out, g_arg, g_dx = Guarded(n), Guarded(n, torch.uint8), Guarded(C * L * E)
    _lib.check(lib.kgcn_seq_convpool_scaled_fwd_f32(ptr(ttok), Bc, rep, ptr(ts), L, ptr(tt), S, E, ptr(tw), ptr(tb), k, F, p, g_out.ptr(),
                                                    g_arg.ptr(), stream()), "kgcn_seq_convpool_scaled_fwd_f32")
    _lib.check(lib.kgcn_seq_convpool_input_grad_f32(ptr(ttok), Bc, rep, L, ptr(tt), S, E, ptr(tw), k, F, p, ptr(tg), g_arg.ptr(), ptr(twt),
                                                    1, g_dx.ptr(), stream()), "kgcn_seq_convpool_input_grad_f32")
    torch.cuda.synchronize()
    assert g_out.intact() and g_arg.intact() and g_dx.intact(), (tag, "wrote outside its buffer")
    assert g_out.same_bits(pooled) and g_arg.same_bits(arg) and g_dx.same_bits(attr), (tag, "differs between two launches")
    r.finish()
