"""Two helpers of csrc/misc.hip as operations: kgcn_dot_f32 (the dot product behind d eps of GINAggregate) and
kgcn_copy2d_multi_f32 (several strided 2-D copies in one launch; until now run only inside ops._CatChannels).

kgcn_dot_f32: dot_partial_kernel has a float4 path (both operands 16-byte aligned: a 4x-unrolled loop, its remainder loop, a scalar
tail of n % 4 elements) and a scalar path (anything else); at most 1024 workgroups, i.e. 262,144 threads.  The exact cases use
integer operands in -2 ... 2: every product and every partial sum is then an integer far below 2^24, float32 carries it
exactly, and the result must EQUAL the integer dot product -- a dropped, doubled or misplaced element cannot hide inside a
rounding bound.
  dot_final_kernel adds at most 1024 partials with 256 threads, so `i + 7 * 256 < nparts` never holds and its 8x-unrolled loop is
  not reachable through kgcn_dot_f32 (it serves the fused d eps kernels, which hand it one partial per graph); the sizes below run
  its remainder loop at 1, 2, 4 and 1024 partials.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import record_accuracy  # noqa: E402

pytestmark = pytest.mark.gpu

DOT_THREADS = 1024 * 256
DOT_SIZES = (0, 1, 3, 4, 5, 255, 256, 257,
             DOT_THREADS * 4 + 4,                           # one float4 each and ONE thread a second: the remainder loop alone
             DOT_THREADS * 16 + DOT_THREADS * 4 + 7)        # one unrolled trip, one remainder trip (one float4 over: a second for
                                                            # thread 0) and a scalar tail of 3


def dev():
    return torch.device("cuda:0")


def _dot(a, b, n):
    from kgcn_amd._lib import lib, ptr, check, current_stream
    wsb = int(lib.kgcn_dot_workspace_bytes(n))
    ws = torch.full((wsb // 4,), 7.0, device=dev())
    out = torch.full((1,), -55.5, device=dev())
    check(lib.kgcn_dot_f32(ptr(a), ptr(b), n, ptr(out), ptr(ws), wsb, current_stream()), "kgcn_dot_f32")
    return out


def _operands(a, b, shift):
    """-> device copies; shift = 1: both are views one float into their storage (not 16-byte aligned: the scalar path)."""
    out = []
    for h in (a, b):
        store = torch.zeros(h.shape[0] + shift, device=dev())
        store[shift:] = torch.from_numpy(h).to(dev())
        out.append(store[shift:])
        assert h.shape[0] == 0 or out[-1].data_ptr() % 16 == 4 * shift          # (an empty tensor has no address)
    return out


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_of_small_integers_is_exact(n, shift):
    rng = np.random.default_rng(n + 17 * shift)
    a = rng.integers(-2, 3, n).astype(np.float32)
    b = rng.integers(-2, 3, n).astype(np.float32)
    want = int(np.dot(a.astype(np.int64), b.astype(np.int64)))
    assert abs(want) < 2 ** 24
    da, db = _operands(a, b, shift)
    got = _dot(da, db, n)
    assert float(got) == float(want), (n, shift, float(got), want)
    if n:                                                        # one more element at the far end must count: no lane stops early
        da[n - 1] += 1.0
        assert float(_dot(da, db, n)) == float(want + int(b[n - 1])), (n, shift, "last element")


def test_dot_of_nothing_is_zero_without_operands():
    from kgcn_amd._lib import lib, ptr, current_stream
    out = torch.full((1,), -55.5, device=dev())
    assert lib.kgcn_dot_f32(None, None, 0, ptr(out), None, 0, current_stream()) == 0
    assert float(out) == 0.0
    assert lib.kgcn_dot_f32(None, None, 4, ptr(out), None, 0, current_stream()) != 0
    assert lib.kgcn_dot_f32(ptr(out), ptr(out), 1, ptr(out), ptr(out), 4, current_stream()) != 0      # workspace too small
    assert lib.kgcn_dot_f32(ptr(out), ptr(out), -1, ptr(out), None, 0, current_stream()) != 0


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
def test_dot_of_a_million_normal_values(shift):
    """n = 1,000,003 N(0, 1) values against fp64.  1024 workgroups: a thread adds at most one float4 term (three products summed,
    then one addition) or four scalar terms; the wave adds 6 levels, the workgroup 2, dot_final_kernel 4 + 6 + 2 -- the longest
    chain of dependent additions is under 64, each off by at most 2^-24 of a partial sum that |a_i b_i| bounds: error <=
    64 * 2^-24 * sum |a_i b_i| = 3.8e-6 of that sum.  Measured on an MI355X: 2.5e-10 of it (the roundings of a million random
    terms cancel; the exact cases above are what catches a misplaced element)."""
    n = 1_000_003
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)
    da, db = _operands(a, b, shift)
    got = float(_dot(da, db, n))
    tol = 64 * 2.0 ** -24 * float(np.abs(prod).sum())
    record_accuracy("dot 1,000,003", abs(got - float(prod.sum())), tol, float(np.abs(prod).sum()))
    assert abs(got - float(prod.sum())) <= tol, (got, float(prod.sum()), tol)


# ---- kgcn_copy2d_multi_f32 -----------------------------------------------------------------------------------------------------
COPY_SHAPES = ((0, 5), (5, 0), (1, 1), (7, 1), (3, 50), (300, 257))
SENTINEL = -4242.25


def _jobs(count, seed, first=0, pad_all=False):
    """count jobs over COPY_SHAPES in turn, from shape `first` on; the leading dimensions equal cols or exceed it: the source's by 3
    in jobs 6-11, 18-23, ..., the destination's by 5 in jobs 12-23, 36-47, ... (all four combinations from 24 jobs on; pad_all: both,
    in every job) -> (ctypes job array, [(src, dst, rows, cols, src_ld, dst_ld)]).  Half of the empty jobs carry NULL pointers."""
    from kgcn_amd import _lib
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    arr, held = (_lib.Copy2dJob * count)(), []
    for i in range(count):
        rows, cols = COPY_SHAPES[(first + i) % len(COPY_SHAPES)]
        src_ld = cols + (3 if pad_all or (i // 6) % 2 else 0)
        dst_ld = cols + (5 if pad_all or (i // 12) % 2 else 0)
        src = torch.randn(rows * src_ld + 2, device=dev(), generator=g)
        dst = torch.full((rows * dst_ld + 2,), SENTINEL, device=dev())
        null = rows * cols == 0 and i % 2 == 1
        arr[i] = _lib.Copy2dJob(0 if null else src.data_ptr(), 0 if null else dst.data_ptr(), rows, cols, src_ld, dst_ld)
        held.append((src, dst, rows, cols, src_ld, dst_ld))
    return arr, held


@pytest.mark.parametrize("count", [1, 16, 17, 40])
def test_copy2d_multi_copies_each_block_and_nothing_else(count):
    """1, 16, 17 and 40 jobs (KGCN_COPY2D_MAX_JOBS = 16: one launch, a full launch, two and three launches), among them jobs
    without rows, without columns (some with NULL pointers), of one column, with leading dimensions wider than cols: every
    job's block equals its source bit for bit and every other float of every destination still holds the sentinel."""
    from kgcn_amd._lib import lib, check, current_stream
    # the one job: the large shape, both leading dimensions padded
    arr, held = _jobs(1, 1, first=5, pad_all=True) if count == 1 else _jobs(count, count)
    check(lib.kgcn_copy2d_multi_f32(ctypes.cast(arr, ctypes.c_void_p), count, current_stream()), "kgcn_copy2d_multi_f32")
    torch.cuda.synchronize()
    for i, (src, dst, rows, cols, src_ld, dst_ld) in enumerate(held):
        want = torch.full_like(dst, SENTINEL)
        if rows * cols:
            want[:rows * dst_ld].view(rows, dst_ld)[:, :cols] = src[:rows * src_ld].view(rows, src_ld)[:, :cols]
        assert torch.equal(dst.view(torch.int32), want.view(torch.int32)), (count, i, rows, cols, src_ld, dst_ld)


def test_copy2d_multi_writes_column_blocks_of_one_wide_buffer():
    """The use ops._CatChannels makes of it: 17 sources of 1 ... 17 columns side by side in one [9, total + gaps] buffer, a one-float gap
    after each block; the gaps keep the sentinel."""
    from kgcn_amd import _lib
    from kgcn_amd._lib import lib, check, current_stream
    rows, widths = 9, list(range(1, 18))
    total = sum(widths) + len(widths)
    wide = torch.full((rows, total), SENTINEL, device=dev())
    want = wide.clone()
    arr, srcs, col = (_lib.Copy2dJob * len(widths))(), [], 0
    for i, w in enumerate(widths):
        src = torch.randn(rows, w, device=dev())
        srcs.append(src)
        arr[i] = _lib.Copy2dJob(src.data_ptr(), wide.data_ptr() + 4 * col, rows, w, w, total)
        want[:, col:col + w] = src
        col += w + 1
    check(lib.kgcn_copy2d_multi_f32(ctypes.cast(arr, ctypes.c_void_p), len(widths), current_stream()), "kgcn_copy2d_multi_f32")
    assert torch.equal(wide.view(torch.int32), want.view(torch.int32))


def test_copy2d_multi_refuses_a_narrow_destination_before_any_copy():
    """dst_ld < cols in job 17 of 20 -- behind the first launch's 16 jobs: non-zero return, the job named, and NO destination
    written, not even those of the sixteen good jobs in front of it."""
    from kgcn_amd._lib import lib, current_stream
    arr, held = _jobs(20, 3)
    assert arr[17].cols == 257 and arr[17].rows == 300
    arr[17].dst_ld = arr[17].cols - 1
    rc = lib.kgcn_copy2d_multi_f32(ctypes.cast(arr, ctypes.c_void_p), 20, current_stream())
    assert rc != 0 and b"job 17" in lib.kgcn_last_error()
    torch.cuda.synchronize()
    for i, (src, dst, *_) in enumerate(held):
        assert bool((dst == SENTINEL).all()), i
    assert lib.kgcn_copy2d_multi_f32(None, 3, current_stream()) != 0
    assert lib.kgcn_copy2d_multi_f32(None, 0, current_stream()) == 0
