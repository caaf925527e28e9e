"""The three forms of the TF-Adam update of csrc/train.hip -- adam_tf_kernel<true> (float4), adam_tf_kernel<false> (scalar: n % 4 != 0
or a buffer that is not 16-byte aligned) and adam_tf_multi_kernel (per-segment gradients) -- held to the promise of the comment
above adam_tf_update that all of them round identically, and to the fp64 update of tests/step_tail_oracle.tf_adam.

Which gap of the suite each test closes:
  adam_tf_kernel<false>                          test_three_forms_agree_bit_for_bit: the call on views one float into their storage at
                                                 every n, and the aligned call at every n % 4 != 0
  the grid-stride tails of the packed forms      n = 256*8*256 + 257 (scalar, second trip of 257 elements) and 4 * 256*8*256 + 1028
                                                 (float4, second trip of 257 float4s; five trips of the scalar form, seventeen of the
                                                 per-segment form)
  a step counter that does not start at 0        counter = 1, 999 and 100,000 (beta1^t underflows: lr_t = lr sqrt(1 - beta2^t))
  more segments than one launch takes, empty segments, a refused segment list
                                                 33 segments; test_adam_multi_refuses_a_bad_segment_before_any_update
  train.TFAdam.step() against step(packed=True)  test_tfadam_step_and_packed_step_give_equal_bytes

Measured on an MI355X against fp64 (largest over all sizes, counters and steps): p 3.0e-7 absolute, at most 15 % of its bound;
v 6.4e-8 relative; m at most 42 % of its rounding bound.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_tail_cases as C  # noqa: E402
import step_tail_oracle as R  # noqa: E402
from conftest import record_accuracy  # noqa: E402

pytestmark = pytest.mark.gpu

H = C.ADAM_HYPER


def dev():
    return torch.device("cuda:0")


def _up(a, shift=0):
    """-> a device tensor holding `a`; shift = 1: a view that starts one float into its storage (4 bytes off a 16-byte boundary)."""
    t = torch.from_numpy(a)
    if not shift:
        out = t.to(dev())
        assert out.data_ptr() % 16 == 0
        return out
    store = torch.zeros(a.shape[0] + shift, dtype=t.dtype, device=dev())
    store[shift:] = t.to(dev())
    out = store[shift:]
    assert out.data_ptr() % 16 == 4 * shift
    return out


class _Form:
    """One way of running the update on its own copies of the parameters, the moments and the counter."""

    def __init__(self, name, d, shift=0, segments=None):
        self.name, self.n, self.segments = name, d["n"], segments
        self.p, self.m, self.v = _up(d["p"], shift), _up(d["m"], shift), _up(d["v"], shift)
        self.grads = [_up(g, shift) for g in d["grads"]]
        self.t = torch.full((1,), d["counter"], dtype=torch.int64, device=dev())

    def step(self, k):
        from kgcn_amd import _lib
        from kgcn_amd._lib import lib, ptr, check, current_stream
        g = self.grads[k]
        if self.segments is None:
            check(lib.kgcn_adam_tf_f32(ptr(self.p), ptr(g), ptr(self.m), ptr(self.v), self.n, H["lr"], H["b1"], H["b2"], H["eps"],
                                       ptr(self.t), current_stream()), self.name)
            return
        segs = (_lib.AdamSegment * len(self.segments))()
        for i, (off, length) in enumerate(self.segments):        # an empty segment brings no gradient pointer at all
            segs[i] = _lib.AdamSegment(g.data_ptr() + 4 * off if length else 0, off, length)
        check(lib.kgcn_adam_tf_multi_f32(ptr(self.p), ptr(self.m), ptr(self.v), self.n, ctypes.cast(segs, ctypes.c_void_p),
                                         len(self.segments), H["lr"], H["b1"], H["b2"], H["eps"], ptr(self.t), current_stream()),
              self.name)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _against_fp64(what, got, ref, relative_only=False, tol=None):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    if tol is None:
        tol = C.ADAM_RTOL * np.abs(ref) + (0.0 if relative_only else C.ADAM_ATOL)
    worst = int(np.argmax(err - tol))
    record_accuracy(what, float(err[worst]), float(tol[worst]), float(np.abs(ref[worst])))
    assert np.all(np.isfinite(got)) and err[worst] <= tol[worst], (what, worst, got[worst], ref[worst])


@pytest.mark.parametrize("counter", C.ADAM_COUNTERS)
@pytest.mark.parametrize("n", C.ADAM_SIZES)
def test_three_forms_agree_bit_for_bit(n, counter):
    """kgcn_adam_tf_f32 on aligned buffers (float4 form when n % 4 == 0), the same call on views one float into their storage (scalar
    form), kgcn_adam_tf_multi_f32 over 1, 3 and 33 uneven segments (one of them empty; 33 > KGCN_ADAM_MAX_SEGMENTS = 32 takes two
    launches and ONE tick): equal bytes in the parameters and both moments after each of three steps, the counter advanced by
    exactly three, and after every step against the fp64 update:
      p   within 2e-6 + 2e-6 |ref| (the bound of the 3M-parameter test of test_gpu_large_sizes.py);
      v   within 2e-6 |ref| and NO absolute term: a sum of non-negative terms, nothing cancels (three roundings a step: 9 * 2^-24 =
          5.4e-7 after three), so a second moment of 1e-27 must be right too;
      m   within 2 * 2^-24 * sum_j A_j, A_j = b1 A_(j-1) + (1 - b1) |g_j| (A_0 = |m_0|) the first moment of the gradients' MAGNITUDES.
          Gradients of either sign over sixteen decades make b1 m and (1 - b1) g cancel to a hundredth of their size in about one
          element of 10,000 a step, and what float32 rounded off m before stays (n = 1025, counter 1: -1.35814 came out as
          -1.35816, 1.1e-5 relative, in all three forms alike); no bound on |ref| alone can hold there.  Each step rounds g (1 - b1)
          and the fma once: e_j <= b1 e_(j-1) + 2^-24 ((1 - b1) |g_j| + |m_j|) <= b1 e_(j-1) + 2 * 2^-24 A_j.  Wherever nothing
          cancels (A <= 5 |m|) this is below 2e-6 |ref|, with no absolute term."""
    d = C.adam_case(n, counter)
    forms = [_Form("aligned", d), _Form("one float off", d, shift=1)]
    forms += [_Form("%d segments" % k, d, segments=C.adam_segments(n, k)) for k in C.ADAM_SEGMENT_COUNTS]
    assert any(length == 0 for _, length in forms[-1].segments) and len(forms[-1].segments) == 33
    p, m, v = (d[k].astype(np.float64) for k in ("p", "m", "v"))
    b1, c1 = R.adam_hyper(**H)[1], R.adam_hyper(**H)[4]
    mag, mag_sum = np.abs(m), np.zeros(n)
    for k in range(C.ADAM_STEPS):
        for f in forms:
            f.step(k)
        first = forms[0]
        for f in forms[1:]:
            for name in ("p", "m", "v"):
                assert torch.equal(_bits(getattr(f, name)), _bits(getattr(first, name))), (n, counter, k, f.name, name)
        p, m, v = R.tf_adam(p, d["grads"][k], m, v, counter + 1 + k, **H)
        mag = b1 * mag + c1 * np.abs(d["grads"][k].astype(np.float64))
        mag_sum = mag_sum + mag
        _against_fp64("adam p", first.p, p)
        _against_fp64("adam m", first.m, m, tol=2 * 2.0 ** -24 * mag_sum)
        _against_fp64("adam v", first.v, v, relative_only=True)
    for f in forms:
        assert int(f.t) == counter + C.ADAM_STEPS, (f.name, int(f.t))


def test_adam_multi_refuses_a_bad_segment_before_any_update():
    """A segment that runs past the buffer BEHIND the 32nd (the second launch's share): non-zero return, no parameter, moment or
    counter touched -- not the first 32 segments updated and the step left half done."""
    from kgcn_amd import _lib
    from kgcn_amd._lib import lib, ptr, current_stream
    n, k = 40 * 16, 40
    d = C.adam_case(n, 7)
    f = _Form("bad", d)
    before = [t.clone() for t in (f.p, f.m, f.v, f.t)]
    segs = (_lib.AdamSegment * k)()
    for i in range(k):
        segs[i] = _lib.AdamSegment(f.grads[0].data_ptr() + 64 * i, 16 * i, 16)
    segs[35] = _lib.AdamSegment(f.grads[0].data_ptr(), n - 8, 16)
    rc = lib.kgcn_adam_tf_multi_f32(ptr(f.p), ptr(f.m), ptr(f.v), n, ctypes.cast(segs, ctypes.c_void_p), k, H["lr"], H["b1"], H["b2"],
                                    H["eps"], ptr(f.t), current_stream())
    assert rc != 0 and b"segment 35" in lib.kgcn_last_error()
    torch.cuda.synchronize()
    for a, b in zip(before, (f.p, f.m, f.v, f.t)):
        assert torch.equal(a, b)


def test_tfadam_step_and_packed_step_give_equal_bytes():
    """train.TFAdam over a model-shaped parameter list whose sizes are no multiples of 4 -- (7,), (3, 5), (1,) -- stepped through the
    per-segment form (step(): each parameter's .grad where it lies) and through the packed form (step(packed=True): flat.grad filled
    from the same gradients): equal bytes in the flat parameter buffer and both moments after each of three steps.  The flat
    buffer places every tensor at a multiple of 64 floats, so its total is a multiple of 4 whatever the shapes and the packed call
    always takes the float4 form; the padding between the tensors (zero gradient, zero moments) must come out untouched."""
    from kgcn_amd import train
    shapes = [(7,), (3, 5), (1,)]
    rng = np.random.default_rng(8)
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-6, 2, s)).astype(np.float32) for s in shapes] for _ in range(3)]
    opts = []
    for _ in range(2):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev())) for a in init]
        opts.append(train.TFAdam(params, **dict(lr=H["lr"], beta1=H["b1"], beta2=H["b2"], eps=H["eps"])))
    multi, packed = opts
    assert multi.flat.total % 4 == 0 and multi.flat.total == 3 * train.FlatParameters.ALIGN
    ref = [(a.astype(np.float64), np.zeros(a.shape), np.zeros(a.shape)) for a in init]
    for k in range(3):
        for p, g in zip(multi.params, grads[k]):
            p.grad = torch.from_numpy(g).to(dev())
        multi.step()
        packed.flat.grad.zero_()
        for view, g in zip(packed.flat.grad_views, grads[k]):
            view.copy_(torch.from_numpy(g).to(dev()))
        packed.step(packed=True)
        for a, b in ((multi.flat.data, packed.flat.data), (multi._m, packed._m), (multi._v, packed._v)):
            assert torch.equal(_bits(a), _bits(b)), k
        ref = [R.tf_adam(p, g, m, v, k + 1, **H) for (p, m, v), g in zip(ref, grads[k])]
        for p, (rp, rm, rv) in zip(multi.params, ref):
            _against_fp64("TFAdam p", p.detach().reshape(-1), rp.reshape(-1))
    assert int(multi._t_dev) == int(packed._t_dev) == 3 and multi.t == packed.t == 3
    pad = torch.ones(multi.flat.total, dtype=torch.bool, device=dev())
    for p, o in zip(multi.params, multi.flat.offsets):
        pad[o:o + p.numel()] = False
    for buf in (packed.flat.data, packed._m, packed._v):
        assert bool((buf[pad] == 0).all())
