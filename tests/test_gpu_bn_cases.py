"""The GraphBatchNormalization kernels (kgcn_amd/csrc/bn.hip) on the cases of tests/bn_cases.py, in both learning phases, every
result against the fp64 reference of oracle/kgcn_oracle.py -- never against another kernel's output:
  * the apply kernels: bn_apply_cols_kernel<4 / 2 / 1> by width and by the alignment of x, bn_apply_kernel<true / false> beyond
    256 column groups, each past its grid cap, with and without a fused activation;
  * bn_colreduce_kernel<0..3> over one to five column blocks, past BN_BLOCKS at one and at several rows a pass; MODE 3 in
    phase 0, MODE 2 in phase 1 and where x needs no gradient;
  * bn_bwd_dx_kernel (phase 1) past its cap and with no valid row; bn_scale_kernel's clamp of enabled and its count;
  * statistics of data whose mean is 30 standard deviations, constant columns, an empty batch, 2-D input.
The misaligned cases go through ops.graph_bn_stats / ops.graph_bn on a view that starts 1 or 2 floats into its buffer, the others
through layers.GraphBatchNormalization.  Bounds: bn_cases.bound -- the written forms, or four times the float32 restatement's own
error where that is more; one line is printed per comparison (case, phase, quantity, error, bound)."""
import numpy as np
import pytest
import torch

import bn_cases as B
import family_bounds
from test_gpu_parity import act64, dact64, dev, t32  # noqa: F401  (the references of bn_cases are made with act64 / dact64)

pytestmark = pytest.mark.gpu

RUNS = [(name, phase) for name in B.NAMES for phase in (0, 1)]


def up(a):
    """to the device; the cases' arrays are read-only and shared between tests: upload a copy"""
    return t32(np.array(a))


def place(case):
    """x on the device, `off` floats into a 16-byte-aligned buffer: a contiguous [T, N, D] view that keeps its offset"""
    n = case.x.size
    buf = torch.zeros(case.off + n, device=dev())
    assert buf.data_ptr() % 16 == 0
    buf[case.off:].copy_(up(case.x).reshape(-1))
    x = buf[case.off:case.off + n].view(case.T, case.N, case.D)
    assert x.is_contiguous() and x.data_ptr() % 16 == (4 * case.off) % 16
    return x


def run_ops(case, phase, x, en, gamma, beta, mm, mv, g):
    """the misaligned cases: ops.graph_bn_stats / ops.graph_bn on the view itself"""
    from kgcn_amd import ops
    assert x.data_ptr() % 16 in (4, 8) and x.data_ptr() % 16 == (4 * case.off) % 16
    x.requires_grad_(True)
    got = {}
    if phase:
        mean, var = ops.graph_bn_stats(x.detach(), en)
        got["mean"], got["var"] = mean, var
    else:
        mean, var = mm, mv
    y = ops.graph_bn(x, gamma, beta, mean, var, en, B.EPS, bool(phase), case.spec.act)
    y.backward(g)
    got.update(y=y, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return got


def run_layer(case, phase, x, en, gamma, beta, mm, mv, g):
    from kgcn_amd import layers, ops
    spec = case.spec
    layer = layers.GraphBatchNormalization(learning_phase=phase, activation=spec.act)
    layer.build((case.T, case.N, case.D), dev())
    assert (layer.eps, layer.momentum) == (B.EPS, B.MOMENTUM)
    with torch.no_grad():
        layer.gamma.copy_(gamma); layer.beta.copy_(beta)
        layer.moving_mean.copy_(mm); layer.moving_variance.copy_(mv)
    squeeze = len(spec.shape) == 2
    got = {}
    if phase:
        got["mean"], got["var"] = ops.graph_bn_stats(x, en)
    tx = (x[0] if squeeze else x).requires_grad_(spec.with_dx)
    y = layer(tx, enabled_node_nums=en)
    assert y.shape == tx.shape
    y.backward(g[0] if squeeze else g)
    assert (tx.grad is not None) == spec.with_dx
    got.update(y=y.detach().reshape(x.shape), dgamma=layer.gamma.grad, dbeta=layer.beta.grad)
    if spec.with_dx:
        got["dx"] = tx.grad.reshape(x.shape)
    if phase:
        got["mm"], got["mv"] = layer.moving_mean, layer.moving_variance
    else:                                                                # phase 0 leaves the moving statistics alone
        assert torch.equal(layer.moving_mean, mm) and torch.equal(layer.moving_variance, mv)
    return got


@pytest.mark.parametrize("name,phase", RUNS)
def test_graph_bn_case(name, phase):
    case = B.build(name)
    spec, ref = case.spec, case.ref[phase]
    route = B.route(case.D, case.off, case.T * case.N)
    for key, want in spec.expect.items():
        assert route[key] == want, (name, key)
    x = place(case)
    en = None if case.enabled is None else torch.as_tensor(np.array(case.enabled), device=dev())
    gamma, beta, mm, mv, g = (up(a) for a in (case.gamma, case.beta, case.mm, case.mv, case.g))
    if case.off:
        got = run_ops(case, phase, x, en, gamma.requires_grad_(True), beta.requires_grad_(True), mm, mv, g)
    else:
        got = run_layer(case, phase, x, en, gamma, beta, mm, mv, g)
    torch.cuda.synchronize()
    got = {q: v.detach().cpu().numpy() for q, v in got.items()}
    compared = [q for q in B.QUANTITIES[phase] if not (q == "dx" and not spec.with_dx) and not (q in ("mm", "mv") and case.off)]
    assert set(got) == set(compared), (sorted(got), compared)
    misses = []
    for q in compared:
        r = getattr(ref, q)
        assert got[q].shape == r.shape and got[q].dtype == np.float32, (q, got[q].shape, got[q].dtype)
        assert np.isfinite(got[q]).all(), q
        err = family_bounds.error_figure(got[q], r, family_bounds.OVER_REF_OR_ABSOLUTE)
        bound = B.bound(name, phase, q)
        print("BN %s | phase %d | %s | err / max|ref| = %.3e | bound %.3e | %s" % (name, phase, q, err, bound, route["apply"]))
        if not err <= bound:
            misses.append((q, err, bound))
    assert not misses, (name, phase, misses)
    # ---- padding rows: exactly 0, or exactly act(0) in the forward ----
    pad = B.padding(case)
    if pad is not None and pad.any():
        a0 = np.float32(act64(np.float64(0.0), spec.act))
        assert np.all(got["y"][pad] == a0), (name, "forward padding rows")
        if spec.with_dx:
            assert np.all(got["dx"][pad] == 0.0), (name, "backward padding rows")
    if name == "all_empty":
        assert not (got["y"].any() or got["dx"].any() or got["dgamma"].any() or got["dbeta"].any())
        if phase:
            assert not (got["mean"].any() or got["var"].any())
