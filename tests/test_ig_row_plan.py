"""CPU tests of the host protocol the compound attribution drivers share (kgcn_amd.visualization): the row plan is exactly what
ig_scales and smooth_rows return, and the parameter freeze gives every parameter its own flag back."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.parametrize("D", [1, 2, 7])
def test_row_plan_is_ig_scales_and_smooth_rows(D):
    from kgcn_amd import visualization as V
    for method in V.IG_METHODS:
        plan = V.ig_row_plan(method, D)
        scales, weights = V.ig_scales(method, D)
        assert (plan.scales, plan.weights) == (scales, weights) and plan.noise is None and plan.method == method
        assert plan.start_row == 0 and plan.end_row == len(scales) - 1
    for method in V.SMOOTH_METHODS:
        plan = V.ig_row_plan(method, D, noise_scale=0.3, seed=77.0)
        scales, sigmas, samples, weights, start_row, end_row = V.smooth_rows(method, D, 0.3)
        assert (plan.scales, plan.weights, plan.start_row, plan.end_row) == (scales, weights, start_row, end_row)
        assert plan.noise == (sigmas, samples, 77) and type(plan.noise[2]) is int and plan.method == method
        # the one-copy plan of a per-step loop: copy r alone, its score both the start and the end
        for r in range(len(scales)):
            row = V.ig_plan_row(plan, r)
            assert row == V.IGRowPlan([scales[r]], [weights[r]], ([sigmas[r]], [samples[r]], 77), method, 0, 0)
    assert V.ig_plan_row(V.ig_row_plan("ig", D), D) == V.IGRowPlan([1.0], [1.0 / D], None, "ig", 0, 0)


def test_row_plan_refusals():
    from kgcn_amd import visualization as V
    with pytest.raises(ValueError, match="unsupported method"):
        V.ig_row_plan("saliency", 3)
    for method in ("ig",) + V.SMOOTH_METHODS:                # grad_prod and grad take no divide_number
        with pytest.raises(ValueError):
            V.ig_row_plan(method, 0)
    for method in V.SMOOTH_METHODS:                          # the clean methods draw no noise
        with pytest.raises(ValueError):
            V.ig_row_plan(method, 3, noise_scale=-0.1)


def test_frozen_parameters_restores_every_flag_after_an_exception():
    from kgcn_amd import visualization as V
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    flags = [True, False, False, True]
    for p, f in zip(model.parameters(), flags):
        p.requires_grad_(f)
    with pytest.raises(RuntimeError, match="inside"):
        with V.frozen_parameters(model):
            assert not any(p.requires_grad for p in model.parameters())
            raise RuntimeError("inside")
    assert [p.requires_grad for p in model.parameters()] == flags
    with V.frozen_parameters(model):
        assert not any(p.requires_grad for p in model.parameters())
    assert [p.requires_grad for p in model.parameters()] == flags
