"""ops.multitask_softmax2_ce (csrc/cvloss.hip) against tests/cv_oracle.softmax2_ce in fp64: costs, predictions and the gradient
within the bounds of tests/golden/cv_bounds.json (ten times the error measured on the MI355X against the oracle, relative to
max(1, max |ref|) per tensor; KGCN_CV_RECORD=<file> writes the errors of a run), counts exact, and the device accumulator."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cv_oracle as O  # noqa: E402
import family_bounds  # noqa: E402

pytestmark = pytest.mark.gpu

FB = family_bounds.FAMILIES["cv"]               # FB.check: max|got - ref| / max(1, max|ref|), held to the stored bound


def run(logits, labels, mask, accum=None, backward=True):
    import torch
    from kgcn_amd import ops
    dev = torch.device("cuda:0")
    x = torch.as_tensor(logits, device=dev).requires_grad_(backward)
    cost, each_cost, each_correct, each_count, pred = ops.multitask_softmax2_ce(
        x, torch.as_tensor(labels, device=dev), torch.as_tensor(mask, device=dev), accum=accum)
    out = {"cost": float(cost.detach()),"each_cost": each_cost.cpu().numpy(), "each_correct": each_correct.cpu().numpy(),
           "each_count": each_count.cpu().numpy(), "prediction": pred.cpu().numpy(), "cost_bits": cost.detach().cpu().numpy().tobytes()}
    if backward:
        cost.backward()
        out["dlogits"] = x.grad.cpu().numpy()
    return out


def compare(logits, labels, mask):
    got = run(logits, labels, mask)
    ref = O.softmax2_ce(logits, labels, mask)
    np.testing.assert_array_equal(got["each_correct"], ref["each_correct"].astype(np.float32))
    np.testing.assert_array_equal(got["each_count"], ref["each_count"].astype(np.float32))
    FB.check("loss_cost", got["cost"], ref["cost"])
    FB.check("loss_each_cost", got["each_cost"], ref["each_cost"])
    FB.check("loss_prediction", got["prediction"], ref["prediction"])
    FB.check("loss_dlogits", got["dlogits"], ref["dlogits"])
    assert np.isfinite(got["dlogits"]).all() and np.isfinite(got["each_cost"]).all()
    return got, ref


def case(rng, B, T, scale=3.0):
    logits = (rng.standard_normal((B, 2, T)) * scale).astype(np.float32)
    labels = (rng.random((B, T)) < 0.5).astype(np.float32)
    mask = (rng.random((B, T)) < 0.7).astype(np.float32)
    return logits, labels, mask


# (2, 257): more tasks than the finish kernel has threads, so its task loop takes a second trip
@pytest.mark.parametrize("B,T", [(B, T) for T in (1, 4, 7) for B in (1, 3, 50, 257)] + [(2, 257)])
def test_against_the_oracle(B, T):
    import torch
    logits, labels, mask = case(np.random.default_rng(100 * B + T), B, T)
    got, _ = compare(logits, labels, mask)
    # the same call twice with an accumulator: its own values unchanged, the block = the float32 sum of the two
    acc = torch.zeros(3 * T + 1, device="cuda:0")
    block = np.concatenate([got["each_cost"], got["each_correct"], got["each_count"], np.frombuffer(got["cost_bits"], np.float32)])
    for _ in range(2):
        again = run(logits, labels, mask, accum=acc, backward=False)
        assert again["cost_bits"] == got["cost_bits"] and again["each_cost"].tobytes() == got["each_cost"].tobytes()
    assert acc.cpu().numpy().tobytes() == (block + block).astype(np.float32).tobytes()


def test_large_logits_stay_finite():
    rng = np.random.default_rng(1)
    logits, labels, mask = case(rng, 50, 4)
    logits[:] = np.where(rng.random(logits.shape) < 0.5, 80.0, -80.0)
    mask[:] = 1.0
    got, ref = compare(logits, labels, mask)
    assert got["cost"] > 160.0                                      # a confident miss costs |z1 - z0| = 160


def test_equal_logits_predict_class_zero():
    rng = np.random.default_rng(2)
    logits, labels, mask = case(rng, 50, 4)
    logits[:, 1, :] = logits[:, 0, :]
    mask[:] = 1.0
    got, _ = compare(logits, labels, mask)
    np.testing.assert_array_equal(got["each_correct"], (labels == 0).sum(axis=0).astype(np.float32))
    np.testing.assert_array_equal(got["prediction"], np.full((50, 4), 0.5, np.float32))


def test_fully_masked_task_is_exactly_zero():
    rng = np.random.default_rng(3)
    logits, labels, mask = case(rng, 257, 4)
    mask[:, 2] = 0.0
    got, _ = compare(logits, labels, mask)
    assert got["each_cost"][2] == 0.0 and got["each_count"][2] == 0.0 and got["each_correct"][2] == 0.0
    assert not got["dlogits"][:, :, 2].any()


def test_zero_padded_tail_rows():
    """the dummy graphs of a short batch: zero logits, labels and mask_label rows add nothing."""
    rng = np.random.default_rng(4)
    logits, labels, mask = case(rng, 50, 4)
    logits[37:], labels[37:], mask[37:] = 0.0, 0.0, 0.0
    got, _ = compare(logits, labels, mask)
    head = run(logits[:37], labels[:37], mask[:37])
    np.testing.assert_array_equal(got["each_count"], head["each_count"])
    np.testing.assert_array_equal(got["each_correct"], head["each_correct"])
    assert not got["dlogits"][37:].any()
    FB.check("loss_each_cost", got["each_cost"], head["each_cost"].astype(np.float64))


def test_flat_logits_are_the_same_call():
    rng = np.random.default_rng(5)
    logits, labels, mask = case(rng, 50, 4)
    a = run(logits, labels, mask)
    b = run(logits.reshape(50, 8), labels, mask)
    assert a["cost_bits"] == b["cost_bits"] and a["dlogits"].tobytes() == b["dlogits"].tobytes()


def test_accumulator_is_the_fixed_order_sum_of_single_calls():
    """k calls with accum= leave the float32 sums of the k single calls' blocks, added in call order, bit for bit."""
    import torch
    rng = np.random.default_rng(6)
    T, k = 4, 7
    acc = torch.zeros(3 * T + 1, device="cuda:0")
    want = np.zeros(3 * T + 1, np.float32)
    for i in range(k):
        logits, labels, mask = case(rng, 50 if i % 2 else 33, T)
        single = run(logits, labels, mask, backward=False)
        block = np.concatenate([single["each_cost"], single["each_correct"], single["each_count"],
                                np.frombuffer(single["cost_bits"], np.float32)])
        want = (want + block).astype(np.float32)
        again = run(logits, labels, mask, accum=acc, backward=False)
        assert again["cost_bits"] == single["cost_bits"]            # the accumulator does not change the call's own values
    assert acc.cpu().numpy().tobytes() == want.tobytes()


def test_shapes_are_checked():
    import torch
    from kgcn_amd import _lib, ops
    dev = torch.device("cuda:0")
    with pytest.raises(_lib.KgcnHipError):
        ops.multitask_softmax2_ce(torch.zeros((4, 3, 2), device=dev), torch.zeros((4, 2), device=dev), torch.zeros((4, 2), device=dev))
    with pytest.raises(_lib.KgcnHipError):
        ops.multitask_softmax2_ce(torch.zeros((4, 2, 2), device=dev), torch.zeros((4, 2), device=dev), torch.zeros((4, 2), device=dev),
                                  accum=torch.zeros(6, device=dev))
