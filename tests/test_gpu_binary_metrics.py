"""ops.binary_metrics (csrc/cvmetrics.hip) against the numpy statement tests/cv_oracle.binary_sums_all and the scikit-learn answers
recorded in tests/golden/g11_cv.npz.

Required of every case: the eight integers per task are exactly the oracle's; |AP - oracle| <= (G + 2) 2^-52 with G the number
of distinct scores of the task (each term takes three roundings, summing G terms adds G - 1 more, the total is at most 1, and
both sides do this); two runs agree bit for bit.  The quantised scores (2 / 8 / 1000 levels) make tie groups straddle every
wave, thread and chunk boundary of the scan (a chunk is 1024 elements)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cv_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
Z = np.load(os.path.join(ROOT, "tests", "golden", "g11_cv.npz"), allow_pickle=False)
CASES = [str(n) for n in Z["m_names"]]
KEYS = [str(k) for k in Z["m_keys"]]


def run(score, label, mask=None, threshold=0.5, strided=False):
    import torch
    from kgcn_amd import ops
    dev = torch.device("cuda:0")
    s = torch.as_tensor(np.ascontiguousarray(score, np.float32), device=dev)
    if strided:                                                     # a column block of a wider buffer
        wide = torch.full((s.shape[0], s.shape[1] + 3), float("nan"), device=dev)
        wide[:, 1:1 + s.shape[1]] = s
        s = wide[:, 1:1 + s.shape[1]]
        assert not s.is_contiguous()
    lab = torch.as_tensor(np.ascontiguousarray(label, np.float32), device=dev)
    mk = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, np.float32), device=dev)
    return ops.binary_metrics(s, lab, mk, threshold=threshold)


def check(score, label, mask=None, threshold=0.5, strided=False):
    counts, ap = run(score, label, mask, threshold, strided)
    want, want_ap, groups = O.binary_sums_all(score, label, mask, threshold)
    assert counts.dtype == np.int64 and ap.dtype == np.float64
    np.testing.assert_array_equal(counts, want)
    for t in range(len(ap)):
        err = abs(ap[t] - want_ap[t])
        print("task %d: G = %d, |AP - oracle| = %.3e (bound %.3e)" % (t, groups[t], err, (groups[t] + 2) * ULP))
        assert err <= (groups[t] + 2) * ULP, (t, ap[t], want_ap[t])
    again, ap2 = run(score, label, mask, threshold, strided)
    assert again.tobytes() == counts.tobytes() and ap2.tobytes() == ap.tobytes()
    return counts, ap


def quantise(u, levels):
    return u if levels is None else np.round(u * (levels - 1)) / (levels - 1)


@pytest.mark.parametrize("T", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099])
def test_sizes_and_tie_structures(n, T):
    rng = np.random.default_rng(1000 * n + T)
    label = (rng.random((n, T)) < 0.4).astype(np.float32)
    mask = (rng.random((n, T)) < 0.7).astype(np.float32)
    for levels in (2, 8, 1000, None):
        score = quantise(rng.random((n, T)) * 0.7 + 0.3 * label * rng.random((n, T)), levels).astype(np.float32)
        check(score, label)
        check(score, label, mask)


def test_all_scores_equal():
    rng = np.random.default_rng(1)
    label = (rng.random((1500, 2)) < 0.5).astype(np.float32)
    counts, ap = check(np.full((1500, 2), 0.75, np.float32), label)
    assert counts[:, 6].tolist() == [1, 1]
    P = counts[:, 1]
    assert counts[:, 5].tolist() == (P * (1500 - P)).tolist()      # one group: AUC 0.5


def test_signed_zero_ties_and_denormals():
    rng = np.random.default_rng(2)
    n = 300
    score = np.zeros((n, 3), np.float32)
    score[::2, 0] = -0.0
    score[:, 1] = np.where(rng.random(n) < 0.5, -0.0, 0.0) * 1.0
    score[:, 1][rng.random(n) < 0.3] = np.float32(1e-3)
    score[:, 2] = rng.integers(-(1 << 10), 1 << 10, n).astype(np.float32) * np.float32(2.0 ** -149)     # denormals, zero among them
    assert np.signbit(score[:, 0]).any() and not np.signbit(score[:, 0]).all()
    label = (rng.random((n, 3)) < 0.5).astype(np.float32)
    counts, _ = check(score, label, threshold=0.0)
    assert counts[0, 6] == 1                                        # -0.0 and +0.0 are one threshold
    check(score, label, threshold=-0.0)


def test_degenerate_tasks():
    """a task without positives, one without negatives, one fully masked, beside a regular one."""
    rng = np.random.default_rng(3)
    n = 1100
    score = rng.random((n, 4)).astype(np.float32)
    label = (rng.random((n, 4)) < 0.5).astype(np.float32)
    label[:, 0], label[:, 1] = 0.0, 1.0
    mask = np.ones((n, 4), np.float32)
    mask[:, 2] = 0.0
    counts, ap = check(score, label, mask)
    assert counts[0, 1] == 0 and ap[0] == 0.0
    assert counts[1, 1] == counts[1, 0] == n and abs(ap[1] - 1.0) <= (n + 2) * ULP
    assert counts[2].tolist() == [0] * 8 and ap[2] == 0.0
    from kgcn_amd import cv
    assert math.isnan(cv.metrics_from_counts(counts[0], ap[0])["auc"]) and cv.metrics_from_counts(counts[1], ap[1])["ap"] == 1.0
    assert math.isnan(cv.metrics_from_counts(counts[2], ap[2])["auc"])


def test_strided_scores():
    rng = np.random.default_rng(4)
    score = quantise(rng.random((777, 3)), 50).astype(np.float32)
    label = (rng.random((777, 3)) < 0.3).astype(np.float32)
    a = check(score, label, strided=True)
    b = check(score, label)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_scores_raise(bad):
    rng = np.random.default_rng(5)
    score = rng.random((100, 2)).astype(np.float32)
    label = (rng.random((100, 2)) < 0.5).astype(np.float32)
    score[37, 1] = bad
    with pytest.raises(ValueError, match="NaN or infinite"):
        run(score, label)
    mask = np.ones((100, 2), np.float32)
    mask[37, 1] = 0.0                                               # a score that does not count is not looked at
    check(score, label, mask)


@pytest.mark.parametrize("j", range(len(CASES)), ids=CASES)
def test_fixture_cases_reproduce_sklearn(j):
    """AUC to one unit in the last place, AP within the derived bound, the confusion metrics as derived on the host."""
    from kgcn_amd import cv
    y, s = Z["m%d_label" % j], Z["m%d_score" % j]
    want = dict(zip(KEYS, Z["m%d_metrics" % j].tolist()))
    counts, ap = check(s[:, None], y[:, None])
    got = cv.metrics_from_counts(counts[0], ap[0])
    for k in KEYS:
        tol = (counts[0, 6] + 2) * ULP if k == "ap" else ULP if k == "auc" else 4 * ULP
        assert (math.isnan(got[k]) and math.isnan(want[k])) or abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


def test_all_tasks_in_one_call_equal_single_task_calls():
    rng = np.random.default_rng(6)
    score = quantise(rng.random((513, 5)), 8).astype(np.float32)
    label = (rng.random((513, 5)) < 0.5).astype(np.float32)
    counts, ap = run(score, label)
    for t in range(5):
        c1, a1 = run(score[:, t:t + 1], label[:, t:t + 1])
        assert c1[0].tolist() == counts[t].tolist() and a1[0] == ap[t]
