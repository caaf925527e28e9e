"""Host side of the cross-validation workflow (kgcn_amd/cv.py) against tests/golden/g11_cv.npz, where
tests/golden/make_golden_cv.py recorded scikit-learn's KFold splits and every metric of gcn.py's compute_metrics: the fold and
hold-out splits, the metrics derived from the integer sums (the numpy statement in tests/cv_oracle.py and cv.metrics_from_counts
alike), early stopping and the layout of cv.json.  No GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cv_oracle as O  # noqa: E402

from kgcn_amd import cv  # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "g11_cv.npz"), allow_pickle=False)
CASES = [str(n) for n in Z["m_names"]]
KEYS = [str(k) for k in Z["m_keys"]]
ULP = 2.0 ** -52


def ap_bound(groups):
    """|AP - reference| <= (G + 2) 2^-52 for G distinct scores: three roundings per term, G - 1 additions, a total of at most 1,
    on either side."""
    return (groups + 2) * ULP


@pytest.mark.parametrize("i", range(int(Z["kf_cases"])))
def test_kfold_indices_are_sklearns(i):
    n, k, s = (int(v) for v in Z["kf%d_nks" % i])
    folds = cv.kfold_indices(n, k, shuffle=bool(s), seed=123)
    assert len(folds) == k
    for f, (tr, te) in enumerate(folds):
        np.testing.assert_array_equal(te, Z["kf%d_test%d" % (i, f)])
        np.testing.assert_array_equal(tr, Z["kf%d_train%d" % (i, f)])
    assert sorted(np.concatenate([te for _, te in folds]).tolist()) == list(range(n))


def test_kfold_refusals():
    with pytest.raises(NotImplementedError, match="stratified"):
        cv.kfold_indices(10, 5, stratified=True)
    with pytest.raises(ValueError):
        cv.kfold_indices(10, 1)
    with pytest.raises(ValueError):
        cv.kfold_indices(3, 5)


def test_holdout_split_is_split_data():
    num, seed = (int(v) for v in Z["ho_args"])
    tr, va = cv.holdout_split(num, float(Z["ho_rate"]), np.random.RandomState(seed))
    np.testing.assert_array_equal(tr, Z["ho_train"])
    np.testing.assert_array_equal(va, Z["ho_valid"])
    assert len(va) == int(num * float(Z["ho_rate"])) and sorted(np.r_[tr, va].tolist()) == list(range(num))


def same(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


@pytest.mark.parametrize("j", range(len(CASES)), ids=CASES)
@pytest.mark.parametrize("derive", [O.metrics, cv.metrics_from_counts], ids=["oracle", "cv"])
def test_metrics_reproduce_sklearn(j, derive):
    """Every metric of compute_metrics from the integer sums: AUC and the confusion metrics to one unit in the last place of 1,
    AP within the derived bound; NaN where scikit-learn answers NaN, 0 where it answers a zero division with 0."""
    y, s = Z["m%d_label" % j], Z["m%d_score" % j]
    want = dict(zip(KEYS, Z["m%d_metrics" % j].tolist()))
    counts, ap, groups = O.binary_sums(s, y)
    assert counts[0] == len(y) and counts[1] == int(y.sum()) and counts[4] == 0 and counts[6] == groups
    assert groups == len(np.unique(s.astype(np.float64) + 0.0))
    got = derive(counts, ap)
    assert got["sup"] is None
    for k in KEYS:
        # the others: at most four roundings of a value <= 1 on either side
        tol = ap_bound(groups) if k == "ap" else ULP if k == "auc" else 4 * ULP
        assert same(got[k], want[k], tol), (CASES[j], k, got[k], want[k])


def test_degenerate_cases_are_in_the_fixture():
    want = {n: dict(zip(KEYS, Z["m%d_metrics" % j].tolist())) for j, n in enumerate(CASES)}
    assert math.isnan(want["no_positives"]["auc"]) and want["no_positives"]["ap"] == 0.0
    assert math.isnan(want["no_negatives"]["auc"]) and want["no_negatives"]["ap"] == 1.0
    assert want["no_predicted_positives"]["pre"] == 0.0 and want["no_predicted_positives"]["f"] == 0.0
    assert want["all_equal"]["auc"] == 0.5 and want["signed_zero"]["auc"] == want["signed_zero"]["auc"]


def test_masked_sums_are_the_sums_of_the_kept_rows():
    y, s = Z["m0_label"], Z["m0_score"]
    keep = np.arange(len(y)) % 3 != 0
    assert O.binary_sums(s, y, keep) == O.binary_sums(s[keep], y[keep])
    c, ap, g = O.binary_sums_all(np.stack([s, s], 1), np.stack([y, 1 - y], 1), np.stack([keep, ~keep], 1))
    assert c.shape == (2, 8) and c[0].tolist() == O.binary_sums(s[keep], y[keep])[0]
    assert c[1].tolist() == O.binary_sums(s[~keep], 1 - y[~keep])[0]


def test_nonfinite_scores_are_counted():
    s = np.array([0.1, np.nan, np.inf, 0.3], np.float32)
    assert O.binary_sums(s, [0, 1, 1, 0])[0][4] == 2


def test_early_stopping_follows_the_reference():
    """kgcn/core.py:15-32 on hand-made sequences: a rise over the PREVIOUS epoch counts, a fall or a tie resets the count, the
    patience-th rise in a row stops."""
    def stops_at(costs, patience):
        e = cv.EarlyStopping(patience)
        for i, c in enumerate(costs):
            if e.evaluate_validation(c):
                return i
        return None

    assert stops_at([5, 4, 3, 2, 1], 3) is None
    assert stops_at([1, 2, 3, 4, 5], 3) == 3
    assert stops_at([1, 2, 3, 2.5, 3, 4, 5], 3) == 6               # the fall at index 3 resets the count
    assert stops_at([1, 2, 2, 3, 4, 5], 3) == 5                    # a tie is no rise
    assert stops_at([1, 2, 3, 4, 5, 6], 0) is None                 # patience 0 never stops
    assert stops_at([1, 2], 1) == 1
    e = cv.EarlyStopping(2)
    assert [e.evaluate_validation(c) for c in (3.0, 4.0)] == [False, False] and e.validation_count == 1
    assert e.prev_validation_cost == 4.0                           # the previous cost moves on while the fit continues


def test_cv_json_layout(tmp_path):
    """cv.json is a list over folds of a list over tasks of the metric dicts (gcn.py:492-500), NaN and `sup` included."""
    folds = []
    for f in range(3):
        tasks = []
        for j in (0, 4):                                            # a regular case and the one without positives
            counts, ap, _ = O.binary_sums(Z["m%d_score" % j], Z["m%d_label" % j])
            tasks.append(cv.metrics_from_counts(counts, ap))
        folds.append(tasks)
    path = str(tmp_path / "out" / "cv.json")
    cv.save_result_cv(folds, path)
    back = json.load(open(path))
    assert len(back) == 3 and all(len(t) == 2 for t in back)
    assert set(back[0][0]) == set(KEYS) | {"sup"} and back[0][0]["sup"] is None
    assert back[1][0]["auc"] == folds[1][0]["auc"] and math.isnan(back[2][1]["auc"])
    rows = cv.auc_table(back)
    assert rows[0][0] == 0 and abs(rows[0][1] - folds[0][0]["auc"]) < 1e-15 and rows[0][2] == 0.0 and math.isnan(rows[1][1])


def test_default_config_is_the_samples_config_mt():
    assert cv.DEFAULT_CONFIG["batch_size"] == 50 and cv.DEFAULT_CONFIG["k-fold_num"] == 5 and cv.DEFAULT_CONFIG["patience"] == 3
    assert cv.DEFAULT_CONFIG["learning_rate"] == 1e-3 and cv.DEFAULT_CONFIG["validation_data_rate"] == 0.2


def test_fixture_dataset_shape():
    assert Z["ds_dense_adj"].shape == (60, 10, 10) and Z["ds_feature"].shape == (60, 10, 8) and Z["ds_label"].shape == (60, 3)
    m = Z["ds_mask_label"]
    assert m[0].sum() == 0 and 0.2 < 1.0 - m.mean() < 0.4
