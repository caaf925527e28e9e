"""kgcn_amd.cv.train_cv on the stand-in dataset of tests/golden/g11_cv.npz (60 graphs, T = 3) with k = 3, 3 epochs, batch 10:
the folds cover every graph once, the reported metrics are the oracle's metrics of the returned predictions, a second run is
bit-identical, fold 2 equals a fit of fold 2 alone (nothing leaks across folds through the reused captured steps), the
parameters left after a fit are the best epoch's, and training lowers the cost.  One run is shared by the tests."""
import json
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
CONFIG = {"k-fold_num": 3, "epoch": 3, "batch_size": 10, "learning_rate": 1e-3, "patience": 3, "seed": 7}
Z = np.load(os.path.join(ROOT, "tests", "golden", "g11_cv.npz"), allow_pickle=False)
T = 3


def validator(config=None):
    import torch
    from kgcn_amd import cv, data_util as D, models
    dev = torch.device("cuda:0")
    channels, _ = D.build_adjs({"dense_adj": Z["ds_dense_adj"], "max_node_num": int(Z["ds_max_node_num"])})
    ds = D.DeviceGraphDataset(channels, Z["ds_feature"], device=dev)
    cfg = dict(CONFIG)
    cfg.update(config or {})
    return cv.CrossValidator(lambda: models.CPIMultitaskNet(len(channels), T), ds, Z["ds_label"], Z["ds_mask_label"], cfg)


_shared = {}


def shared_run():
    if not _shared:
        v = validator()
        out = v.run()
        _shared.update(v=v, out=out, pred=[p.cpu().numpy() for p in out["predictions"]])
    return _shared


def test_every_graph_is_in_exactly_one_test_fold():
    out = shared_run()["out"]
    seen = np.concatenate([np.asarray(i["test_data_idx"]) for i in out["info_cv"]])
    assert sorted(seen.tolist()) == list(range(60))
    for (tr, te), info in zip(out["folds"], out["info_cv"]):
        assert info["test_data_idx"] == te.tolist() and not set(tr.tolist()) & set(te.tolist())
    assert len(out["result_cv"]) == 3 and all(len(fold) == T for fold in out["result_cv"])


@pytest.mark.parametrize("masked", [False, True])
def test_reported_metrics_are_the_oracles_of_the_predictions(masked):
    s = shared_run() if not masked else None
    if masked:
        v = validator({"metrics_mask": True, "epoch": 1})
        out = v.run()
        pred = [p.cpu().numpy() for p in out["predictions"]]
    else:
        out, pred = s["out"], s["pred"]
    for f, (info, p) in enumerate(zip(out["info_cv"], pred)):
        idx = np.asarray(info["test_data_idx"])
        assert p.shape == (len(idx), T) and np.isfinite(p).all() and (p > 0).all() and (p < 1).all()
        want, want_ap, groups = O.binary_sums_all(p, Z["ds_label"][idx], Z["ds_mask_label"][idx] if masked else None)
        assert info["counts"] == want.tolist()
        for t in range(T):
            assert abs(info["ap"][t] - want_ap[t]) <= (groups[t] + 2) * ULP
            ref = O.metrics(want[t], info["ap"][t])
            got = out["result_cv"][f][t]
            for k in O.METRIC_KEYS:
                assert (math.isnan(got[k]) and math.isnan(ref[k])) or got[k] == ref[k], (f, t, k)


def test_second_run_is_bit_identical():
    s = shared_run()
    again = validator().run()
    for a, b in zip(s["pred"], again["predictions"]):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    for a, b in zip(s["out"]["info_cv"], again["info_cv"]):
        for k in ("training_cost", "validation_cost", "training_acc", "validation_acc", "test_cost", "counts", "ap", "best_epoch"):
            assert a[k] == b[k], k
    # ... and so is a second pass through the SAME captured steps
    third = s["v"].run()
    for a, b in zip(s["pred"], third["predictions"]):
        assert a.tobytes() == b.cpu().numpy().tobytes()


def test_fold_two_alone_equals_fold_two_of_the_run():
    """the in-place re-initialisation and the Adam reset are complete: fold 2 after fold 1 == fold 2 on fresh captures."""
    s = shared_run()
    v = validator()
    train_valid, test = s["out"]["folds"][1]
    metrics, info, pred = v.run_fold(2, train_valid, test)
    assert pred.cpu().numpy().tobytes() == s["pred"][1].tobytes()
    ref = s["out"]["info_cv"][1]
    assert info["training_cost"] == ref["training_cost"] and info["validation_cost"] == ref["validation_cost"]
    assert info["counts"] == ref["counts"] and info["ap"] == ref["ap"]
    assert json.dumps(metrics) == json.dumps(s["out"]["result_cv"][1])


def test_best_epoch_parameters_are_restored():
    """with the validation cost forced to worsen after epoch 1, the fit leaves epoch 1's parameters, not the last epoch's."""
    import torch
    v = validator({"epoch": 4, "patience": 0})
    snaps = []

    def forced(epoch, cost):
        torch.cuda.synchronize()
        snaps.append(v.flat.data.detach().clone())
        return [5.0, 1.0, 2.0, 3.0][epoch]

    out = v.fit(np.arange(0, 40), np.arange(40, 50), seed=3, validation_cost_fn=forced)
    assert len(snaps) == 4 and out["best_epoch"] == 1
    assert torch.equal(v.flat.data, snaps[1]) and not torch.equal(v.flat.data, snaps[3]) and not torch.equal(snaps[0], snaps[1])
    # the parameters of the model are views of the buffer: the model itself computes with the restored values
    for p, view in zip(v.model.parameters(), v.flat.views):
        assert p.data_ptr() == view.data_ptr()
    # with patience 2 the third epoch (two rises in a row) stops the fit, and epoch 1 is still what is restored
    v2 = validator({"epoch": 4, "patience": 2})
    out2 = v2.fit(np.arange(0, 40), np.arange(40, 50), seed=3, validation_cost_fn=lambda e, c: [5.0, 1.0, 2.0, 3.0][e])
    assert len(out2["training_cost"]) == 4 and out2["best_epoch"] == 1
    assert torch.equal(v2.flat.data, snaps[1])


def test_training_lowers_the_cost():
    for info in shared_run()["out"]["info_cv"]:
        assert len(info["training_cost"]) == 3
        assert info["training_cost"][-1] < info["training_cost"][0]


def test_stratified_kfold_is_refused():
    with pytest.raises(NotImplementedError, match="stratified"):
        validator({"stratified_kfold": True})


def test_cv_json_is_written(tmp_path):
    from kgcn_amd import cv
    s = shared_run()
    path = str(tmp_path / "cv.json")
    cv.save_result_cv(s["out"]["result_cv"], path)
    back = json.load(open(path))
    assert len(back) == 3 and len(back[0]) == T and set(back[0][0]) == set(O.METRIC_KEYS) | {"sup"}
    rows = cv.auc_table(back)
    assert [r[0] for r in rows] == [0, 1, 2]
