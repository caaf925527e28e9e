"""CPU checks of the vector-modality / regression work: the fp64 oracle tests/vecmodal_oracle.py against central differences, the
loader (data_util.vector_table / vector_modal_info) against the feeds the reference emits for the stand-in dataset
(tests/golden/g12_vecmodal.npz), cv.regression_metrics_from_sums against the stored scikit-learn answers, and the new entry points'
argument validation (no launch happens: every refusal comes before one)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vecmodal_oracle as O  # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "g12_vecmodal.npz"), allow_pickle=False)


def _f64(tree):
    if isinstance(tree, dict):
        return {k: _f64(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_f64(v) for v in tree]
    return np.asarray(tree, np.float64)


def _directional(loss_of, P, G, rng, h=1e-6):
    """central difference of loss_of along one random direction over ALL trainable leaves vs the analytic sum(grad * direction)"""
    leaves = O.flatten(P)
    grads = dict(O.flatten(G))
    dirs = {path: rng.standard_normal(a.shape) for path, a in leaves}
    # a direction of unit length over the tens of thousands of leaves: one element moves by ~1e-8, so that hardly any relu
    # changes side inside the step (each one that does costs O(h) of the difference quotient)
    norm = np.sqrt(sum(float((d * d).sum()) for d in dirs.values()))
    dirs = {path: d / norm for path, d in dirs.items()}
    analytic = sum(float((grads[path] * dirs[path]).sum()) for path, _ in leaves)
    saved = {path: a.copy() for path, a in leaves}

    def at(step):
        for path, a in leaves:
            a[...] = saved[path] + step * dirs[path]
        return loss_of()

    numeric = (at(h) - at(-h)) / (2 * h)
    at(0.0)
    return analytic, numeric


@pytest.mark.parametrize("act", [None, "relu", "tanh", "sigmoid"])
@pytest.mark.parametrize("bn", [True, False])
def test_oracle_layer_gradients_against_central_differences(act, bn):
    rng = np.random.default_rng(3)
    B, K, N = 7, 5, 6
    p = _f64(O.draw_dense_bn(rng, K, N, batch_norm=bn))
    x, dy = rng.standard_normal((B, K)), rng.standard_normal((B, N))
    g = O.dense_bn_bwd(x, p, dy, act)
    h = 1e-6
    for name in ("x", "w", "b") + (("gamma", "beta") if bn else ()):
        target = x if name == "x" else p[name]
        num = np.zeros_like(target)
        it = np.nditer(target, flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            keep = target[i]
            target[i] = keep + h
            up = float((O.dense_bn_fwd(x, p, act) * dy).sum())
            target[i] = keep - h
            dn = float((O.dense_bn_fwd(x, p, act) * dy).sum())
            target[i] = keep
            num[i] = (up - dn) / (2 * h)
        assert np.abs(num - g[name]).max() <= 1e-7 * max(1.0, np.abs(g[name]).max()), (name, act, bn)


def _fixture_batch(tag):
    idx = Z["feed_%s_idx" % tag]
    B = int(Z["feed_batch_size"])
    feat = np.zeros((B,) + Z["ds_feature"].shape[1:], np.float64)
    adj = np.zeros((B,) + Z["ds_dense_adj"].shape[1:], np.float64)
    feat[:len(idx)], adj[:len(idx)] = Z["ds_feature"][idx], Z["ds_dense_adj"][idx]
    return idx, feat, adj


@pytest.mark.parametrize("tag", ["full", "short"])
def test_oracle_model_gradients_against_central_differences(tag):
    rng = np.random.default_rng(5)
    idx, feat, adj = _fixture_batch(tag)
    P = _f64(O.draw_vec_model(rng, feat.shape[2], 70))
    labels = Z["feed_%s_labels_classification" % tag].astype(np.float64)
    mask, vec = Z["feed_%s_mask" % tag], Z["feed_%s_profeat" % tag]
    _, _, G = O.vec_model(feat, adj, vec, P, labels, mask)
    a, n = _directional(lambda: O.vec_model(feat, adj, vec, P, labels, mask)[1][0], P, G, rng)
    assert abs(a - n) <= 1e-7 * max(1.0, abs(a)), (a, n)
    R = _f64(O.draw_regression_model(rng, feat.shape[2], 37))
    sizes, y, ml = Z["feed_%s_enabled_node_nums" % tag], Z["feed_%s_labels_regression" % tag], Z["feed_%s_mask_label" % tag]
    vec = Z["feed_%s_dragon" % tag]
    _, L, G = O.regression_model(feat, sizes, vec, R, y, ml)
    a, n = _directional(lambda: O.regression_model(feat, sizes, vec, R, y, ml)[1]["cost_opt"], R, G, rng)
    assert abs(a - n) <= 1e-7 * max(1.0, abs(a)), (a, n)
    assert L["count"].tolist() == ml.sum(axis=0).tolist()


def test_loader_serves_what_the_reference_feeds():
    from kgcn_amd import data_util as D
    data = {"profeat": Z["ds_profeat"], "dragon": Z["ds_dragon"], "feature": Z["ds_feature"]}
    names, dims = D.vector_modal_info(data)
    assert names == dict(zip(Z["info_vector_modal_names"].tolist(), Z["info_vector_modal_pos"].tolist()))
    assert dims == Z["info_vector_modal_dim"].tolist()
    B = int(Z["feed_batch_size"])
    for name in ("profeat", "dragon"):
        table = D.vector_table(data, name, device="cpu")
        assert table.dtype.is_floating_point and table.element_size() == 4 and tuple(table.shape) == (120, dims[names[name]])
        for tag in ("full", "short"):
            idx = Z["feed_%s_idx" % tag]
            want = Z["feed_%s_%s" % (tag, name)]
            got = D.batch_features(table.numpy(), idx, B, device="cpu").numpy()
            assert want.dtype == np.float32 and got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert D.vector_table(data, None, device="cpu").shape[1] == 70            # the first modality the loader's order finds
    with pytest.raises(ValueError):
        D.vector_table({"feature": Z["ds_feature"]}, None, device="cpu")
    with pytest.raises(ValueError):
        D.vector_table(data, "chemical_fp", device="cpu")
    # labels: float32 under task regression, int32 otherwise (kgcn/feed.py:141-146)
    assert Z["feed_full_labels_regression"].dtype == np.float32 and Z["feed_full_labels_classification"].dtype == np.int32
    idx = Z["feed_short_idx"]
    want = np.zeros((B, 2), np.float32)
    want[:len(idx)] = Z["ds_label_reg"][idx]
    assert want.tobytes() == Z["feed_short_labels_regression"].tobytes()


def _same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * max(1.0, abs(b))


def test_regression_metrics_from_sums_against_scikit_learn():
    from kgcn_amd import cv
    names = Z["r_names"].tolist()
    assert {"constant_target_perfect", "constant_target_off", "single_row", "negative_ratio", "masked_subset"} <= set(names)
    for j, name in enumerate(names):
        mask = Z["r%d_mask" % j][:, None] if "r%d_mask" % j in Z.files else None
        sums = O.regression_sums(Z["r%d_pred" % j][:, None], Z["r%d_label" % j][:, None], mask)
        got = cv.regression_metrics_from_sums(sums[0])
        assert sorted(got) == ["gmfe", "mse", "r2"]
        for key, want in zip(Z["r_keys"].tolist(), Z["r%d_metrics" % j]):
            assert _same(got[key], float(want), 1e-12), (name, key, got[key], float(want))
    assert np.isnan(cv.regression_metrics_from_sums([0, 0, 0, 0, 0, 0])["mse"])
    assert cv.auc_table([[{"r2": 0.5, "mse": 1.0, "gmfe": 1.0}], [{"r2": 0.7, "mse": 1.0, "gmfe": 1.0}]], key="r2")[0][1] == pytest.approx(0.6)


def test_unknown_task_is_refused_before_anything_runs():
    from kgcn_amd import cv
    assert cv.DEFAULT_CONFIG["task"] == "classification" and cv.TASKS == ("classification", "regression")
    with pytest.raises(ValueError, match="task"):
        cv.CrossValidator(None, None, None, None, {"task": "regression_gmfe"})


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from kgcn_amd import _lib, ops
    L = _lib.lib
    one = 4096                                                     # any non-NULL address: a refusal comes before any launch
    assert ops.dense_bn_short_supported(1, 1, 1) and ops.dense_bn_short_supported(128, 4096, 512)
    for rows, k, n in ((0, 8, 8), (257, 8, 8), (8, 0, 8), (8, 8193, 8), (8, 8, 0), (8, 8, 1025)):
        assert not ops.dense_bn_short_supported(rows, k, n)
        assert L.kgcn_dense_bn_short_fwd_f32(one, k, rows, k, one, one, n, None, None, None, None, 1e-3, 0, one, n, None, None) != 0
        assert b"outside" in L.kgcn_last_error()
        assert L.kgcn_dense_bn_short_bwd_f32(one, k, rows, k, n, one, n, one, n, None, None, None, None, 1e-3, 0, one, one, None, None,
                                             None, None) != 0
        assert L.kgcn_dense_bn_short_dx_f32(one, rows, n, one, k, one, k, None) != 0
    fwd = lambda **kw: L.kgcn_dense_bn_short_fwd_f32(*[kw.get(a, d) for a, d in (
        ("x", one), ("x_ld", 8), ("rows", 4), ("k", 8), ("w", one), ("bias", one), ("n", 8), ("gamma", None), ("beta", None),
        ("mean", None), ("var", None), ("eps", 1e-3), ("act", 0), ("y", one), ("y_ld", 8), ("pre", None), ("stream", None))])
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(x_ld=7), dict(y_ld=7), dict(act=4), dict(act=-1), dict(gamma=one),
                dict(beta=one), dict(gamma=one, beta=one, mean=one, var=one, eps=0.0)):
        assert fwd(**bad) != 0 and L.kgcn_last_error(), bad
    bwd = lambda **kw: L.kgcn_dense_bn_short_bwd_f32(*[kw.get(a, d) for a, d in (
        ("x", one), ("x_ld", 8), ("rows", 4), ("k", 8), ("n", 8), ("y", one), ("y_ld", 8), ("dy", one), ("dy_ld", 8), ("pre", None),
        ("gamma", None), ("mean", None), ("var", None), ("eps", 1e-3), ("act", 0), ("dw", one), ("dbias", one), ("dgamma", None),
        ("dbeta", None), ("dpre", None), ("stream", None))])
    for bad in (dict(y=None), dict(dy=None), dict(x=None), dict(dy_ld=7), dict(y_ld=7), dict(x_ld=7), dict(gamma=one), dict(dgamma=one),
                dict(dw=None, dbias=None), dict(act=9)):
        assert bwd(**bad) != 0 and L.kgcn_last_error(), bad
    assert L.kgcn_dense_bn_short_dx_f32(None, 4, 8, one, 8, one, 8, None) != 0
    assert L.kgcn_dense_bn_short_dx_f32(one, 4, 8, one, 8, one, 7, None) != 0
    assert L.kgcn_act_cols_fwd_f32(None, 8, 4, 8, 3, one, 8, None) != 0 and L.kgcn_act_cols_fwd_f32(one, 7, 4, 8, 3, one, 8, None) != 0
    assert L.kgcn_act_cols_fwd_f32(one, 8, 0, 8, 3, one, 8, None) != 0 and L.kgcn_act_cols_fwd_f32(one, 8, 4, 8, 7, one, 8, None) != 0
    assert L.kgcn_act_cols_bwd_f32(one, 8, None, 8, 4, 8, 3, one, 8, None) != 0
    assert L.kgcn_act_cols_bwd_f32(one, 8, one, 8, 4, 8, 3, one, 7, None) != 0
    sq = lambda pred=one, labels=one, ml=one, b=4, t=2, d=one, st=one: L.kgcn_masked_sqerr_f32(pred, labels, ml, b, t, d, st, None, None)
    for bad in (dict(pred=None), dict(labels=None), dict(ml=None), dict(d=None), dict(st=None), dict(b=0), dict(b=(1 << 24) + 1),
                dict(t=0), dict(t=65536)):
        assert sq(**bad) != 0 and b"kgcn_masked_sqerr_f32" in L.kgcn_last_error(), bad
    rs = lambda p=one, pl=3, y=one, yl=3, n=5, t=3, out=one: L.kgcn_regression_sums_f64(p, pl, y, yl, None, n, t, out, None)
    for bad in (dict(p=None), dict(y=None), dict(out=None), dict(pl=2), dict(yl=2), dict(n=0), dict(t=0)):
        assert rs(**bad) != 0 and b"kgcn_regression_sums_f64" in L.kgcn_last_error(), bad
