"""csrc/vecig.hip, ops.ig_copies_expand / ig_copies_reduce and visualization.vecmodal_integrated_gradients against the fp64 oracle
of tests/vecmodal_ig_oracle.py (the two sweeps for the ops, the literal loop of kgcn/visualization.py:187-260 for the public
function).

Compounds: the first five of tests/golden/g12_vecmodal.npz (4, 12, 7, 9 and 8 nodes of N = 12: the smallest and a full one),
profeat 70 wide for models.MultimodalVecGCN, dragon 37 wide for models.MultimodalRegressionGCN (with its node counts), D = 8,
parameters drawn by vecmodal_oracle with the seeds tests/test_vecmodal_ig_oracle.py clears of near-zero relu units.  For the smooth
methods the oracle receives the device's own noise, read back by perturbing with scale 0 and sigma 1.

Bound: 1e-5 of max|oracle| per output array (the family's bound: test_gpu_cpi_ig.py, test_gpu_kg_ig.py), ratcheted to ten times
the error measured on the MI355X (tests/golden/vecmodal_ig_bounds.json; never below one fp32 ulp, 2^-23; never above 1e-5).
KGCN_VECMODAL_IG_RECORD=<file> writes the errors of a run."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_bounds  # noqa: E402
import vecmodal_ig_oracle as IO  # noqa: E402
from gpu_helpers import load_dense_bn, set_param, to_device as t  # noqa: E402

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(ROOT, "tests", "golden", "g12_vecmodal.npz"), allow_pickle=False)
# FB.check: equal shapes, finite values, a reference that is not all zero; then max|got - ref| / max|oracle| (big=: over the given
# magnitude instead) under `key`, held to min(1e-5, max(2^-23, stored))
FB = family_bounds.FAMILIES["vecmodal_ig"]
ACTS = (None, "relu", "tanh", "sigmoid")
G = len(IO.COMPOUNDS)
D = IO.DIVIDE


# ---- the kernels against the oracle's sweeps ------------------------------------------------------------------------------------------
def _layer(rng, H, bn):
    p = {"b": (0.3 * rng.standard_normal(H)).astype(np.float32)}
    if bn:
        p.update(gamma=(1.0 + 0.2 * rng.standard_normal(H)).astype(np.float32), beta=(0.1 * rng.standard_normal(H)).astype(np.float32),
                 mean=(0.3 * rng.standard_normal(H)).astype(np.float32), var=(0.5 + rng.random(H)).astype(np.float32))
    return p


def _constants(p, H):
    if "gamma" not in p:
        return np.ones(H), np.zeros(H)
    scale = p["gamma"].astype(np.float64) / np.sqrt(p["var"].astype(np.float64) + 1e-3)
    return scale, p["beta"] - scale * p["mean"]


def _bn_kw(p):
    return {} if "gamma" not in p else dict(gamma=t(p["gamma"]), beta=t(p["beta"]), moving_mean=t(p["mean"]), moving_variance=t(p["var"]))


def _alpha(K):
    return np.linspace(0.0, 1.0, K).astype(np.float32)               # contains 0 (the start copy) and 1


def _weights(rng, K):
    w = (rng.random(K) + 0.1).astype(np.float32)
    w[0] = 0.0
    if K > 4:
        w[K // 2] = 0.0
    return w


def _expand(Pm, alpha, p, act, wide):
    """-> (Y [C K, H] as numpy, the tensor); wide: Y is the block at column 3 of a [C K, H + 3] buffer"""
    from kgcn_amd import ops
    C, H = Pm.shape
    K = len(alpha)
    if not wide:
        y = ops.ig_copies_expand(t(Pm), alpha, t(p["b"]), activation=act, **_bn_kw(p))
        assert y.stride(0) == H
    else:
        before = np.full((C * K, H + 3), 7.25, np.float32)
        buf = t(before)
        y = ops.ig_copies_expand(t(Pm), alpha, t(p["b"]), activation=act, out=buf, out_col=3, **_bn_kw(p))
        assert y.data_ptr() == buf.data_ptr() + 12 and y.stride(0) == H + 3
        assert np.array_equal(buf.cpu().numpy()[:, :3], before[:, :3]), "columns outside the block were written"
    assert tuple(y.shape) == (C * K, H)
    return y.cpu().numpy(), y


def _strided(a):
    """the [rows, H] array as the block at column 3 of a [rows, H + 3] device buffer filled with NaN"""
    buf = torch.full((a.shape[0], a.shape[1] + 3), float("nan"), device="cuda")
    buf[:, 3:] = t(a)
    return buf[:, 3:]


@pytest.mark.parametrize("H", [1, 8, 63, 64, 65, 300])
def test_kernels_against_the_sweeps(H):
    from kgcn_amd import ops
    rng = np.random.default_rng(1000 + H)
    for C in (1, 5):
        for K in (2, 9, 10):
            Pm = rng.standard_normal((C, H)).astype(np.float32)
            alpha, w = _alpha(K), _weights(rng, K)
            for act in ACTS:
                for bn in (True, False):
                    p = _layer(rng, H, bn)
                    scale, shift = _constants(p, H)
                    tag = "C=%d K=%d H=%d %s%s" % (C, K, H, act, " bn" if bn else "")
                    ref_y = IO.expand(Pm, alpha, p["b"], scale, shift, act)
                    y, _ = _expand(Pm, alpha, p, act, wide=False)
                    yw, _ = _expand(Pm, alpha, p, act, wide=True)
                    if np.abs(ref_y).max() > 0:
                        FB.check("op expand", y, ref_y, tag)
                    assert np.array_equal(y, yw), tag                # the unaligned column block: the same bits
                    assert np.array_equal(y, _expand(Pm, alpha, p, act, wide=False)[0]), tag
                    # reduce: on the DEVICE's Y, so that a relu unit is on or off on both sides; NaN where the weight is 0
                    dY = rng.standard_normal((C * K, H)).astype(np.float32)
                    dY.reshape(C, K, H)[:, w == 0] = np.nan
                    ref_s = IO.reduce(dY, y, w, scale, act)
                    sc = t(scale) if bn else None
                    s = ops.ig_copies_reduce(t(dY), t(y), w, sc, act)
                    ss = ops.ig_copies_reduce(_strided(dY), _strided(y), t(w), sc, act)
                    assert tuple(s.shape) == (C, H) and torch.isfinite(s).all(), tag
                    if np.abs(ref_s).max() > 0:
                        FB.check("op reduce", s.cpu().numpy(), ref_s, tag)
                    assert torch.equal(s, ss) and torch.equal(s, ops.ig_copies_reduce(t(dY), t(y), w, sc, act)), tag
                    if C == 5:                                        # a compound alone: the same bits
                        for c in range(C):
                            y1, _ = _expand(Pm[c:c + 1], alpha, p, act, wide=False)
                            assert np.array_equal(y1, y[c * K:(c + 1) * K]), (tag, c)
                            s1 = ops.ig_copies_reduce(t(dY[c * K:(c + 1) * K]), t(y1), w, sc, act)
                            assert torch.equal(s1[0], s[c]), (tag, c)


@pytest.mark.parametrize("H", [1, 8, 63, 64, 65, 300])
def test_a_scale_one_copy_is_the_composed_layer_bit_for_bit(H):
    """Given the same P, the copy with alpha = 1 equals what dense -> graph_bn computes after the GEMM: graph_bn on P + bias (the
    dense layer's bias add, one rounding) with the activation in the same pass; ops.activation without normalisation."""
    from kgcn_amd import ops
    rng = np.random.default_rng(2000 + H)
    C = 5
    Pm = rng.standard_normal((C, H)).astype(np.float32)
    for act in ACTS:
        for bn in (True, False):
            p = _layer(rng, H, bn)
            pre = t(Pm) + t(p["b"])
            if bn:
                want = ops.graph_bn(pre.reshape(C, 1, H), t(p["gamma"]), t(p["beta"]), t(p["mean"]), t(p["var"]), None, 1e-3, False,
                                    act).reshape(C, H)
            else:
                want = ops.activation(pre, act) if act is not None else pre
            for wide in (False, True):
                y, _ = _expand(Pm, [0.5, 1.0], p, act, wide)
                assert np.array_equal(y[1::2], want.cpu().numpy()), (H, act, bn, wide)


def test_entry_points_refuse_what_they_do_not_serve():
    from kgcn_amd import _lib, ops
    lib = _lib.lib
    buf = torch.zeros(64, device="cuda")
    p, null, s = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(0), _lib.current_stream()

    def refused(rc, word):
        assert rc != 0 and word in lib.kgcn_last_error(), (rc, lib.kgcn_last_error())

    ex = lambda P, C, K, H, al, Y, ld, gamma=null: lib.kgcn_ig_copies_expand_f32(P, C, K, H, al, p, gamma, null, null, null, 1e-3, 0, Y, ld, s)
    re = lambda dY, Y, C, K, H, w, S, ld=8: lib.kgcn_ig_copies_reduce_f32(dY, ld, Y, ld, C, K, H, w, null, 0, S, s)
    refused(ex(p, 1, 2, 0, p, p, 8), b"H = 0")
    refused(ex(p, 1, 0, 8, p, p, 8), b"K = 0")
    refused(ex(p, 1, 2, 8, p, p, 7), b"row stride")
    refused(ex(null, 1, 2, 8, p, p, 8), b"NULL")
    refused(ex(p, 1, 2, 8, null, p, 8), b"NULL")
    refused(ex(p, 1, 2, 8, p, null, 8), b"NULL")
    refused(ex(p, 1, 2, 8, p, p, 8, gamma=p), b"come together")
    refused(ex(p, -1, 2, 8, p, p, 8), b"compounds")
    refused(ex(p, 1, 2, ops.IG_COPIES_MAX_WIDTH + 1, p, p, ops.IG_COPIES_MAX_WIDTH + 1), b"outside")
    refused(ex(p, 1, ops.IG_COPIES_MAX_COPIES + 1, 8, p, p, 8), b"outside")
    refused(lib.kgcn_ig_copies_expand_f32(p, 1, 2, 8, p, p, null, null, null, null, 1e-3, 9, p, 8, s), b"activation")
    refused(re(p, p, 1, 2, 0, p, p), b"H = 0")
    refused(re(p, p, 1, 0, 8, p, p), b"K = 0")
    refused(re(p, p, 1, 2, 8, p, p, ld=7), b"row stride")
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        refused(re(args[0], args[1], 1, 2, 8, args[2], args[3]), b"NULL")
    assert ex(null, 0, 2, 8, null, null, 8) == 0 and re(null, null, 0, 2, 8, null, null) == 0      # no compounds: nothing to do
    assert not buf.any()
    # the op wrappers
    P = torch.zeros((2, 8), device="cuda")
    with pytest.raises(_lib.KgcnHipError):
        ops.ig_copies_expand(torch.zeros((2, 8)), [0.0, 1.0])                                      # a host tensor
    with pytest.raises(ValueError):
        ops.ig_copies_expand(P, [])
    with pytest.raises(ValueError):
        ops.ig_copies_expand(P, [0.0, 1.0], bias=torch.zeros(7, device="cuda"))
    with pytest.raises(ValueError):
        ops.ig_copies_expand(P, [0.0, 1.0], gamma=torch.ones(8, device="cuda"))
    with pytest.raises(ValueError):
        ops.ig_copies_expand(torch.zeros((2, 0), device="cuda"), [0.0, 1.0])
    with pytest.raises(_lib.KgcnHipError):
        ops.ig_copies_expand(P, [0.0, 1.0], out=torch.zeros((4, 9), device="cuda"), out_col=2)     # the block does not fit
    with pytest.raises(ValueError):
        ops.ig_copies_reduce(torch.zeros((4, 8), device="cuda"), torch.zeros((4, 7), device="cuda"), [0.0, 1.0])
    with pytest.raises(ValueError):
        ops.ig_copies_reduce(torch.zeros((5, 8), device="cuda"), torch.zeros((5, 8), device="cuda"), [0.0, 1.0])
    with pytest.raises(ValueError):
        ops.ig_copies_reduce(torch.zeros((4, 8), device="cuda"), torch.zeros((4, 8), device="cuda"), [0.0, 1.0], scale=[1.0] * 7)
    assert tuple(ops.ig_copies_expand(torch.zeros((0, 8), device="cuda"), [0.0, 1.0]).shape) == (0, 8)


# ---- the public function against the literal loop ---------------------------------------------------------------------------------------
_SETUPS = {}


def _setup(kind):
    """Parameters, data, dataset and model of one kind, made once -> dict"""
    if kind not in _SETUPS:
        from kgcn_amd import data_util as DU, models
        P, X, A, V, sizes = IO.case(kind, Z)
        X, A, V = X[:G], A[:G], np.ascontiguousarray(V[:G])
        sizes = None if sizes is None else sizes[:G]
        channels, _ = DU.build_adjs({"dense_adj": Z["ds_dense_adj"][:G], "max_node_num": int(Z["ds_max_node_num"])})
        ds = DU.DeviceGraphDataset(channels, X, device="cuda")
        model = (models.MultimodalRegressionGCN(2) if kind == "regression" else models.MultimodalVecGCN(1, 2)).cuda()
        adj, xb = ds.batch(np.arange(G))
        with torch.no_grad():
            model(xb, adj, vectors=t(V))                                        # builds the layers
        if kind == "vec":
            set_param(model.conv.w[0], P["conv"]["w"]); set_param(model.conv.bias[0], P["conv"]["b"])
            set_param(model.dense.kernel, P["dense"]["w"]); set_param(model.dense.bias, P["dense"]["b"])
            for layer, p in zip(list(model.tower) + [model.hidden, model.out], P["tower"] + [P["hidden"], P["out"]]):
                load_dense_bn(layer, p)
        else:
            for i, (d, b) in enumerate(((model.dense1, model.bn1), (model.dense2, model.bn2), (model.dense3, model.bn3))):
                set_param(d.kernel, P["gd"][i]["w"]); set_param(d.bias, P["gd"][i]["b"])
                set_param(b.gamma, P["bn"][i]["gamma"]); set_param(b.beta, P["bn"][i]["beta"])
                set_param(b.moving_mean, P["bn"][i]["mean"]); set_param(b.moving_variance, P["bn"][i]["var"])
            load_dense_bn(model.vec, P["vec"])
            load_dense_bn(model.out, P["out"])
        labels = Z["ds_label_reg"][:G] if kind == "regression" else Z["ds_label_cls"][:G]
        _SETUPS[kind] = dict(P=P, X=X, A=A, V=V, sizes=sizes, ds=ds, model=model, labels=labels,
                             name="dragon" if kind == "regression" else "profeat")
    return _SETUPS[kind]


def _run(kind, **kw):
    from kgcn_amd import visualization as Vz
    s = _setup(kind)
    kw.setdefault("divide_number", D)
    kw.setdefault("noise_scale", IO.NOISE_SCALE)
    kw.setdefault("seed", IO.NOISE_SEED)
    return Vz.vecmodal_integrated_gradients(s["model"], None, s["ds"], t(s["V"]), labels=s["labels"], enabled_node_nums=s["sizes"], **kw)


_NOISE = {}


def _device_noise(kind):
    """The N(0, 1) values of every (compound, sample), read back from the device: scale 0, sigma 1 -> per compound the dict
    vecmodal_ig_oracle.literal takes"""
    if kind not in _NOISE:
        from kgcn_amd import ops, visualization as Vz
        s = _setup(kind)
        ids = list(range(G))
        zero, smp = torch.zeros(G * D, device="cuda"), t(np.tile(np.arange(D), G), np.int32)
        N, F = s["X"].shape[1:]
        Dv = s["V"].shape[1]
        zx = ops.ig_perturb(t(s["X"]), zero, 1.0, smp, ids, D, ops.IG_STREAM_FEATURES, IO.NOISE_SEED).cpu().numpy().reshape(G, D, N, F)
        zv = ops.ig_perturb(t(s["V"]).view(G, 1, Dv), zero, 1.0, smp, ids, D, ops.IG_STREAM_VECTOR, IO.NOISE_SEED).cpu().numpy().reshape(G, D, Dv)
        adj, _ = s["ds"].batch([i for i in ids for _ in range(D)])
        c0 = adj.channels[0]
        za = ops.ig_perturb_values(c0, c0.values, zero, 1.0, smp, [i for i in ids for _ in range(D)], ops.IG_STREAM_ADJACENCY, IO.NOISE_SEED)
        za = Vz.values_to_dense(c0, za).cpu().numpy().reshape(G, D, N, N)
        assert np.abs(zv).max() > 1 and not np.array_equal(zv[0, 0], zv[0, 1]) and not np.array_equal(zv[0, 0], zv[1, 0])
        assert not np.array_equal(zv[0, 0, :F], zx[0, 0, 0])                     # a stream of its own
        host = IO.host_noise(IO.NOISE_SEED, 1, D, (N, F), s["A"][1], Dv)         # ... that follows the header's definition
        assert np.abs(zv[1] - host["vector"]).max() < 1e-4 and np.abs(za[1] - host["adjs"]).max() < 1e-4
        _NOISE[kind] = [{"features": zx[g], "adjs": za[g], "vector": zv[g]} for g in range(G)]
    return _NOISE[kind]


_LITERAL = {}


def _literal(kind, modal, method):
    """The literal loop for the five compounds, targeting the oracle's own top prediction, computed once per case and shared."""
    key = (kind, modal, method)
    if key not in _LITERAL:
        s = _setup(kind)
        noise = _device_noise(kind) if method in IO.SMOOTH else [None] * G
        out = []
        for g in range(G):
            size = None if s["sizes"] is None else int(s["sizes"][g])
            x, A, v = s["X"][g], s["A"][g], s["V"][g]
            if kind == "vec":
                pred = IO.O.vec_model(x[None], A[None], v[None], s["P"])[0][0]
                pred = np.exp(pred - pred.max()) / np.exp(pred - pred.max()).sum()
            else:
                pred = IO.O.regression_model(x[None], np.array([size]), v[None], s["P"])[0][0]
            mask = np.zeros(2)
            mask[int(np.argmax(pred))] = 1.0
            rec = IO.literal(kind, s["P"], x, A, v, mask, modal, method, D, size, noise[g], IO.NOISE_SCALE)
            rec["target"], rec["prediction"] = int(np.argmax(pred)), float(pred.max())
            out.append(rec)
        _LITERAL[key] = out
    return _LITERAL[key]


def _against_literal(prefix, kind, recs, ref, modal, tag):
    from kgcn_amd import visualization as Vz
    s = _setup(kind)
    targets, name = IO.modal_targets(kind, modal)
    assert [r["compound_id"] for r in recs] == list(range(G))
    assert [r["target_label"] for r in recs] == [q["target"] for q in ref]
    for m in targets:
        FB.check("%s %s %s_IG" % (prefix, kind, "vector" if m == name else m), np.stack([r[m + "_IG"] for r in recs]),
               np.stack([q[m + "_IG"] for q in ref]), tag)
    # check_score = end - start is the difference of two fp32 scores (two softmax probabilities close to each other, or two
    # predictions): each carries an error of its own magnitude, so the difference is held to 1e-5 of the scores it is formed from
    FB.check("%s %s check_score" % (prefix, kind), [r["check_score"] for r in recs], [q["end"] - q["start"] for q in ref], tag,
           big=max(max(abs(q["end"]), abs(q["start"])) for q in ref))
    FB.check("%s %s prediction_score" % (prefix, kind), [r["prediction_score"] for r in recs], [q["prediction"] for q in ref], tag)
    N, F = s["X"].shape[1:]
    Dv = s["V"].shape[1]
    for r in recs:
        g = r["compound_id"]
        assert r["sum_of_IG"] == sum(float(r[m + "_IG"].astype(np.float64).sum()) for m in targets)
        assert r["true_label"] == int(np.argmax(s["labels"][g])) and r["mol"] is None and r["mol_smiles"] is None and r["mol_id"] is None
        rec = Vz.dump_record(r)
        assert set(rec) == set(Vz.DUMP_KEYS_FIXED) | set(targets) | {m + "_IG" for m in targets}
        if "features" in targets:
            assert r["features"].shape == (N, F) == r["features_IG"].shape and np.array_equal(r["features"], s["X"][g])
        if "adjs" in targets:
            assert r["adjs"].shape == (N, N) == r["adjs_IG"].shape and np.array_equal(r["adjs"], s["A"][g])
            assert not r["adjs_IG"][s["A"][g] == 0].any()
        if name in targets:
            assert r[name].shape == (Dv,) and r[name + "_IG"].shape == (1, Dv) and np.array_equal(r[name], s["V"][g])
        assert r["assay"] in ("active", "inactive")
        assert Vz.ig_filename("mol", g, r["assay"], modal) == "mol_%04d_task_0_%s_%s_scaling.jbl" % (g, r["assay"], modal)


CASES = [(kind, modal, method) for kind in ("vec", "regression") for modal in IO.modal_targets(kind, "all")[0] + ("all",)
         for method in IO.METHODS]


@pytest.mark.parametrize("kind,modal,method", CASES)
def test_public_function_matches_the_literal_loop(kind, modal, method):
    """Every modal x method, fused and composed, against the literal loop; the two routes to each other within the sum of their bounds."""
    ref = _literal(kind, modal, method)
    tag = "%s %s" % (modal, method)
    fused = _run(kind, modal=modal, method=method, fused=True)
    comp = _run(kind, modal=modal, method=method, fused=False)
    _against_literal("fused", kind, fused, ref, modal, tag)
    _against_literal("composed", kind, comp, ref, modal, tag)
    targets, name = IO.modal_targets(kind, modal)
    for m in targets:
        key = "%s %s_IG" % (kind, "vector" if m == name else m)
        a, b = (np.stack([r[m + "_IG"] for r in recs]).astype(np.float64) for recs in (fused, comp))
        err = float(np.abs(a - b).max() / np.abs(np.stack([q[m + "_IG"] for q in ref])).max())
        print("vecmodal_ig fused vs composed %s %s: %.3e of max|oracle|" % (key, tag, err))
        assert err <= FB.bound("fused " + key) + FB.bound("composed " + key)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["vec", "regression"])
def test_runs_are_bitwise_equal_and_chunks_and_subsets_change_nothing(kind, fused):
    name = _setup(kind)["name"]
    for method in ("ig", "grad", "smooth_ig"):
        kw = dict(modal="all", method=method, fused=fused)
        a, b, c = _run(kind, **kw), _run(kind, **kw), _run(kind, chunk=1, **kw)
        d = _run(kind, chunk=2, compounds=[3, 0, 4], **kw)
        assert [r["compound_id"] for r in d] == [3, 0, 4]
        keys = [k for k in a[0] if k.endswith("_IG")]
        assert name + "_IG" in keys and "features_IG" in keys
        for ra, rb, rc in zip(a, b, c):
            for k in keys:
                assert np.array_equal(ra[k], rb[k]) and np.array_equal(ra[k], rc[k]), (method, k, ra["compound_id"])
            for k in ("check_score", "sum_of_IG", "prediction_score"):
                assert ra[k] == rb[k] == rc[k], (method, k)
        for rd in d:
            ra = a[rd["compound_id"]]
            for k in keys:
                assert np.array_equal(ra[k], rd[k]), (method, k, rd["compound_id"])
            assert ra["check_score"] == rd["check_score"]


def test_refusals_targets_and_the_untargeted_vector():
    from kgcn_amd import models, visualization as Vz
    s = _setup("regression")
    with pytest.raises(ValueError):
        _run("regression", modal="adjs")
    with pytest.raises(TypeError):
        Vz.vecmodal_integrated_gradients(models.GCN(1, 2).cuda(), None, s["ds"], t(s["V"]))
    with pytest.raises(ValueError):
        _run("vec", modal="features", method="ig", compounds=[0], label_target=5)
    with pytest.raises(ValueError):
        Vz.vecmodal_integrated_gradients(s["model"], None, s["ds"], t(s["V"][:3]))                  # three vectors for five graphs
    # label targets: 'label' attributes the true class, 'correct' / 'uncorrect' split the compounds between them
    v = _setup("vec")
    by_label = _run("vec", modal="profeat", label_target="label")
    assert [r["target_label"] for r in by_label] == [int(np.argmax(l)) for l in v["labels"]]
    kept, dropped = _run("vec", modal="profeat", label_target="correct"), _run("vec", modal="profeat", label_target="uncorrect")
    assert sorted([r["compound_id"] for r in kept] + [r["compound_id"] for r in dropped]) == list(range(G))
    both = _run("regression", modal="dragon", label_target="all", method="grad_prod")
    assert [r["target_label"] for r in both] == ["all"] * G
    # host arrays in place of a dataset and a device table; the vector's own name
    from kgcn_amd import data_util as DU
    channels, _ = DU.build_adjs({"dense_adj": Z["ds_dense_adj"][:G], "max_node_num": int(Z["ds_max_node_num"])})
    host = Vz.vecmodal_integrated_gradients(v["model"], v["X"], channels, v["V"], divide_number=D, modal="vec", vector_name="vec")
    ref = _run("vec", modal="profeat")
    assert all(np.array_equal(a["vec_IG"], b["profeat_IG"]) for a, b in zip(host, ref))
    # a vector that is not a target is fed unscaled: the start copy of modal='features' still sees it
    feat, whole = _run("vec", modal="features"), _run("vec", modal="all")
    assert all(a["check_score"] != b["check_score"] for a, b in zip(feat, whole))


def test_completeness_with_the_reference_step_count():
    """D = 100, every modal: sum_of_IG ~ end - start; the GPU's gap is held to the oracle's own gap plus the family's bound for this key
    (at most 1e-5) of the magnitudes."""
    for kind in ("vec", "regression"):
        s = _setup(kind)
        recs = _run(kind, modal="all", divide_number=100)
        targets, name = IO.modal_targets(kind, "all")
        for r in recs:
            g = r["compound_id"]
            mask = np.zeros(2)
            mask[r["target_label"]] = 1.0
            ref = IO.closed_form(kind, s["P"], s["X"][g], s["A"][g], s["V"][g], mask, "all", "ig", 100,
                                 None if s["sizes"] is None else int(s["sizes"][g]))
            want = ref["end"] - ref["start"]
            scale = sum(np.abs(ref[m + "_IG"]).sum() for m in targets) + abs(want)
            excess = max(0.0, abs(r["sum_of_IG"] - r["check_score"]) - abs(ref["sum_of_IG"] - want)) / scale
            print("vecmodal_ig %s compound %d: sum_of_IG %.6f check_score %.6f (oracle %.6f / %.6f)"
                  % (kind, g, r["sum_of_IG"], r["check_score"], ref["sum_of_IG"], want))
            FB.hold("completeness excess / scale", excess, "%s compound %d" % (kind, g))


def test_example_writes_its_dumps(tmp_path):
    """examples/visualize_vecmodal.py end to end on the stand-in dataset for both models: a short fit, one file per compound under
    the reference's name, read back; then the same dumps from parameters examples/train_vecmodal.py saved."""
    import importlib.util
    joblib = pytest.importorskip("joblib")

    def load(name):
        spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    example, trainer = load("visualize_vecmodal"), load("train_vecmodal")
    for kind, name, dv in (("vec", "profeat", 70), ("regression", "dragon", 37)):
        out, out2, saved = tmp_path / kind, tmp_path / (kind + "2"), tmp_path / (kind + ".pt")
        files = example.main(["--model", kind, "--epochs", "2", "--limit", "4", "--divide-number", "10", "--out", str(out)])
        names = sorted(os.listdir(out))
        assert sorted(os.path.basename(f) for f in files) == names and len(names) == 4
        assert all(f.startswith("mol_") and "_task_0_" in f and f.endswith("_all_scaling.jbl") for f in names)
        rec = joblib.load(os.path.join(out, names[0]))
        modals = ("features", name) if kind == "regression" else ("features", "adjs", name)
        assert set(rec) == {m + s for m in modals for s in ("", "_IG")} | {"check_score", "sum_of_IG", "prediction_score", "target_label",
                                                                            "true_label", "mol", "mol_smiles", "mol_id"}
        assert rec[name + "_IG"].shape == (1, dv) and np.isfinite(rec[name + "_IG"]).all() and np.abs(rec[name + "_IG"]).max() > 0
        trainer.main(["--model", kind, "--epochs", "2", "--save", str(saved)])
        assert saved.exists()
        example.main(["--model", kind, "--params", str(saved), "--limit", "4", "--divide-number", "10", "--out", str(out2)])
        assert sorted(os.listdir(out2)) == names
        again = joblib.load(os.path.join(out2, names[0]))
        assert np.array_equal(again[name + "_IG"], rec[name + "_IG"]) and np.array_equal(again["features_IG"], rec["features_IG"])
