"""csrc/cpiig.hip, ops.cpi_ig and visualization.cpi_integrated_gradients against the fp64 oracle of tests/cpi_ig_oracle.py (the
literal loop of kgcn/visualization.py:187-260 for the public function, the sweep for the op).

Compounds: N = 10 padded rows, sizes 7, 0 (no entry at all), 10, 4 and 1; directed entries with values in {0.5, 1, 2}; node 0 of
every compound holds its self loop only; rows past the size are padding and still add sigmoid(0) = 0.5 to the read-out.

Bound: 1e-5 of max|oracle| per output array (the family's bound: test_gpu_kg_ig.py, test_gpu_multimodal_ig.py), ratcheted to ten
times the error measured on the MI355X (tests/golden/cpi_ig_bounds.json; never below one fp32 ulp, 2^-23: the outputs are fp32;
never above 1e-5).  KGCN_CPI_IG_RECORD=<file> writes the errors of a run."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpi_ig_oracle as O  # noqa: E402
import family_bounds  # noqa: E402

pytestmark = pytest.mark.gpu

N, F, WD = 10, 6, 512
SIZES = [7, 0, 10, 4, 1]
D = 8
TOL = 1e-5
# FB.check: equal shapes, finite values, a reference that is not all zero; then max|got - ref| / max|oracle| under `key`, held to
# min(1e-5, max(2^-23, stored))
FB = family_bounds.FAMILIES["cpi_ig"]
MODALS = ("all", "features", "adjs")
METHODS = ("ig", "grad_prod", "grad")


# ---- the op against the sweep ------------------------------------------------------------------------------------------------
def _op_case(seed, C, n, wd, T, K, zmax=None):
    from kgcn_amd import visualization as V
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((C, n, wd)).astype(np.float32)
    Q = (rng.standard_normal((C, n, wd)) * 0.5).astype(np.float32)
    if zmax is not None:                                   # the end copy (alpha = gamma = 1) reaches |Z| = zmax
        f = np.float32(zmax / np.abs(P.astype(np.float64) + Q).max())
        P, Q = P * f, Q * f
    u = (rng.standard_normal((T, wd)) * 2.0 / (n * np.sqrt(wd))).astype(np.float32)
    e = (rng.standard_normal(T) * 0.1).astype(np.float32)
    co = V.cpi_ig_coefficients("all", "ig" if K > 2 else "grad_prod", K - 1)
    f32 = lambda v: np.asarray(v, np.float32)
    return P, Q, u, e, f32(co["alpha"]), f32(co["gamma"]), f32(co["wA"]), f32(co["wB"])


def _run_op(case, with_b=True):
    from kgcn_amd import ops
    P, Q, u, e, al, ga, wA, wB = case
    t = lambda a: torch.as_tensor(a, device="cuda")
    out = ops.cpi_ig(t(P), t(Q), t(u), t(e), al, ga, wA, wB if with_b else None)
    torch.cuda.synchronize()
    return out


def _op_oracle(case):
    P, Q, u, e, al, ga, wA, wB = case
    res = [O.sweep(P[c], Q[c], u, e, al, ga, wA, wB) for c in range(P.shape[0])]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


@pytest.mark.parametrize("shape", ["(10,512,3,101)", "(70,40,cap+1,8)", "(1,512,1,2)", "(10,512,3,9) |Z|=90"])
def test_op_parity(shape):
    """p, G^A and G^B of ops.cpi_ig at (N, Wd, T, K): the reference's D = 100; more tasks than one accumulate pass carries, N Wd
    no multiple of 256 and Wd below a wave; the smallest of everything; pre-activations out to |Z| = 90."""
    from kgcn_amd import ops
    cap = ops.CPI_IG_TASKS_PER_PASS
    n, wd, T, K, zmax = {"(10,512,3,101)": (10, 512, 3, 101, None), "(70,40,cap+1,8)": (70, 40, cap + 1, 8, None),
                         "(1,512,1,2)": (1, 512, 1, 2, None), "(10,512,3,9) |Z|=90": (10, 512, 3, 9, 90.0)}[shape]
    case = _op_case(len(shape), 2, n, wd, T, K, zmax)
    if zmax is not None:
        assert abs(np.abs(case[0].astype(np.float64) + case[1]).max() - 90.0) < 1e-3
    p, GA, GB = _run_op(case)
    rp, rGA, rGB = _op_oracle(case)
    assert tuple(p.shape) == (2, K, T) and tuple(GA.shape) == (2, T, n, wd) == tuple(GB.shape)
    for name, got in (("p", p), ("GA", GA), ("GB", GB)):
        assert torch.isfinite(got).all(), name
    FB.check("op p", p.cpu().numpy(), rp, shape)
    FB.check("op GA", GA.cpu().numpy(), rGA, shape)
    FB.check("op GB", GB.cpu().numpy(), rGB, shape)
    p1, GA1, GB1 = _run_op(case, with_b=False)                        # the one-tensor kernel: the same bits, no G^B
    assert GB1 is None and torch.equal(p1, p) and torch.equal(GA1, GA)
    one = _run_op(tuple(a[1:2] if i < 2 else a for i, a in enumerate(case)))      # a compound alone: the same bits
    assert all(torch.equal(a[0], b[1]) for a, b in zip(one, (p, GA, GB)))


def test_op_refuses_what_it_does_not_serve():
    from kgcn_amd import _lib, ops
    P, Q, u, e, al, ga, wA, wB = _op_case(0, 1, 3, 8, 2, 4)
    t = lambda a: torch.as_tensor(a, device="cuda")
    with pytest.raises(_lib.KgcnHipError):
        ops.cpi_ig(torch.as_tensor(P), torch.as_tensor(Q), torch.as_tensor(u), torch.as_tensor(e), al, ga, wA)      # CPU tensors
    with pytest.raises(ValueError):
        ops.cpi_ig(t(P), t(Q), t(u), t(e), al[:1], ga[:1], wA[:1])                                                  # K = 1
    with pytest.raises(ValueError):
        ops.cpi_ig(t(P), t(Q[:, :2]), t(u), t(e), al, ga, wA)
    with pytest.raises(ValueError):
        ops.cpi_ig_limits_check(0, 8, 2, 4)
    assert ops.cpi_ig_limits_check(1, 1, 1, 2) == (1, 1, 1, 2)


# ---- the public function against the literal loop ----------------------------------------------------------------------------
_SETUPS = {}


def _setup(channels, T):
    """Data, parameters, dataset and model of (channels, T), made once."""
    key = (channels, T)
    if key not in _SETUPS:
        from kgcn_amd import data_util as DU, models
        rng = np.random.default_rng(100 * channels + T)
        x, dense = O.make_compounds(rng, SIZES, N, F, channels)
        assert not dense[0][1].any() and np.count_nonzero(dense[0][0][0]) == 1 and np.abs(dense[0][2] - dense[0][2].T).sum() > 0
        assert set(np.unique(dense[0])) == {0.0, 0.5, 1.0, 2.0}
        params = O.make_params(rng, F, WD, T, channels)
        params["kernel"] = (params["kernel"] * (2.0 / N)).astype(np.float32)          # predictions away from saturation
        ds = DU.DeviceGraphDataset([DU.FlatAdjacency.from_dense(d) for d in dense], x, device="cuda")
        model = models.CPIMultitaskNet(channels, T).cuda()
        adj, xb = ds.batch(np.arange(len(SIZES)))
        with torch.no_grad():
            model(xb, adj)                                             # builds the layers
            f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
            for ch in range(channels):
                model.conv.w[ch].copy_(f(params["w"][ch]))
                model.conv.bias[ch].copy_(f(params["b"][ch]).view(1, -1))
            model.out.kernel.copy_(f(params["kernel"]))
            model.out.bias.copy_(f(params["bias"]))
        _SETUPS[key] = (x, dense, params, ds, model)
    return _SETUPS[key]


_LITERAL = {}


def _literal(channels, T, modal, method, divide=D):
    """The literal loop for every (compound, task), computed once per case and shared."""
    key = (channels, T, modal, method, divide)
    if key not in _LITERAL:
        x, dense, params, _, _ = _setup(channels, T)
        _LITERAL[key] = [[O.literal(params, x[g], [d[g] for d in dense], t, modal, method, divide) for t in range(T)]
                         for g in range(len(SIZES))]
    return _LITERAL[key]


def _stack(recs, ref, name):
    return np.stack([r[name] for r in recs]), np.stack([ref[r["compound_id"]][r["task"]][name] for r in recs])


def _against_literal(prefix, recs, ref, modal, tag):
    assert [(r["compound_id"], r["task"]) for r in recs] == [(g, t) for g in range(len(SIZES)) for t in range(len(ref[0]))]
    for m in O.modal_targets(modal):
        FB.check(prefix + " " + m + "_IG", *_stack(recs, ref, m + "_IG"), tag)
    se = np.array([[ref[r["compound_id"]][r["task"]]["start"], ref[r["compound_id"]][r["task"]]["end"]] for r in recs])
    FB.check(prefix + " start", [r["start_score"] for r in recs], se[:, 0], tag)
    FB.check(prefix + " end", [r["end_score"] for r in recs], se[:, 1], tag)
    FB.check(prefix + " check_score", [r["check_score"] for r in recs], se[:, 1] - se[:, 0], tag)
    FB.check(prefix + " prediction_score", [r["prediction_score"] for r in recs], se[:, 1], tag)      # the unscaled forward pass
    for r in recs:
        total = sum(float(r[m + "_IG"].astype(np.float64).sum()) for m in O.modal_targets(modal))
        assert r["sum_of_IG"] == total and r["check_score"] == r["end_score"] - r["start_score"]


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("modal", MODALS)
def test_public_function_matches_the_literal_loop(modal, method, channels, T):
    from kgcn_amd import visualization as V
    x, dense, params, ds, model = _setup(channels, T)
    ref = _literal(channels, T, modal, method)
    recs = V.cpi_integrated_gradients(model, None, ds, divide_number=D, modal=modal, method=method)
    tag = "%s %s C=%d T=%d" % (modal, method, channels, T)
    _against_literal("public", recs, ref, modal, tag)
    for r in recs:
        g = r["compound_id"]
        assert r["target_label"] == 0 and r["true_label"] is None and r["mol"] is None and r["mol_smiles"] is None and r["mol_id"] is None
        assert r["assay"] == ("active" if r["prediction_score"] > 0.5 else "inactive")
        if "features" in r:
            assert r["features"].shape == (N, F) == r["features_IG"].shape and np.array_equal(r["features"], x[g])
        if "adjs" in r:
            assert r["adjs"].shape == (N, N) == r["adjs_IG"].shape and np.array_equal(r["adjs"], dense[0][g])
            assert not r["adjs_IG"][dense[0][g] == 0].any()
        assert set(V.cpi_dump_record(r)) == set(r) - {"compound_id", "task", "assay", "start_score", "end_score"}
        assert set(V.DUMP_KEYS_FIXED) <= set(V.cpi_dump_record(r))


@pytest.mark.parametrize("channels,T", [(1, 1), (2, 3)])
@pytest.mark.parametrize("modal", MODALS)
def test_fused_against_the_composed_route(modal, channels, T):
    """fused=False runs the copies through the model and autograd: held to the literal loop like the fused route, and the two
    to each other within the sum of their bounds."""
    from kgcn_amd import visualization as V
    _, _, _, ds, model = _setup(channels, T)
    ref = _literal(channels, T, modal, "ig")
    fused = V.cpi_integrated_gradients(model, None, ds, divide_number=D, modal=modal)
    comp = V.cpi_integrated_gradients(model, None, ds, divide_number=D, modal=modal, fused=False)
    tag = "%s C=%d T=%d" % (modal, channels, T)
    _against_literal("composed", comp, ref, modal, tag)
    for m in O.modal_targets(modal):
        a, b = np.stack([r[m + "_IG"] for r in fused]).astype(np.float64), np.stack([r[m + "_IG"] for r in comp]).astype(np.float64)
        big = np.abs(np.stack([ref[r["compound_id"]][r["task"]][m + "_IG"] for r in fused])).max()
        err = float(np.abs(a - b).max() / big)
        print("cpi_ig fused vs composed %s %s: %.3e of max|oracle|" % (m, tag, err))
        assert err <= 2 * TOL
    some = V.cpi_integrated_gradients(model, None, ds, divide_number=D, modal=modal, fused=False, tasks=[T - 1], compounds=[3, 0])
    assert [(r["compound_id"], r["task"]) for r in some] == [(3, T - 1), (0, T - 1)]
    pick = {(r["compound_id"], r["task"]): r for r in comp}
    for r in some:
        for m in O.modal_targets(modal):
            assert np.array_equal(r[m + "_IG"], pick[(r["compound_id"], r["task"])][m + "_IG"])


@pytest.mark.parametrize("channels,T", [(1, 3), (2, 3)])
def test_runs_are_bitwise_equal_and_chunks_change_nothing(channels, T):
    from kgcn_amd import visualization as V
    _, _, _, ds, model = _setup(channels, T)
    for method in ("ig", "grad"):
        kw = dict(divide_number=D, modal="all", method=method)
        a = V.cpi_integrated_gradients(model, None, ds, **kw)
        b = V.cpi_integrated_gradients(model, None, ds, **kw)
        c = V.cpi_integrated_gradients(model, None, ds, chunk=1, **kw)
        d = V.cpi_integrated_gradients(model, None, ds, chunk=2, tasks=[2, 0], compounds=[4, 2, 0], **kw)
        assert [(r["compound_id"], r["task"]) for r in d] == [(g, t) for g in (4, 2, 0) for t in (2, 0)]
        pick = {(r["compound_id"], r["task"]): r for r in a}
        for ra, rb, rc in zip(a, b, c):
            for k in ("features_IG", "adjs_IG"):
                assert np.array_equal(ra[k], rb[k]) and np.array_equal(ra[k], rc[k]), (method, k, ra["compound_id"], ra["task"])
            for k in ("check_score", "sum_of_IG", "prediction_score"):
                assert ra[k] == rb[k] == rc[k]
        for rd in d:
            ra = pick[(rd["compound_id"], rd["task"])]
            assert np.array_equal(ra["features_IG"], rd["features_IG"]) and np.array_equal(ra["adjs_IG"], rd["adjs_IG"])
            assert ra["check_score"] == rd["check_score"]


def test_chunks_change_nothing_across_the_dense_row_threshold():
    """110 compounds of 10 rows: one chunk hands the dense op 1,100 rows (3,300 in the contraction), past the 1,024 rows from
    which it would pick its table kernels, and past CPI_IG_DENSE_ROWS, so the rows go in slices; chunk=1 hands it 10."""
    from kgcn_amd import data_util as DU, visualization as V
    x, dense, _, _, model = _setup(2, 3)
    rep = 22
    ds = DU.DeviceGraphDataset([DU.FlatAdjacency.from_dense(np.tile(d, (rep, 1, 1))) for d in dense], np.tile(x, (rep, 1, 1)), device="cuda")
    assert ds.num_graphs * N > V.CPI_IG_DENSE_ROWS + 1
    kw = dict(divide_number=4, modal="all")
    whole = V.cpi_integrated_gradients(model, None, ds, **kw)
    parts = V.cpi_integrated_gradients(model, None, ds, chunk=1, **kw)
    few = V.cpi_integrated_gradients(model, None, _setup(2, 3)[3], **kw)
    assert len(whole) == len(parts) == 3 * 5 * rep
    for i, (a, b) in enumerate(zip(whole, parts)):
        c = few[i % len(few)]                                          # the same compound in the five-compound dataset
        for k in ("features_IG", "adjs_IG"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (k, a["compound_id"], a["task"])
        assert a["start_score"] == b["start_score"] == c["start_score"] and a["end_score"] == b["end_score"] == c["end_score"]


def test_completeness_with_the_reference_step_count():
    """D = 100, one channel, both modals: sum_of_IG ~ end - start.  The GPU's gap is held to the oracle's own gap at D = 100 plus
    1e-5 of the magnitudes summed (fp32 sums of fp32 terms)."""
    from kgcn_amd import visualization as V
    x, dense, params, ds, model = _setup(1, 3)
    recs = V.cpi_integrated_gradients(model, None, ds, divide_number=100, modal="all")
    for r in recs:
        ref = O.closed_form(params, x[r["compound_id"]], [dense[0][r["compound_id"]]], r["task"], "all", "ig", 100)
        want = ref["end"] - ref["start"]
        oracle_gap = abs(ref["sum_of_IG"] - want)
        gpu_gap = abs(r["sum_of_IG"] - r["check_score"])
        scale = np.abs(ref["features_IG"]).sum() + np.abs(ref["adjs_IG"]).sum() + abs(want)
        if scale == 0:                                                 # the compound without an entry: nothing to attribute
            assert r["compound_id"] == 1 and gpu_gap == 0 and r["sum_of_IG"] == 0
            continue
        excess = max(0.0, gpu_gap - oracle_gap) / scale
        print("cpi_ig compound %d task %d: gap gpu %.3e oracle %.3e of %.3e" % (r["compound_id"], r["task"], gpu_gap, oracle_gap, abs(want)))
        FB.hold("completeness excess / scale", excess, "compound %d task %d" % (r["compound_id"], r["task"]))
        assert oracle_gap <= 0.05 * abs(want) + 1e-9                   # D = 100 is close to the integral


def test_refusals_and_label_targets():
    from kgcn_amd import models, visualization as V
    x, dense, params, ds, model = _setup(1, 3)
    with pytest.raises(TypeError):
        V.cpi_integrated_gradients(models.GCN(1, 2), None, ds)
    with pytest.raises(ValueError):
        V.cpi_integrated_gradients(model, None, ds, modal="embedded_layer")
    for method in ("smooth_grad", "smooth_ig"):
        with pytest.raises(ValueError):
            V.cpi_integrated_gradients(model, None, ds, method=method)
    labels = np.array([[0, 1, 0]] * len(SIZES), np.float32)
    with pytest.raises(ValueError):                                    # label 1 indexes outside the one-entry prediction
        V.cpi_integrated_gradients(model, None, ds, labels=labels, label_target="label", divide_number=2, tasks=[1])
    recs = V.cpi_integrated_gradients(model, None, ds, labels=labels, label_target="label", divide_number=2, tasks=[0, 2])
    assert [(r["task"], r["true_label"], r["target_label"]) for r in recs] == [(0, 0, 0), (2, 0, 0)] * len(SIZES)
    kept = V.cpi_integrated_gradients(model, None, ds, labels=labels, label_target="correct", divide_number=2)
    assert [(r["compound_id"], r["task"]) for r in kept] == [(g, t) for g in range(len(SIZES)) for t in (0, 2)]
    one = V.cpi_integrated_gradients(models.CPIMultitaskNet(1, 1).cuda(), x, [DU_channel(dense[0])], labels=np.array([[1, 0]] * len(SIZES)),
                                     divide_number=2)
    assert [r["true_label"] for r in one] == [0] * len(SIZES) and len(one) == len(SIZES)


def DU_channel(dense):
    from kgcn_amd import data_util as DU
    return DU.FlatAdjacency.from_dense(dense)


def test_example_writes_its_dumps(tmp_path):
    """examples/visualize_cpi.py end to end on the stand-in dataset: fold 1 trained for two epochs, one file per (test compound,
    task) under the reference's name, read back; then the same dumps from the saved model.001.best.pt."""
    import importlib.util
    joblib = pytest.importorskip("joblib")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("visualize_cpi_example", os.path.join(root, "examples", "visualize_cpi.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out, out2, saved = tmp_path / "viz", tmp_path / "viz2", tmp_path / "model"
    files = example.main(["--epochs", "2", "--outdir", str(out), "--divide-number", "10", "--save-model", str(saved)])
    names = sorted(os.listdir(out))
    assert sorted(os.path.basename(f) for f in files) == names and len(names) == 12 * 3
    assert all(f.startswith("mol_") and f.endswith("_all_scaling.jbl") and "_task_" in f for f in names)
    rec = joblib.load(os.path.join(out, names[0]))
    assert set(rec) == {"features", "features_IG", "adjs", "adjs_IG", "check_score", "sum_of_IG", "prediction_score", "target_label",
                        "true_label", "mol", "mol_smiles", "mol_id"}
    assert rec["features_IG"].shape == rec["features"].shape and np.isfinite(rec["features_IG"]).all() and np.abs(rec["features_IG"]).max() > 0
    best = saved / "model.001.best.pt"
    assert best.exists()
    example.main(["--params", str(best), "--outdir", str(out2), "--divide-number", "10"])
    assert sorted(os.listdir(out2)) == names
    again = joblib.load(os.path.join(out2, names[0]))
    assert np.array_equal(again["features_IG"], rec["features_IG"]) and np.array_equal(again["adjs_IG"], rec["adjs_IG"])
