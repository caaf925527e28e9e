"""kgcn_amd.visualization.seqcnn_integrated_gradients and the two kernels of csrc/convig.hip on the GPU.

Kernels: ops.conv1d_ig_expand / ops.conv1d_ig_reduce against tests/seqcnn_ig_oracle.expand32 / reduce32, bit for bit.

Model level: against the fp64 per-copy loop of tests/seqcnn_ig_oracle.integrated_gradients, at the model's real widths
(505 / 200 / 100; S = 26, E = 25, L = 26, D = 4, two proteins) and at a narrow subclass (33 / 20 / 12; L = 50, D = 8, three
proteins, chunk 2: the last chunk is short and every pool leaves conv positions outside its windows).  A case is drawn from the
first seed (300 allowed) whose oracle values meet the preconditions of tests/test_gpu_seqcnn.py over every copy of non-zero
weight; the search runs on the oracle alone and is asserted before anything is compared.

Bounds: the family `seqcnn_ig` (cap 1e-5, max |err| / max |ref|), held through this module's own family_bounds.Family on
tests/golden/seqcnn_ig_bounds.json; KGCN_SEQCNN_IG_RECORD=<file> records, and
    python tests/test_gpu_seqcnn_ig.py RECORD.json
rewrites the file by the project's rule, stored = min(cap, max(10 x measured, ULP)).  Error figures: embedded_layer_IG over
max |ref|; check_score = end - start over the larger of |start| and |end| (the scores' own magnitude: the difference may cancel);
sum_of_IG over sum |ref IG| (the magnitude of what is summed).  The smooth methods are compared with the oracle fed the device's own
noise (read back through ops.ig_perturb with scale 0 and sigma 1) and held to the written tolerance of the smooth_ig family,
1e-4, as a local bound; without noise they are the clean methods and are held to this family's bounds."""
import atexit
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_bounds  # noqa: E402
import seqcnn_ig_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu

FB = family_bounds.Family("seqcnn_ig", 1e-5, family_bounds.ULP, family_bounds.OVER_REF, strict=True)
atexit.register(FB.write_record)
SMOOTH_CAP = 1e-4                                   # family_bounds.FAMILIES["smooth_ig"].cap, held locally
S, E = 26, 25
CASES = {"real": dict(L=26, D=4, G=2, widths=(505, 200, 100), chunk=None),
         "narrow": dict(L=50, D=8, G=3, widths=(33, 20, 12), chunk=2)}
METHODS = ("ig", "grad_prod", "grad")
ROUTES = {"fused": dict(fused=True), "composed": dict(fused=False), "loop": dict(fused=False, batched=False)}


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(1, 1, 1, 1), (2, 9, 6, 505), (3, 5, 12, 33), (1, 101, 3, 200)]


def _kernel_inputs(C, K, T, F):
    rng = np.random.default_rng(1000 * C + 10 * K + T + F)
    Pm = rng.standard_normal((C, T, F)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, F).astype(np.float32)
    alpha = (np.arange(K) / max(K - 1, 1)).astype(np.float32) if K > 1 else np.ones(1, np.float32)
    w = np.array([0.0] + [1.0 / max(K - 1, 1)] * (K - 1), np.float32) if K > 1 else np.ones(1, np.float32)
    dout = rng.standard_normal((C * K, T, F)).astype(np.float32)
    return Pm, bias, alpha, w, dout


def _dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", KERNEL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_expand_and_reduce_bit_for_bit(shape):
    from kgcn_amd import ops
    C, K, T, F = shape
    Pm, bias, alpha, w, dout = _kernel_inputs(*shape)
    out = ops.conv1d_ig_expand(_dev(Pm), alpha, _dev(bias))
    ref = IO.expand32(Pm, alpha, bias)
    assert tuple(out.shape) == (C * K, T, F)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref))
    r = ops.conv1d_ig_reduce(_dev(dout), out, w)
    assert tuple(r.shape) == (C, T, F)
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(IO.reduce32(dout, ref, w)))


def test_reduce_never_reads_a_copy_of_weight_zero():
    from kgcn_amd import ops
    shape = (2, 9, 6, 505)
    Pm, bias, alpha, w, dout = _kernel_inputs(*shape)
    w[[3, 4, 8]] = 0.0                                       # zeros in the middle and at the end, beside copy 0
    d4 = dout.reshape(2, 9, 6, 505)
    d4[:, w == 0] = np.nan
    ref_out = IO.expand32(Pm, alpha, bias)
    ref = IO.reduce32(dout, ref_out, w)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    r = ops.conv1d_ig_reduce(_dev(dout), _dev(ref_out), w).cpu().numpy()
    assert np.array_equal(_bits(r), _bits(ref))
    zero = ops.conv1d_ig_reduce(_dev(dout), _dev(ref_out), np.zeros(9, np.float32)).cpu().numpy()
    assert np.array_equal(_bits(zero), np.zeros((2, 6, 505), np.uint32))


def test_expand_on_the_relu_edge():
    """Pm entries of exactly -b / alpha and one ulp to either side: the sum is exactly 0 and the output +0, never -0."""
    from kgcn_amd import ops
    alpha = np.array([0.5, 1.0, 0.25], np.float32)
    bias = np.array([0.25, -0.5, 0.0, 0.75, 0.125], np.float32)
    edge = np.array([-0.5, 1.0, 0.0, -1.5, -0.25], np.float32)            # -b / 0.5
    Pm = np.stack([edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf)), -edge])[None]
    Pm[0, 2, 2] = -0.0                                                      # -0 * alpha + 0 must give +0
    out = ops.conv1d_ig_expand(_dev(Pm), alpha, _dev(bias)).cpu().numpy()
    ref = IO.expand32(Pm, alpha, bias)
    assert np.array_equal(_bits(out), _bits(ref))
    assert np.array_equal(_bits(out[0, 0]), np.zeros(5, np.uint32))          # alpha 0.5, the edge row: +0
    assert not np.signbit(out).any()
    # the gradient mask of the reduce follows: nothing flows through the edge
    dout = np.ones_like(out)
    r = ops.conv1d_ig_reduce(_dev(dout), _dev(out), np.array([1.0, 0.0, 0.0], np.float32)).cpu().numpy()
    assert np.array_equal(r[0, 0], np.zeros(5, np.float32))
    assert np.array_equal(_bits(r), _bits(IO.reduce32(dout, ref, [1.0, 0.0, 0.0])))


def test_expand_at_scale_one_is_the_composed_first_layer():
    """csrc/conv1d.hip adds its bias after the accumulation, so expand at alpha = 1 equals the token-mode first layer bit for bit."""
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(7)
    C, L, F, k, pool = 3, 50, 505, 4, 4
    tokens = _dev(rng.integers(0, S, (C, L)).astype(np.int32))
    table = _dev(rng.uniform(-1, 1, (S, E)).astype(np.float32))
    w = _dev((rng.standard_normal((k, E, F)) / 8).astype(np.float32))
    bias = _dev(rng.uniform(-0.1, 0.1, F).astype(np.float32))
    with torch.no_grad():
        composed = ops.conv1d_pool(None, w, bias, pool, "relu", tokens=tokens, table=table)
    Pm, arg = ops.conv1d_pool_window_max(tokens, table, w, pool)
    assert arg.dtype == torch.uint8 and int(arg.max()) < pool
    fused = ops.conv1d_ig_expand(Pm, [1.0], bias)
    assert float(composed.max()) > 0 and float((composed == 0).float().mean()) > 0.01          # both sides of the relu occur
    assert torch.equal(composed, fused)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]
    bound = family_bounds.FAMILIES["seqcnn"].bound("forward")
    seed, p, tokens, labels = IO.find_case(9000, S, E, c["L"], c["G"], c["D"], c["widths"], bound)
    return seed, p, tokens, labels, bound


@functools.lru_cache(maxsize=None)
def _reference(name, method):
    _, p, tokens, _, _ = _case(name)
    table = np.asarray(p["embeddings"], np.float64)
    return [IO.integrated_gradients(p, table[tok], np.array([0.0, 1.0]), method, CASES[name]["D"]) for tok in tokens]


@functools.lru_cache(maxsize=None)
def _model(name):
    import torch
    from kgcn_amd import models
    from test_gpu_seqcnn import model_params
    c = CASES[name]
    _, p, tokens, _, _ = _case(name)
    cls = type("Narrow", (models.SeqCNN,), {"WIDTHS": c["widths"]}) if name == "narrow" else models.SeqCNN
    assert cls.WIDTHS == c["widths"]
    dev = torch.device("cuda:0")
    model = cls(S, embedding_dim=E, label_dim=2).to(dev)
    tok = torch.as_tensor(tokens, device=dev)
    with torch.no_grad():
        model(None, None, sequences=tok)                                    # lazy build
        for k, q in model_params(model).items():
            q.copy_(torch.as_tensor(p[k], device=dev).reshape(q.shape))
    return model, tok


def _run(name, method, **kw):
    from kgcn_amd import visualization as V
    model, tok = _model(name)
    c = CASES[name]
    kw.setdefault("chunk", c["chunk"])
    kw.setdefault("label_target", 1)
    return V.seqcnn_integrated_gradients(model, tok, labels=_case(name)[3], divide_number=c["D"], method=method, **kw)


def _hold(recs, refs, method, tag):
    assert [r["compound_id"] for r in recs] == list(range(len(refs)))
    for r, ref in zip(recs, refs):
        t = "%s protein %d" % (tag, r["compound_id"])
        FB.check("embedded_layer_IG_" + method, r["embedded_layer_IG"], ref["ig"], t)
        FB.check("check_score", [r["check_score"]], [ref["end"] - ref["start"]], t, big=max(abs(ref["start"]), abs(ref["end"])))
        FB.check("sum_of_IG_" + method, [r["sum_of_IG"]], [ref["sum"]], t, big=float(np.abs(ref["ig"]).sum()))
        assert r["target_label"] == 1 and abs(r["prediction_score"] - ref["end"]) <= 1e-5


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_well_conditioned(name):
    seed, p, tokens, _, bound = _case(name)
    print("SEQCNN_IG case %s: seed %d, margin factor %.3e" % (name, seed, bound))
    assert IO.case_conditioned(p, tokens, CASES[name]["D"], bound)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_against_the_oracle(name, method):
    _, p, tokens, _, bound = _case(name)
    assert IO.case_conditioned(p, tokens, CASES[name]["D"], bound)
    refs = _reference(name, method)
    got = {}
    for route, kw in ROUTES.items():
        got[route] = _run(name, method, **kw)
        _hold(got[route], refs, method, "%s %s %s" % (name, method, route))
    assert [r["target_label"] for r in got["fused"]] == [r["target_label"] for r in got["composed"]]
    assert [r["embedded_layer"].shape for r in got["fused"]] == [(CASES[name]["L"], E)] * CASES[name]["G"]
    assert np.array_equal(got["fused"][0]["embedded_layer"], np.asarray(p["embeddings"])[tokens[0]])


def test_default_route_is_the_module_constant():
    from kgcn_amd import visualization as V
    a, b = _run("narrow", "ig"), _run("narrow", "ig", fused=V.SEQCNN_IG_FUSED)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x["embedded_layer_IG"]), _bits(y["embedded_layer_IG"]))


@pytest.mark.parametrize("route", ["fused", "composed"])
def test_two_runs_give_the_same_bits(route):
    a, b = _run("narrow", "ig", **ROUTES[route]), _run("narrow", "ig", **ROUTES[route])
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x["embedded_layer_IG"]), _bits(y["embedded_layer_IG"]))
        assert x["check_score"] == y["check_score"] and x["sum_of_IG"] == y["sum_of_IG"]


def test_chunking_changes_no_bit_on_the_fused_route():
    runs = [_run("narrow", "ig", fused=True, chunk=ch) for ch in (1, 2, 3)]
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(_bits(x["embedded_layer_IG"]), _bits(y["embedded_layer_IG"]))
            assert x["check_score"] == y["check_score"]
    sub = _run("narrow", "ig", fused=True, proteins=[2, 0])
    assert [r["compound_id"] for r in sub] == [2, 0]
    assert np.array_equal(_bits(sub[0]["embedded_layer_IG"]), _bits(runs[0][2]["embedded_layer_IG"]))


@pytest.mark.parametrize("method,clean", [("smooth_ig", "ig"), ("smooth_grad", "grad")])
def test_smooth_methods(method, clean):
    import torch
    from kgcn_amd import ops
    same = [_run("narrow", method, seed=77), _run("narrow", method, seed=77)]
    other = _run("narrow", method, seed=78)
    loop = _run("narrow", method, seed=77, batched=False)
    # the oracle receives the device's own noise, read back as 0 * 0 + 1 * z: sample k of protein g, stream IG_STREAM_SEQUENCE
    c = CASES["narrow"]
    G, L, D = c["G"], c["L"], c["D"]
    dev = torch.device("cuda:0")
    noise = ops.ig_perturb(torch.zeros((G, L, E), device=dev), torch.zeros(G * D, device=dev), 1.0, list(range(D)) * G, list(range(G)), D,
                           ops.IG_STREAM_SEQUENCE, 77).cpu().numpy().reshape(G, D, L, E)
    assert np.abs(noise).max() > 1 and abs(float(noise.mean())) < 0.1
    _, p, tokens, _, _ = _case("narrow")
    table = np.asarray(p["embeddings"], np.float64)
    for g, (x, y, z, q) in enumerate(zip(same[0], same[1], other, loop)):
        assert np.array_equal(_bits(x["embedded_layer_IG"]), _bits(y["embedded_layer_IG"]))
        assert not np.array_equal(_bits(x["embedded_layer_IG"]), _bits(z["embedded_layer_IG"]))
        ref = IO.smooth(p, table[tokens[g]], [0.0, 1.0], method, D, 0.1, noise[g])
        for tag, r in (("batched", x), ("per-copy loop", q)):
            assert r["embedded_layer_IG"].shape == ref["ig"].shape and np.isfinite(r["embedded_layer_IG"]).all()
            err = family_bounds.rel_err(r["embedded_layer_IG"], ref["ig"])
            print("BOUND smooth (local) | %s %s protein %d | err / max|ref| = %.3e | bound %.3e" % (method, tag, g, err, SMOOTH_CAP))
            assert err <= SMOOTH_CAP
            assert abs(r["check_score"] - (ref["end"] - ref["start"])) <= SMOOTH_CAP * max(abs(ref["start"]), abs(ref["end"]))
    # without noise the smooth methods are the clean ones: D samples at the clean scales, held to the family's bound
    refs = _reference("narrow", clean)
    if method == "smooth_grad":                          # D samples of the scale-1 gradient, weight 1 / D each: the gradient itself
        quiet = _run("narrow", method, noise_scale=0.0)
        for r, ref in zip(quiet, refs):
            FB.check("embedded_layer_IG_grad", r["embedded_layer_IG"], ref["ig"], "smooth_grad, noise 0")
    else:
        quiet = _run("narrow", method, noise_scale=0.0)
        for r, ref in zip(quiet, refs):
            FB.check("embedded_layer_IG_ig", r["embedded_layer_IG"], ref["ig"], "smooth_ig, noise 0")
            FB.check("check_score", [r["check_score"]], [ref["end"] - ref["start"]], "smooth_ig, noise 0",
                     big=max(abs(ref["start"]), abs(ref["end"])))
    with pytest.raises(ValueError):
        _run("narrow", method, fused=True)


@pytest.mark.parametrize("label_target", [1, "all", "label", "correct"])
def test_label_targets_give_the_jobs_select_label_target_defines(label_target):
    import torch
    from kgcn_amd import visualization as V
    model, tok = _model("narrow")
    labels = _case("narrow")[3]
    with torch.no_grad():
        pred = torch.softmax(model(None, None, sequences=tok), 1).cpu().numpy()
    want = []
    for i in range(tok.shape[0]):
        sel = V.select_label_target(pred[i], label_target, int(np.argmax(labels[i])))
        if sel is not None:
            want.append((i, sel[0], sel[1], int(np.argmax(labels[i]))))
    recs = _run("narrow", "grad_prod", label_target=label_target, fused=True)
    assert [(r["compound_id"], r["target_label"], r["true_label"]) for r in recs] == [(i, t, y) for i, t, _, y in want]
    for r, (_, _, score, _) in zip(recs, want):
        assert r["prediction_score"] == pytest.approx(score, abs=1e-6)
        assert set(r) >= {"embedded_layer", "embedded_layer_IG", "prediction_score", "target_label", "true_label", "check_score",
                          "sum_of_IG", "mol", "mol_smiles", "mol_id"}
    if label_target == "all":                            # the probabilities sum to one at every scale: nothing to attribute
        assert all(abs(r["check_score"]) <= 1e-6 for r in recs)


def test_sequence_symbol_gives_the_amino_acid_string():
    tokens = _case("narrow")[2]
    recs = _run("narrow", "grad", fused=True, sequence_symbol=tokens, proteins=[1])
    assert recs[0]["amino_acid_seq"] == "".join(chr(ord("A") + int(t)) for t in tokens[1])


def test_example_writes_loadable_files(tmp_path):
    import joblib
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "visualize_seqcnn.py"), "--divide-number", "4",
           "--proteins", "all", "--limit", "2", "--epochs", "1", "--out", str(tmp_path)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-3000:]
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 2 and all(f.startswith("mol_000%d_task_0_" % i) and f.endswith("_embedded_layer_scaling.jbl") for i, f in enumerate(files))
    for f in files:
        rec = joblib.load(os.path.join(str(tmp_path), f))
        assert rec["embedded_layer"].shape == rec["embedded_layer_IG"].shape == (96, 25)
        assert np.isfinite(rec["embedded_layer_IG"]).all() and rec["target_label"] == 1
        assert len(rec["amino_acid_seq"]) == 96 and "compound_id" not in rec
        assert abs(rec["sum_of_IG"] - float(rec["embedded_layer_IG"].astype(np.float64).sum())) <= 1e-12


def regenerate(record_path, bounds_path=None):
    """`bounds` and `measured` of tests/golden/seqcnn_ig_bounds.json from the record of a run, by family_bounds' rule."""
    path = bounds_path or FB.path
    measured = json.load(open(record_path))["measured"]
    table = json.load(open(path)) if os.path.exists(path) else {}
    table["measured"] = {k: measured[k] for k in sorted(measured)}
    table["bounds"] = {k: min(FB.cap, max(10.0 * measured[k], FB.floor)) for k in sorted(measured)}
    with open(path, "w") as out:
        json.dump(table, out, indent=1)
        out.write("\n")
    return table


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit("usage: python tests/test_gpu_seqcnn_ig.py RECORD.json [BOUNDS.json]")
    print("seqcnn_ig: %d bounds written" % len(regenerate(*sys.argv[1:])["bounds"]))
