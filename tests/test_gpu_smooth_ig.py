"""The smooth attribution methods on the GPU (csrc/igprep.hip, the perturbed staging mode of csrc/seq.hip, ops.ig_perturb /
ops.ig_perturb_values / ops.seq_conv_pool_perturbed, visualization.multimodal_integrated_gradients and integrated_gradients with
method 'smooth_grad' / 'smooth_ig') against the fp64 oracle of tests/smooth_ig_oracle.py, which draws the same noise value for value.

Bounds.  The device draws its normals in fp32 (logf, sincospif) and the oracle in fp64, so every compared quantity carries a few
ulp of sigma |z| on top of the clean path's rounding.  Each comparison prints its error (max abs error over max |oracle|; absolute
for check_score and sum_of_IG), records it, and is held to the bound of tests/golden/smooth_ig_bounds.json = max(10 x the error
measured on an MI355X, 2^-23), and never to more than CAP = 1e-4 (ten times the clean path's tolerance): an error beyond CAP is a
defect, not a bound to record.  KGCN_SMOOTH_IG_RECORD=<file> writes the errors of a run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_ig_oracle as IG  # noqa: E402
import family_bounds  # noqa: E402
import smooth_ig_oracle as SO  # noqa: E402
from family_bounds import rel_err  # noqa: E402
from gpu_helpers import conv_case, g7_case, multimodal_params, oracle_inputs, to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

# FB.check: max|got - ref| / max(1e-30, max|oracle|) (absolute=True: max|got - ref|) under `key`, held to min(CAP, max(2^-23, stored)),
# CAP = 1e-4; a comparison without a stored bound is an error, except in a recording run, where CAP alone holds
FB = family_bounds.FAMILIES["smooth_ig"]
SEED = 1234
NS = float(np.float32(0.1))                    # the noise scale as the device holds it


# ---- the perturbation kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", [(3, 5), (1, 4), (50, 81)])
def test_perturb_rows_match_the_oracle_noise(N, F):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(N * 100 + F)
    C, rep = 2, 4
    ids = [5, 2]
    x = rng.standard_normal((C, N, F)).astype(np.float32)
    scale = np.tile(np.array([0.0, 0.5, 1.0, 0.75], np.float32), C)
    sigma = np.tile(np.array([0.0, 0.1, 0.1, 0.0], np.float32), C)
    sample = np.tile(np.array([0, 0, 3, 1], np.int32), C)
    out = ops.ig_perturb(_t(x), _t(scale), _t(sigma), _t(sample, np.int32), ids, rep, ops.IG_STREAM_FEATURES, SEED)
    assert tuple(out.shape) == (C * rep, N, F)
    ref = np.empty((C * rep, N, F))
    for b in range(C * rep):
        c = b // rep
        if sigma[b] == 0:
            assert torch.equal(out[b], _t(x[c]) * float(scale[b])), b
        z = SO.noise(SEED, SO.STREAM_FEATURES, ids[c], int(sample[b]), N, F)
        ref[b] = SO.add_perturbation(x[c].astype(np.float64), float(scale[b]), z, float(sigma[b]))
    FB.check("perturb rows N=%d F=%d" % (N, F), _np(out), ref)
    assert torch.equal(out, ops.ig_perturb(_t(x), _t(scale), _t(sigma), _t(sample, np.int32), ids, rep, ops.IG_STREAM_FEATURES, SEED))
    other = ops.ig_perturb(_t(x), _t(scale), _t(sigma), _t(sample, np.int32), ids, rep, ops.IG_STREAM_FEATURES, SEED + 1)
    assert not torch.equal(out, other)


def test_perturb_values_empty_single_and_duplicate_entries():
    import torch
    from kgcn_amd import ops
    from kgcn_amd.batched_csr import BatchedCSR
    rng = np.random.default_rng(5)
    M = 6
    # graph 0: no entry; 1: one entry; 2: (1, 2) stored twice beside (0, 1); 3: 21 entries (more than one Philox block a row);
    # 4: no entry again (the last graph)
    g3 = rng.integers(0, M, size=(21, 2))
    graph = np.r_[[1], [2, 2, 2], np.full(21, 3)]
    row = np.r_[[4], [1, 0, 1], g3[:, 0]]
    col = np.r_[[5], [2, 1, 2], g3[:, 1]]
    val = rng.uniform(0.5, 2.0, graph.shape[0]).astype(np.float32)
    csr = BatchedCSR.from_arrays(graph, row, col, val, 5, M, M, device="cuda")
    rp = csr.rowptr.cpu().numpy().astype(np.int64)
    per = rp[M::M] - rp[:-1:M]
    assert list(per) == [0, 1, 3, 21, 0]
    ids = [7, 3, 11, 0, 2]
    scale = np.array([1.0, 0.5, 0.25, 1.0, 0.5], np.float32)
    sigma = np.array([0.1, 0.1, 0.1, 0.1, 0.0], np.float32)
    sample = np.array([0, 2, 1, 5, 0], np.int32)
    stream = ops.IG_STREAM_ADJACENCY + 2
    v = csr.values
    out = ops.ig_perturb_values(csr, v, _t(scale), _t(sigma), _t(sample, np.int32), ids, stream, SEED)
    vals = _np(v)
    ref = np.empty_like(vals)
    for b in range(5):
        e0, e1 = rp[b * M], rp[(b + 1) * M]
        z = SO.noise(SEED, stream, ids[b], int(sample[b]), 1, int(e1 - e0))[0]
        ref[e0:e1] = SO.add_perturbation(vals[e0:e1], float(scale[b]), z, float(sigma[b]))
    FB.check("perturb values", _np(out), ref)
    # the two stored copies of (1, 2) in graph 2 carry their own noise
    e0 = rp[2 * M]
    assert len({float(x) for x in (out[e0:e0 + 3] - v[e0:e0 + 3] * 0.25).cpu()}) == 3
    clean = ops.ig_perturb_values(csr, v, _t(scale), 0.0, _t(sample, np.int32), ids, stream, SEED)
    assert torch.equal(clean, v * _t(scale)[torch.as_tensor(np.repeat(np.arange(5), per), device="cuda")])
    empty = BatchedCSR.from_arrays([], [], [], [], 2, M, M, device="cuda")
    assert ops.ig_perturb_values(empty, empty.values, _t(scale[:2]), 0.1, [0, 0], [0, 1], stream, SEED).numel() == 0


# ---- the noisy conv-pool forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,k,p", [(37, 4, 4), (70, 3, 3), (129, 4, 2)])
def test_perturbed_forward_matches_oracle(L, k, p):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(L)
    C, rep, E = 3, 5, 6
    ids = [4, 0, 9]
    ttok, table, w, b, tok = conv_case(rng, C, L, E, k, p)
    scale = np.tile(np.array([0.0, 0.25, 0.5, 1.0, 0.8], np.float32), C)
    sigma = np.tile(np.array([0.0, 0.1, 0.0, 0.1, 0.1], np.float32), C)
    sample = np.tile(np.array([0, 0, 1, 2, 7], np.int32), C)
    args = (ttok, _t(table), _t(w), _t(b), p, _t(scale), rep)
    pooled, arg = ops.seq_conv_pool_perturbed(*args, _t(sigma), _t(sample, np.int32), ids, SEED, argmax=True)
    emb = np.empty((C * rep, L, E))
    for r in range(C * rep):
        z = SO.noise(SEED, SO.STREAM_SEQUENCE, ids[r // rep], int(sample[r]), L, E)
        emb[r] = SO.add_perturbation(table[tok[r // rep]].astype(np.float64), float(scale[r]), z, float(sigma[r]))
    ref, ref_arg, _ = IG.conv_pool_fwd_emb(emb, w, b, p)
    FB.check("perturbed conv-pool L=%d k=%d p=%d pooled" % (L, k, p), _np(pooled), ref)
    a = arg.cpu().numpy()
    live = ref > 1e-4
    assert np.array_equal(a[live], ref_arg[live]) and np.all(a[ref == 0] == 0xFF)
    # the noise reaches the output, and only the rows that carry it
    clean, clean_arg = ops.seq_conv_pool_scaled(*args, argmax=True)
    noisy_rows = torch.as_tensor(sigma != 0, device="cuda")
    assert torch.equal(pooled[~noisy_rows], clean[~noisy_rows]) and torch.equal(arg[~noisy_rows], clean_arg[~noisy_rows])
    assert all(not torch.equal(pooled[r], clean[r]) for r in np.nonzero(sigma)[0] if scale[r] > 0)
    # sigma = 0 everywhere: the scaled kernel's bytes; one copy at scale 1: the training kernel's
    zero, zero_arg = ops.seq_conv_pool_perturbed(*args, 0.0, _t(sample, np.int32), ids, SEED, argmax=True)
    assert torch.equal(zero, clean) and torch.equal(zero_arg, clean_arg)
    one, _ = ops.seq_conv_pool_perturbed(ttok, _t(table), _t(w), _t(b), p, torch.ones(C, device="cuda"), 1, 0.0, [0] * C, ids, SEED)
    assert torch.equal(one, ops.seq_conv_pool(ttok, _t(table), _t(w), _t(b), p))
    again, again_arg = ops.seq_conv_pool_perturbed(*args, _t(sigma), _t(sample, np.int32), ids, SEED, argmax=True)
    assert torch.equal(pooled, again) and torch.equal(arg, again_arg)


# ---- the whole attribution ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g7():
    return g7_case()


def _device_entries(dataset, cid):
    """Per channel the [nnz, 2] stored entries of compound cid in the CSR order of the device batch (what the noise of the
    values is indexed by)."""
    adj, _ = dataset.batch([cid])
    out = []
    for c in adj.channels:
        rp = c.rowptr.cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))
        out.append(np.stack([rows, c.cv[:, 0].cpu().numpy().astype(np.int64)], 1))
    return out


def _compare(res, p, dataset, channels, features, tok_np, table, N, D, modal, method, tag):
    for r in res:
        cid = r["compound_id"]
        x, A, Sm, emb = oracle_inputs(channels, features, tok_np, table, cid, N)
        mask = np.zeros(2)
        mask[r["target_label"]] = 1.0
        ref = SO.smooth(p, x, A, Sm, emb, mask, D, modal, method, NS, SEED, cid, entries=_device_entries(dataset, cid))
        for m in (IG.MODALS if modal == "all" else (modal,)):
            FB.check("%s %s_IG" % (tag, m), r[m + "_IG"], ref[m + "_IG"])
        FB.check("%s check_score" % tag, r["check_score"], ref["check_score"], absolute=True)
        FB.check("%s sum_of_IG" % tag, r["sum_of_IG"], ref["sum_of_IG"], absolute=True)


@pytest.mark.parametrize("modal", ["all", "features", "adjs", "embedded_layer"])
@pytest.mark.parametrize("method", ["smooth_grad", "smooth_ig"])
def test_smooth_on_g7_matches_oracle(g7, modal, method):
    from kgcn_amd import visualization as V
    g, channels, dataset, tokens, model = g7
    D = 16
    res = V.multimodal_integrated_gradients(model, None, dataset, tokens, labels=g["label"], divide_number=D, modal=modal,
                                            method=method, sequence_symbol=g["sequence"], noise_scale=0.1, seed=SEED)
    assert len(res) == 5
    keys = set(IG.MODALS if modal == "all" else (modal,))
    assert keys | {m + "_IG" for m in keys} | set(V.DUMP_KEYS_FIXED) | {"amino_acid_seq"} <= set(V.dump_record(res[0]))
    _compare(res, multimodal_params(model), dataset, channels, g["feature"], g["sequence"], _np(model.sequence.embeddings), 3, D, modal,
             method, "g7 %s %s" % (method, modal))


def test_smooth_ig_at_cpi_shape_matches_oracle():
    import torch
    from oracle import kgcn_oracle as K
    from kgcn_amd import data_util as D, models, visualization as V
    C, N, F, L, S, Dn = 2, 50, 81, 700, 25, 8
    rng = np.random.default_rng(7)
    adjs = K.synth_mol_graphs(rng, C, N, 3)
    channels = [D.FlatAdjacency.from_coo_list([a[0] for a in adjs], N)]
    x = (rng.standard_normal((C, N, F)) * 0.3).astype(np.float32)
    tok = rng.integers(0, S, size=(C, L)).astype(np.int32)
    dataset = D.DeviceGraphDataset(channels, x, device="cuda")
    torch.manual_seed(2)
    model = models.MultimodalGCN(S, embedding_dim=25, label_dim=2).cuda()
    with torch.no_grad():
        model.sequence.embeddings.uniform_(-1.0, 1.0)
    ttok = torch.as_tensor(tok, device="cuda")
    adj, xx = dataset.batch(np.arange(C))
    model(xx, adj, sequences=ttok)
    with torch.no_grad():                              # 50-atom read-outs saturate the softmax at the initial scale
        model.out.kernel.mul_(0.02)
    res = V.multimodal_integrated_gradients(model, None, dataset, ttok, divide_number=Dn, method="smooth_ig", chunk=1, seed=SEED)
    assert min(abs(r["check_score"]) for r in res) > 1e-4          # an unsaturated prediction: the attribution is not all zero
    _compare(res, multimodal_params(model), dataset, channels, x, tok, _np(model.sequence.embeddings), N, Dn, "all", "smooth_ig",
             "CPI shape smooth_ig all")


def test_invariants_of_the_smooth_attribution(g7):
    import torch
    from kgcn_amd import visualization as V
    g, channels, dataset, tokens, model = g7
    for method in V.SMOOTH_METHODS:
        kw = dict(labels=g["label"], divide_number=6, modal="all", method=method, seed=SEED)
        a = V.multimodal_integrated_gradients(model, None, dataset, tokens, **kw)
        by_id = {r["compound_id"]: r for r in a}
        # chunking and compound subsets see the same noise: identical arrays
        c = V.multimodal_integrated_gradients(model, None, dataset, tokens, chunk=2, **kw)
        sub = V.multimodal_integrated_gradients(model, None, dataset, tokens, compounds=[3, 1], **kw)
        assert [r["compound_id"] for r in sub] == [3, 1]
        for rc in c + sub:
            ra = by_id[rc["compound_id"]]
            for m in IG.MODALS:
                assert np.array_equal(ra[m + "_IG"], rc[m + "_IG"]), (method, m)
            assert ra["check_score"] == rc["check_score"] and ra["sum_of_IG"] == rc["sum_of_IG"]
        # a second run is byte-identical, another seed is not
        d = V.multimodal_integrated_gradients(model, None, dataset, tokens, **kw)
        for ra, rd in zip(a, d):
            for k in ra:
                assert np.array_equal(np.asarray(ra[k]), np.asarray(rd[k])), k
        e = V.multimodal_integrated_gradients(model, None, dataset, tokens, **dict(kw, seed=SEED + 1))
        for ra, re_ in zip(a, e):
            assert ra["check_score"] == re_["check_score"]                          # the clean copies
            assert any(not np.array_equal(ra[m + "_IG"], re_[m + "_IG"]) for m in IG.MODALS), method
        # the per-step loop, held as the clean path's test holds it: every array relative to its maximum and sum_of_IG relative to
        # itself, all to 1e-6
        b = V.multimodal_integrated_gradients(model, None, dataset, tokens, batched=False, **kw)
        worst = {}
        for ra, rb in zip(a, b):
            for m in IG.MODALS:
                worst[m] = max(worst.get(m, 0.0), rel_err(ra[m + "_IG"], rb[m + "_IG"]))
            worst["sum_of_IG"] = max(worst.get("sum_of_IG", 0.0),
                                     abs(ra["sum_of_IG"] - rb["sum_of_IG"]) / max(1e-30, abs(rb["sum_of_IG"])))
            assert ra["check_score"] == rb["check_score"]
        print("%s batched vs loop: %s" % (method, "  ".join("%s %.2e" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1e-6
    assert all(p.requires_grad for p in model.parameters())               # the attribution leaves the parameters trainable
    with pytest.raises(TypeError):
        V.multimodal_integrated_gradients(torch.nn.Linear(2, 2), None, dataset, tokens, method="smooth_grad")


@pytest.mark.parametrize("smooth,clean", [("smooth_grad", "grad"), ("smooth_ig", "ig")])
def test_zero_noise_is_the_clean_method(g7, smooth, clean):
    from kgcn_amd import visualization as V
    g, channels, dataset, tokens, model = g7
    kw = dict(labels=g["label"], divide_number=6, modal="all")
    a = V.multimodal_integrated_gradients(model, None, dataset, tokens, method=smooth, noise_scale=0.0, **kw)
    b = V.multimodal_integrated_gradients(model, None, dataset, tokens, method=clean, **kw)
    worst = 0.0
    for ra, rb in zip(a, b):
        for m in IG.MODALS:
            worst = max(worst, rel_err(ra[m + "_IG"], rb[m + "_IG"]))
        assert ra["check_score"] == rb["check_score"]
    print("%s at noise_scale 0 vs %s: max rel err %.2e" % (smooth, clean, worst))
    assert worst <= 1e-6


# ---- the generic loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["smooth_grad", "smooth_ig"])
def test_generic_integrated_gradients_match_the_oracle_loop(method):
    import torch
    from oracle import kgcn_oracle as K
    from kgcn_amd import BatchedAdjacency, layers, visualization as V
    rng = np.random.default_rng(23)
    B, N, F, Dh, D = 2, 10, 3, 8, 6
    adjs = K.normalize_adj(K.synth_mol_graphs(rng, B, N, 2))
    x = rng.standard_normal((B, N, F)).astype(np.float32)
    conv = layers.GraphConv(Dh, 1).to("cuda")
    adj = BatchedAdjacency.from_adjs(adjs, n_nodes=N, device="cuda")
    conv(_t(x), adj=adj)
    w, b = [_np(conv.w[0])], [_np(conv.bias[0])]
    ro = rng.standard_normal(Dh).astype(np.float32)
    tro = _t(ro)

    def score_fn(feat, a):
        return (layers.GraphGather()(torch.sigmoid(conv(feat, adj=a))) @ tro).sum()

    res = V.integrated_gradients(score_fn, _t(x), adj, divide_number=D, method=method, noise_scale=0.1, seed=SEED)
    x64 = x.astype(np.float64)
    vals = [np.asarray(adjs[g][0][1], np.float64) for g in range(B)]
    ig_x, ig_a = np.zeros_like(x64), [np.zeros(len(v)) for v in vals]
    for k in range(D):
        sc = 1.0 if method == "smooth_grad" else (k + 1) / float(D)
        xs = np.stack([SO.add_perturbation(x64[g], sc, SO.noise(SEED, SO.STREAM_FEATURES, g, k, N, F), NS) for g in range(B)])
        adjs_s = [[(adjs[g][0][0], SO.add_perturbation(vals[g], sc, SO.noise(SEED, SO.STREAM_ADJACENCY, g, k, 1, len(vals[g]))[0], NS),
                    adjs[g][0][2])] for g in range(B)]
        dx, dvals = K.probe_score_grads(xs, adjs_s, w, b, ro)
        ig_x += dx / D if method == "smooth_grad" else dx * x64 / D
        for g in range(B):
            ig_a[g] += dvals[g][0] / D if method == "smooth_grad" else dvals[g][0] * vals[g] / D
    # the reference's COO order is row-major here, = the CSR order of the container
    FB.check("generic %s features" % method, _np(res["features"]), ig_x)
    FB.check("generic %s adjs" % method, _np(res["adjs"]), np.concatenate(ig_a))
    clean = V.integrated_gradients(score_fn, _t(x), adj, divide_number=D, method="grad")
    assert res["start_score"] == clean["start_score"] and res["end_score"] == clean["end_score"]


# ---- the three staging modes of the one conv-pool forward, through the C ABI ------------------------------------------------
def test_convpool_staging_modes_agree_bit_for_bit_through_the_c_abi():
    """The equalities include/kgcn_hip.h promises, at the smallest shape in which every staging path differs: C = 2 token rows
    x rep = 2; E = 5 (E4 = 8: the tail of the Philox block and the zero columns); k = 4 (asymmetric SAME padding); F = 50 (idle
    lanes); p = 2, L = 37 -> T = 18 > 16: two tiles per sequence, whose halo rows the neighbouring tile draws again; S = 7.
    Pooled values and arg-max bytes go into buffers bracketed by sentinels."""
    import torch
    from kgcn_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    C, rep, E, k, F, p, L, S = 2, 2, 5, 4, 50, 2, 37, 7
    B, T, GUARD = C * rep, L // p, 256
    rng = np.random.default_rng(11)
    tok = _t(rng.integers(0, S, (C, L)), np.int32)
    table, w, bias = _t(rng.standard_normal((S, E))), _t(rng.standard_normal((k, E, F)) * 0.3), _t(rng.standard_normal(F) * 0.1)
    scale, one = _t([0.0, 0.5, 1.0, 0.75]), _t(np.ones(C))
    zero, sigma = _t(np.zeros(B)), _t([0.1, 0.0, 0.2, 0.1])
    sample, ids = _t([0, 1, 0, 3], np.int32), _t([5, 2], np.int32)
    conv = (L, ptr(table), S, E, ptr(w), ptr(bias), k, F, p)
    guarded = []

    def run(fn, rows, *head):
        bufs = []
        for dtype, fill in ((torch.float32, 1.2345e30), (torch.uint8, 0xA5)):
            big = torch.full((rows * T * F + 2 * GUARD,), fill, device="cuda", dtype=dtype)
            guarded.append((big, fill))
            bufs.append(big[GUARD:-GUARD])
        _lib.check(getattr(lib, fn)(ptr(tok), rows, *head, *conv, ptr(bufs[0]), ptr(bufs[1]), _lib.current_stream()), fn)
        return bufs

    def same(a, b):
        return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])

    noise = lambda sg: (rep, ptr(scale), ptr(sg), ptr(sample), ptr(ids), SEED)
    scaled = run("kgcn_seq_convpool_scaled_fwd_f32", B, rep, ptr(scale))
    assert same(run("kgcn_seq_convpool_perturbed_fwd_f32", B, *noise(zero)), scaled), "sigma = 0 is not the scaled forward"
    plain = run("kgcn_seq_convpool_fwd_f32", C)
    assert same(run("kgcn_seq_convpool_scaled_fwd_f32", C, 1, ptr(one)), plain), "scale = 1, rep = 1 is not the plain forward"
    noisy = run("kgcn_seq_convpool_perturbed_fwd_f32", B, *noise(sigma))
    assert same(run("kgcn_seq_convpool_perturbed_fwd_f32", B, *noise(sigma)), noisy), "the same draw differs between two launches"
    assert not same(noisy, scaled) and float(plain[0].max()) > 0.0                # noise was drawn; relu passed something
    torch.cuda.synchronize()
    for big, fill in guarded:
        edge = torch.full((GUARD,), fill, device="cuda", dtype=big.dtype)
        assert torch.equal(big[:GUARD], edge) and torch.equal(big[-GUARD:], edge), "wrote outside its buffer"


# ---- limits and argument errors -------------------------------------------------------------------------------------------
def test_limits_and_argument_errors_raise_before_launch(g7):
    import torch
    from kgcn_amd import _lib, ops, visualization as V
    g, channels, dataset, tokens, model = g7
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            V.multimodal_integrated_gradients(model, None, dataset, tokens, method="smooth_grad", noise_scale=bad)
    with pytest.raises(ValueError):
        V.multimodal_integrated_gradients(model, None, dataset, tokens, method="smooth")
    with pytest.raises(ValueError):
        V.multimodal_integrated_gradients(model, None, dataset, tokens, method="smooth_ig", divide_number=0)
    E = _lib.KgcnHipError
    x = torch.zeros((2, 3, 5), device="cuda")
    ones, smp = torch.ones(4, device="cuda"), [0, 1, 0, 1]
    with pytest.raises(E):
        ops.ig_perturb(x, ones, -0.1, smp, [0, 1], 2, 0, SEED)                          # negative noise scale
    with pytest.raises(E):
        ops.ig_perturb(x, ones, 0.1, smp, [0, 1, 2], 2, 0, SEED)                        # three ids for two compounds
    with pytest.raises(E):
        ops.ig_perturb(x, ones, 0.1, smp[:3], [0, 1], 2, 0, SEED)                       # three sample numbers for four rows
    with pytest.raises(E):
        ops.ig_perturb(x, ones, 0.1, smp, [0, 1], 3, 0, SEED)                           # four rows are not 2 x 3 copies
    with pytest.raises(E):
        ops.ig_perturb(x, ones, 0.1, smp, [0, -1], 2, 0, SEED)                          # a negative id
    with pytest.raises(E):
        ops.ig_perturb(x, ones, torch.full((3,), 0.1, device="cuda"), smp, [0, 1], 2, 0, SEED)
    from kgcn_amd.batched_csr import BatchedCSR
    csr = BatchedCSR.from_arrays([0, 1], [0, 1], [1, 0], [1.0, 2.0], 2, 3, 3, device="cuda")
    with pytest.raises(E):
        ops.ig_perturb_values(csr, csr.values, ones, 0.1, smp, [0, 1, 2, 3], 1, SEED)   # four scales for two graphs
    with pytest.raises(E):
        ops.ig_perturb_values(csr, csr.values, ones[:2], 0.1, [0, 1], [0], 1, SEED)     # ids are per graph
    with pytest.raises(E):
        ops.ig_perturb_values(csr, csr.values[:1], ones[:2], 0.1, [0, 1], [0, 1], 1, SEED)
    tok = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    table, w, bias = torch.zeros((4, 8), device="cuda"), torch.zeros((4, 8, 8), device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(E):
        ops.seq_conv_pool_perturbed(tok, table, w, bias, 4, ones, 2, 0.1, smp, [0], SEED)          # one id for two token rows
    with pytest.raises(E):
        ops.seq_conv_pool_perturbed(tok, table, w, bias, 4, ones, 2, 0.1, smp[:2], [0, 1], SEED)   # two sample numbers, four rows
    with pytest.raises(E):
        ops.seq_conv_pool_perturbed(tok, table, w, bias, 4, ones, 4, 0.1, smp, [0, 1], SEED)       # four rows are not 2 x 4 copies
    with pytest.raises(E):
        ops.seq_conv_pool_perturbed(tok, table, w, bias, 4, ones, 2, -1.0, smp, [0, 1], SEED)
    with pytest.raises(E):                                                                          # k = 9 > 8
        ops.seq_conv_pool_perturbed(tok, table, torch.zeros((9, 8, 8), device="cuda"), bias, 4, ones, 2, 0.1, smp, [0, 1], SEED)
    lib = _lib.lib
    assert lib.kgcn_seq_convpool_perturbed_fwd_f32(None, 4, 0, None, None, None, None, 0, 16, None, 4, 8, None, None, 4, 8, 4, None,
                                                   None, None) != 0
    assert lib.kgcn_ig_perturb_rows_f32(None, 4, 3, 2, 2, None, None, None, None, 0, 0, None, None) != 0
    assert lib.kgcn_ig_perturb_values_f32(None, 2, 3, 2, 1, None, None, None, None, None, 1, 0, None, None) != 0
