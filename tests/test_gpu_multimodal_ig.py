"""Integrated gradients of the multimodal model on the GPU (csrc/seq.hip scaled conv-pool forward and input-gradient kernel,
ops.seq_conv_pool_scaled / ops.seq_conv_pool_input_grad, visualization.multimodal_integrated_gradients) against the fp64 oracle
of tests/multimodal_ig_oracle.py.  Every comparison prints its error (max abs error / max abs reference value)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_ig_oracle as IG  # noqa: E402
from family_bounds import rel_err  # noqa: E402
from gpu_helpers import conv_case, g7_case, multimodal_params, oracle_inputs, to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.mark.parametrize("L,k,p", [(37, 4, 4), (70, 3, 3), (129, 4, 2)])
def test_scaled_forward_matches_oracle(L, k, p):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(L)
    C, rep, E = 3, 5, 6
    ttok, table, w, b, tok = conv_case(rng, C, L, E, k, p)
    scale = np.tile(np.array([0.0, 0.25, 0.5, 1.0, 0.8], np.float32), C)
    pooled, arg = ops.seq_conv_pool_scaled(ttok, _t(table), _t(w), _t(b), p, _t(scale), rep, argmax=True)
    emb = table[np.repeat(tok, rep, 0)].astype(np.float64) * scale.astype(np.float64)[:, None, None]
    ref, ref_arg, _ = IG.conv_pool_fwd_emb(emb, w, b, p)
    err = rel_err(_np(pooled), ref)
    print("scaled conv-pool L=%d k=%d p=%d: pooled %.2e" % (L, k, p, err))
    assert err <= TOL
    a = arg.cpu().numpy()
    live = ref > 1e-4
    assert np.array_equal(a[live], ref_arg[live]) and np.all(a[ref == 0] == 0xFF)
    # scale 1, one copy: bit for bit the training-path kernel
    one, _ = ops.seq_conv_pool_scaled(ttok, _t(table), _t(w), _t(b), p, torch.ones(C, device="cuda"), 1)
    assert torch.equal(one, ops.seq_conv_pool(ttok, _t(table), _t(w), _t(b), p))


@pytest.mark.parametrize("L,k,p", [(37, 4, 4), (70, 3, 3), (45, 4, 4), (700, 4, 4)])
def test_input_grad_kernel_matches_oracle(L, k, p):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(100 + L + k)
    C, rep, E = 2, 4, 25
    ttok, table, w, b, tok = conv_case(rng, C, L, E, k, p, S=25)
    scale = np.tile(np.array([0.0, 0.3, 0.7, 1.0], np.float32), C)
    pooled, arg = ops.seq_conv_pool_scaled(ttok, _t(table), _t(w), _t(b), p, _t(scale), rep, argmax=True)
    assert int((arg == 0xFF).sum()) > 0                             # relu-dead outputs (the scale-0 rows at least)
    g = rng.standard_normal(tuple(pooled.shape)).astype(np.float32)
    emb = table[np.repeat(tok, rep, 0)].astype(np.float64) * scale.astype(np.float64)[:, None, None]
    _, _, conv = IG.conv_pool_fwd_emb(emb, w, b, p)
    # the oracle routes through the kernel's own bytes (ties at fp32 resolution are not the oracle's to decide)
    a = arg.cpu().numpy()
    ref = IG.conv_pool_input_grad(conv, np.where(a == 0xFF, 0, a), w, p, g * (a != 0xFF))
    per_row = ops.seq_conv_pool_input_grad(_t(g), arg, ttok.repeat_interleave(rep, 0), _t(table), _t(w), p, 1)
    err = rel_err(_np(per_row), ref)
    wt = rng.uniform(0.1, 1.0, C * rep).astype(np.float32)
    wt[::rep] = 0.0
    summed = ops.seq_conv_pool_input_grad(_t(g), arg, ttok, _t(table), _t(w), p, rep, row_weight=_t(wt))
    host = (_np(per_row) * wt[:, None, None]).reshape(C, rep, L, E).sum(1)
    err_sum = rel_err(_np(summed), host)
    attr = ops.seq_conv_pool_input_grad(_t(g), arg, ttok, _t(table), _t(w), p, rep, row_weight=_t(wt), times_table=True)
    err_attr = rel_err(_np(attr), _np(summed) * table[tok])
    print("input gradient L=%d k=%d p=%d: per row %.2e, sum over copies %.2e, times table %.2e" % (L, k, p, err, err_sum, err_attr))
    assert err <= TOL and err_sum <= 1e-6 and err_attr <= 1e-6
    again = ops.seq_conv_pool_input_grad(_t(g), arg, ttok, _t(table), _t(w), p, rep, row_weight=_t(wt))
    assert torch.equal(summed, again)


def _compare(res, p, channels, features, tok_np, table, N, D, modal, method, tag):
    worst = {}
    for r in res:
        cid = r["compound_id"]
        x, A, Sm, emb = oracle_inputs(channels, features, tok_np, table, cid, N)
        mask = np.zeros(2)
        mask[r["target_label"]] = 1.0
        ref = IG.integrated_gradients(p, x, A, Sm, emb, mask, D, modal, method)
        for m in ((IG.MODALS) if modal == "all" else (modal,)):
            worst[m] = max(worst.get(m, 0.0), rel_err(r[m + "_IG"], ref[m + "_IG"]))
        worst["check_score"] = max(worst.get("check_score", 0.0), abs(r["check_score"] - ref["check_score"]))
        worst["sum_of_IG"] = max(worst.get("sum_of_IG", 0.0), abs(r["sum_of_IG"] - ref["sum_of_IG"]))
        assert np.allclose(r["embedded_layer"] if "embedded_layer" in r else emb, emb, atol=0)
    print("%s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in worst.items())))
    return worst


@pytest.mark.parametrize("modal", ["all", "features", "adjs", "embedded_layer"])
@pytest.mark.parametrize("method", ["ig", "grad_prod", "grad"])
def test_ig_on_g7_matches_oracle(modal, method):
    from kgcn_amd import visualization as V
    g, channels, dataset, tokens, model = g7_case()
    D = 100
    res = V.multimodal_integrated_gradients(model, None, dataset, tokens, labels=g["label"], divide_number=D, modal=modal,
                                            method=method, sequence_symbol=g["sequence"])
    assert len(res) == 5
    r0 = res[0]
    keys = {m for m in (IG.MODALS if modal == "all" else (modal,))}
    assert keys | {m + "_IG" for m in keys} | set(V.DUMP_KEYS_FIXED) | {"amino_acid_seq"} <= set(V.dump_record(r0))
    if "adjs" in keys:
        assert r0["adjs"].shape == r0["adjs_IG"].shape == (3, 3)
    if "embedded_layer" in keys:
        assert r0["embedded_layer_IG"].shape == (5, 4)
    worst = _compare(res, multimodal_params(model), channels, g["feature"], g["sequence"], _np(model.sequence.embeddings), 3, D, modal,
                     method, "g7 %s %s" % (modal, method))
    assert max(worst.values()) <= TOL


def test_ig_at_cpi_shape_matches_oracle():
    import torch
    from oracle import kgcn_oracle as K
    from kgcn_amd import data_util as D, models, visualization as V
    C, N, F, L, S, Dn = 8, 50, 81, 700, 25, 100
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
    res = V.multimodal_integrated_gradients(model, None, dataset, ttok, divide_number=Dn, chunk=3)
    assert min(abs(r["check_score"]) for r in res) > 1e-4          # an unsaturated prediction: the attribution is not all zero
    worst = _compare(res, multimodal_params(model), channels, x, tok, _np(model.sequence.embeddings), N, Dn, "all", "ig",
                     "CPI shape, C = 8, N = 50, L = 700, E = 25, D = 100")
    assert max(worst.values()) <= TOL


def test_batched_matches_the_step_loop_and_is_deterministic():
    import torch
    from kgcn_amd import visualization as V
    g, channels, dataset, tokens, model = g7_case()
    kw = dict(labels=g["label"], divide_number=10, modal="all", method="ig")
    a = V.multimodal_integrated_gradients(model, None, dataset, tokens, **kw)
    b = V.multimodal_integrated_gradients(model, None, dataset, tokens, batched=False, **kw)
    c = V.multimodal_integrated_gradients(model, None, dataset, tokens, chunk=2, **kw)
    worst = 0.0
    for ra, rb, rc in zip(a, b, c):
        for m in IG.MODALS:
            worst = max(worst, rel_err(ra[m + "_IG"], rb[m + "_IG"]))
            assert np.array_equal(ra[m + "_IG"], rc[m + "_IG"])      # chunking does not change a compound's rows
        worst = max(worst, abs(ra["sum_of_IG"] - rb["sum_of_IG"]) / max(1e-30, abs(rb["sum_of_IG"])))
        assert ra["check_score"] == rc["check_score"]
    print("batched vs loop: max rel err %.2e" % worst)
    assert worst <= 1e-6
    d = V.multimodal_integrated_gradients(model, None, dataset, tokens, **kw)
    for ra, rd in zip(a, d):
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rd[k])), k
    assert all(p.requires_grad for p in model.parameters())               # the attribution leaves the parameters trainable


def test_default_path_and_scale_one_are_bit_identical():
    import torch
    g, channels, dataset, tokens, model = g7_case()
    adj, x = dataset.batch(np.arange(5))
    with torch.no_grad():
        a = model(x, adj, sequences=tokens)
        b, _, _ = model.run(x, adj, tokens, torch.ones(5, device="cuda"), 1)
        c = model(x, adj, sequences=tokens)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_limits_raise_before_launch():
    import torch
    from kgcn_amd import _lib, ops
    tok = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    table = torch.zeros((4, 33), device="cuda")
    w = torch.zeros((4, 33, 8), device="cuda")
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_conv_pool_scaled(tok, table, w, torch.zeros(8, device="cuda"), 4, torch.ones(4, device="cuda"), 2)
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_conv_pool_input_grad(torch.zeros((4, 4, 8), device="cuda"), torch.zeros((4, 4, 8), dtype=torch.uint8, device="cuda"),
                                     tok, table, w, 4, 2)
    table, w = torch.zeros((4, 8), device="cuda"), torch.zeros((9, 8, 8), device="cuda")          # k = 9 > 8
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_conv_pool_scaled(tok, table, w, torch.zeros(8, device="cuda"), 4, torch.ones(4, device="cuda"), 2)
    w = torch.zeros((4, 8, 8), device="cuda")
    with pytest.raises(_lib.KgcnHipError):                                                        # 5 rows are not 2 x 2 copies
        ops.seq_conv_pool_scaled(tok, table, w, torch.zeros(8, device="cuda"), 4, torch.ones(5, device="cuda"), 2)
    lib = _lib.lib
    assert lib.kgcn_seq_convpool_input_grad_f32(None, 4, 3, 16, None, 4, 8, None, 4, 8, 4, None, None, None, 0, None, None) != 0
    assert lib.kgcn_seq_convpool_scaled_fwd_f32(None, 4, 0, None, 16, None, 4, 8, None, None, 4, 8, 4, None, None, None) != 0
