"""The graph VAE on the GPU (csrc/vae.hip, ops.vae_sample / ops.vae_recon, models.GraphVAE) against the fp64 oracle of
tests/vae_oracle.py: Philox words and normals, the reparameterisation, the fused reconstruction loss, the whole model, and the
captured training step."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import vae_oracle as V  # noqa: E402
from test_vae_oracle import make_batch  # noqa: E402
from oracle import kgcn_oracle as K  # noqa: E402
from gpu_helpers import to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(1e-30, np.abs(ref).max()))


def _packed(adjs, N):
    from kgcn_amd.batched_csr import as_batched_adjacency
    return as_batched_adjacency(adjs, n_nodes=N, device="cuda")


# ---- noise ---------------------------------------------------------------------------------------------------------
def test_philox_words_bit_equal_numpy():
    import torch
    from kgcn_amd import ops
    for seed, step in ((0, 0), (99, 5), (2 ** 64 - 3, 2 ** 33 + 1)):
        st = torch.tensor(step, dtype=torch.int64, device="cuda") if step < 2 ** 63 else None
        words = ops.philox4x64_raw(seed, st, 4096, "cuda").cpu().numpy().view(np.uint64)
        ours = V.philox_blocks(seed, step, 4096)
        assert np.array_equal(words, ours)
        assert np.array_equal(words[:5], V.numpy_philox_blocks(seed, step, 5))


def test_normals_against_fp64_box_muller_and_moments():
    import torch
    from kgcn_amd import ops
    n = 1 << 20
    st = torch.tensor(12, dtype=torch.int64, device="cuda")
    z = _np(ops.normal(31, st, (n,), "cuda"))
    ref = V.noise(31, 12, (n,))
    err = np.abs(z - ref)
    # measured bound: f32 log / sqrt / sincospi of the same 24-bit uniforms, relative to max(1, |ref|)
    assert float((err / np.maximum(1.0, np.abs(ref))).max()) < 2e-6, float(err.max())
    assert abs(z.mean()) < 5e-3 and abs(z.var() - 1) < 5e-3
    assert abs((z ** 3).mean()) < 1.5e-2 and abs((z ** 4).mean() - 3) < 3e-2
    st.fill_(13)
    z2 = _np(ops.normal(31, st, (n,), "cuda"))                 # the step is read on the device at run time
    assert np.array_equal(z2, np.float32(V.noise(31, 13, (n,))).astype(np.float64)) or rel(z2, V.noise(31, 13, (n,))) < 2e-6
    assert not np.array_equal(z, z2)


# ---- reparameterisation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [True, False])
def test_sample_against_oracle(explicit):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(5)
    B, N, D = 9, 13, 64
    m = (rng.standard_normal((B, D)) * 3).astype(np.float32)
    s = (rng.standard_normal((B, D)) * 2).astype(np.float32)
    m[0, :4] = [100.0, -100.0, 130.0, -250.0]                  # at the clip limits (gradient passes) and beyond (blocked)
    s[1, 0] = np.float32(np.log(np.expm1(24.5)))                # sqrt(softplus) just below 5 (equality: the CPU oracle test)
    s[1, 1] = 40.0                                              # beyond 5: blocked
    s[2, :3] = [1e-4, -1e-4, 0.0]                               # softplus near its small end
    s[3, :2] = [-30.0, -60.0]
    step = torch.tensor(7, dtype=torch.int64, device="cuda")
    eps = rng.standard_normal((B, N, D)).astype(np.float32) if explicit else None
    eps_ref = eps if explicit else np.float32(V.noise(3, 7, (B, N, D)))
    tms = _t(np.concatenate([m, s], axis=1)).requires_grad_(True)
    kl, z1, z2 = ops.vae_sample(tms, N, None if eps is None else _t(eps), seed=3, step=step, copies=2)
    gz1, gz2, gk = rng.standard_normal((B, N, D)), rng.standard_normal((B, N, D)), rng.standard_normal(B)
    torch.autograd.backward([z1, z2, kl], [_t(gz1), _t(gz2), _t(gk)])
    zr, klr = V.sample_fwd(m, s, eps_ref)
    dm, ds = V.sample_bwd(m, s, eps_ref, np.float32(gz1) + np.float32(gz2), np.float32(gk))
    tol = TOL if explicit else 2e-5           # generated eps: the f32 Box-Muller values against fp64 ones of the same words
    assert rel(_np(z1), zr) < tol and np.array_equal(_np(z1), _np(z2))
    assert rel(_np(kl), klr) < TOL
    gm, gs = _np(tms.grad)[:, :D], _np(tms.grad)[:, D:]
    assert rel(gm, dm) < TOL, rel(gm, dm)
    assert rel(gs, ds) < tol, rel(gs, ds)
    assert gm[0, 2] == 0 and gm[0, 3] == 0 and gm[0, 0] != 0 and gm[0, 1] != 0
    assert gs[1, 1] == 0


# ---- reconstruction loss -----------------------------------------------------------------------------------------------
RECON_SHAPES = [(30, 10, 1, 3), (64, 32, 1, 16), (48, 70, 6, 100), (7, 65, 3, 5), (5, 128, 8, 8)]


def _recon_case(B, N, C, F, seed=0):
    rng = np.random.default_rng(seed + N + C)
    real = max(1, B - 3)
    adjs, x, mask = make_batch(rng, B, N, F, C, real=real, weights=True)     # self loops, non-unit values, dummies
    A = V.dense_labels(adjs, B, C, N)
    D = 64
    ys = [rng.random((B, N, D)).astype(np.float32) for _ in range(C)]
    ws = [(rng.uniform(0.05, 0.3, D) * rng.choice([-1, 1], D)).astype(np.float32) for _ in range(C)]
    xf = rng.standard_normal((B, N, F)).astype(np.float32)
    kl = rng.standard_normal(B).astype(np.float32)
    return adjs, x.astype(np.float32), mask.astype(np.float32), A, ys, ws, xf, kl


def _run_recon(adjs, N, x, mask, ys, ws, xf, kl, go=1.0, gs=0.5):
    import torch
    from kgcn_amd import ops
    tys = [_t(y).requires_grad_(True) for y in ys]
    tws = [_t(w).requires_grad_(True) for w in ws]
    txf, tkl = _t(xf).requires_grad_(True), _t(kl).requires_grad_(True)
    co, cs, cc = ops.vae_recon(_packed(adjs, N), tys, tws, txf, _t(x), _t(mask), tkl)
    torch.autograd.backward([co, cs], [torch.tensor(go, device="cuda"), torch.tensor(gs, device="cuda")])
    torch.cuda.synchronize()
    return co, cs, cc, tys, tws, txf, tkl


@pytest.mark.parametrize("B,N,C,F", RECON_SHAPES)
def test_recon_against_oracle(B, N, C, F):
    adjs, x, mask, A, ys, ws, xf, kl = _recon_case(B, N, C, F)
    res = V.recon_fwd(ys, ws, A, xf, x, mask, kl)
    co, cs, cc, tys, tws, txf, tkl = _run_recon(adjs, N, x, mask, ys, ws, xf, kl, 1.0, 0.5)
    assert rel(float(co), res["cost_opt"]) < TOL
    assert rel(float(cs), res["cost_sum"]) < TOL
    # correct_count is exact away from max_c L ~ 0; an entry within 1e-5 of 0 may flip in fp32
    Lmax = np.max(np.stack(res["L"]), axis=0)
    ties = float((mask[:, None, None] * (np.abs(Lmax) < 1e-5)).sum()) / (N * N)
    assert abs(float(cc) - res["correct_count"]) <= ties + 1e-4 * max(1.0, res["correct_count"])
    dys, dws, dxf, dkl = V.recon_bwd(ys, ws, A, xf, x, mask, 1.0, 0.5)
    for c in range(C):
        assert rel(_np(tys[c].grad), dys[c]) < TOL, (c, rel(_np(tys[c].grad), dys[c]))
        assert rel(_np(tws[c].grad), dws[c]) < TOL, (c, rel(_np(tws[c].grad), dws[c]))
    assert rel(_np(txf.grad), dxf) < TOL
    assert rel(_np(tkl.grad), dkl) < TOL


def test_recon_bitwise_reproducible():
    B, N, C, F = 48, 70, 6, 100
    case = _recon_case(B, N, C, F, seed=9)
    adjs, x, mask, A, ys, ws, xf, kl = case
    r1 = _run_recon(adjs, N, x, mask, ys, ws, xf, kl)
    r2 = _run_recon(adjs, N, x, mask, ys, ws, xf, kl)
    for a, b in zip(r1[:3], r2[:3]):
        assert float(a) == float(b)
    for c in range(C):
        assert np.array_equal(_np(r1[3][c].grad), _np(r2[3][c].grad))
        assert np.array_equal(_np(r1[4][c].grad), _np(r2[4][c].grad))
    assert np.array_equal(_np(r1[5].grad), _np(r2[5].grad))


@pytest.mark.parametrize("N,C,D", [(129, 1, 64), (10, 9, 64), (10, 1, 65)])
def test_recon_out_of_range_raises(N, C, D):
    from kgcn_amd import ops, _lib
    rng = np.random.default_rng(0)
    B, F = 2, 3
    adjs, x, mask = make_batch(rng, B, N, F, C)
    ys = [_t(rng.random((B, N, D))) for _ in range(C)]
    ws = [_t(rng.random(D)) for _ in range(C)]
    with pytest.raises(_lib.KgcnHipError, match="supported"):
        ops.vae_recon(_packed(adjs, N), ys, ws, _t(rng.random((B, N, F))), _t(x), _t(mask))


# ---- the whole model ---------------------------------------------------------------------------------------------------
def _params_of(model):
    """models.GraphVAE parameters in vae_oracle's nesting (fp64)."""
    def bn(m):
        return dict(gamma=_np(m.gamma), beta=_np(m.beta), mean=_np(m.moving_mean), var=_np(m.moving_variance))

    p = dict(conv1=([_np(w) for w in model.conv1.w], [_np(b).reshape(-1) for b in model.conv1.bias]), bn1=bn(model.bn1),
             conv2=([_np(w) for w in model.conv2.w], [_np(b).reshape(-1) for b in model.conv2.bias]), bn2=bn(model.bn2),
             dense=(_np(model.dense.kernel), _np(model.dense.bias)), mean=(_np(model.mean.kernel), _np(model.mean.bias)),
             std=(_np(model.std.kernel), _np(model.std.bias)), node=(_np(model.node_decoder.kernel), _np(model.node_decoder.bias)),
             links=[dict(d1=(_np(d.dense1.kernel), _np(d.dense1.bias)), bn=bn(d.bn), d2=(_np(d.dense2.kernel), _np(d.dense2.bias)),
                         w=_np(d.distmult.w[0])) for d in model.link_decoders])
    return p


def _grads_pairs(model, g):
    out = [("dense.kernel", model.dense.kernel, g["dense"][0]), ("dense.bias", model.dense.bias, g["dense"][1]),
           ("mean.kernel", model.mean.kernel, g["mean"][0]), ("mean.bias", model.mean.bias, g["mean"][1]),
           ("std.kernel", model.std.kernel, g["std"][0]), ("std.bias", model.std.bias, g["std"][1]),
           ("node.kernel", model.node_decoder.kernel, g["node"][0]), ("node.bias", model.node_decoder.bias, g["node"][1]),
           ("bn1.gamma", model.bn1.gamma, g["bn1"]["gamma"]), ("bn1.beta", model.bn1.beta, g["bn1"]["beta"]),
           ("bn2.gamma", model.bn2.gamma, g["bn2"]["gamma"]), ("bn2.beta", model.bn2.beta, g["bn2"]["beta"])]
    for name, conv in (("conv1", model.conv1), ("conv2", model.conv2)):
        for c in range(len(conv.w)):
            out.append(("%s.w%d" % (name, c), conv.w[c], g[name][0][c]))
            out.append(("%s.b%d" % (name, c), conv.bias[c], g[name][1][c].reshape(conv.bias[c].shape)))
    for c, (d, gq) in enumerate(zip(model.link_decoders, g["links"])):
        out += [("link%d.d1.kernel" % c, d.dense1.kernel, gq["d1"][0]), ("link%d.d1.bias" % c, d.dense1.bias, gq["d1"][1]),
                ("link%d.bn.gamma" % c, d.bn.gamma, gq["bn"]["gamma"]), ("link%d.bn.beta" % c, d.bn.beta, gq["bn"]["beta"]),
                ("link%d.d2.kernel" % c, d.dense2.kernel, gq["d2"][0]), ("link%d.d2.bias" % c, d.dense2.bias, gq["d2"][1]),
                ("link%d.w" % c, d.distmult.w[0], gq["w"])]
    return out


def _model_check(adjs, x, mask, C, seed):
    import torch
    from kgcn_amd import models
    B, N, F = x.shape
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = models.GraphVAE(F, C).cuda()
    eps = rng.standard_normal((B, N, 64)).astype(np.float32)
    model(_t(x), adjs, graph_mask=_t(mask), eps=_t(eps))                       # builds the parameters
    with torch.no_grad():                                                # non-trivial BN statistics / biases
        for mod in model.modules():
            if isinstance(mod, models.GraphBatchNormalization):
                mod.gamma.copy_(_t(1 + 0.1 * rng.standard_normal(64)))
                mod.beta.copy_(_t(0.1 * rng.standard_normal(64)))
                mod.moving_mean.copy_(_t(0.1 * rng.standard_normal(64)))
                mod.moving_variance.copy_(_t(1 + 0.2 * rng.random(64)))
    for prm in model.parameters():
        prm.grad = None
    out = model(_t(x), adjs, graph_mask=_t(mask), eps=_t(eps))
    out.backward()
    torch.cuda.synchronize()
    p = _params_of(model)
    A = V.dense_labels(adjs, B, C, N)
    res, cache = V.forward(p, np.float32(x), adjs, A, np.float64(mask), np.float32(eps))
    assert rel(float(out), res["cost_opt"]) < TOL, (float(out), res["cost_opt"])
    assert rel(float(model.cost_sum), res["cost_sum"]) < TOL
    Lmax = np.max(np.stack(res["L"]), axis=0)
    ties = float((mask[:, None, None] * (np.abs(Lmax) < 1e-5)).sum()) / (N * N)
    assert abs(float(model.correct_count) - res["correct_count"]) <= ties + 1e-4 * max(1.0, res["correct_count"])
    g = V.backward(p, cache, 1.0, 0.0)
    errs = {name: rel(_np(prm.grad), ref) for name, prm, ref in _grads_pairs(model, g)}
    worst = max(errs, key=errs.get)
    assert errs[worst] < TOL, (worst, errs[worst])
    return errs


def test_model_on_synthetic_with_dummy_tail():
    raw = np.load(os.path.join(ROOT, "tests", "golden", "g1_synthetic_raw.npz"))
    idx = np.arange(190, 200)                                            # the last batch of vae.json: 10 real + 20 dummy graphs
    B, N = 30, int(raw["max_node_num"])
    adjs = [[K.dense_to_sparse(raw["dense_adj"][i].astype(np.float32))] for i in idx]
    adjs += [[(np.zeros((0, 2), np.int32), np.zeros(0, np.float32), [N, N])] for _ in range(B - len(idx))]
    adjs = [[(a[0], a[1], [N, N]) for a in row] for row in adjs]
    x = np.zeros((B, N, raw["feature"].shape[2]), np.float32)
    x[:len(idx)] = raw["feature"][idx]
    mask = (np.arange(B) < len(idx)).astype(np.float32)
    _model_check(adjs, x, mask, 1, 0)


def test_model_zinc_shape():
    rng = np.random.default_rng(3)
    B, N, F, C = 6, 70, 20, 6
    adjs, x, mask = make_batch(rng, B, N, F, C, real=5)
    _model_check(adjs, x.astype(np.float32), mask.astype(np.float32), C, 1)


# ---- training through the captured step ------------------------------------------------------------------------------
def _setup_training(seed=0):
    import torch
    from kgcn_amd import data_util as D, models, train
    raw = np.load(os.path.join(ROOT, "tests", "golden", "g1_synthetic_raw.npz"))
    channels, _ = D.build_adjs({"dense_adj": raw["dense_adj"].astype(np.int64), "max_node_num": int(raw["max_node_num"])})
    dataset = D.DeviceGraphDataset(channels, raw["feature"], device="cuda")
    torch.manual_seed(seed)
    model = models.GraphVAE(raw["feature"].shape[2], len(channels), seed=11).cuda()
    adj0, x0 = dataset.batch(np.arange(30), 30)
    model(x0, adj0, graph_mask=torch.ones(30, device="cuda"))
    opt = train.TFAdam(model.parameters(), lr=1e-3)
    model.bind_step(opt._t_dev)
    return dataset, model, opt


def test_replayed_steps_equal_eager_steps():
    import torch
    from kgcn_amd import train
    k = 4
    batches = [np.arange(30 * i, 30 * i + 30) for i in range(k - 1)] + [np.arange(190, 200)]
    # eager
    dataset, model, opt = _setup_training()
    eager = []
    for idx in batches:
        adj, x = dataset.batch(idx, 30)
        mask = (torch.arange(30, device="cuda") < len(idx)).float()
        cs, _ = train.train_step(model, opt, model.loss, x, adj, None, mask, graph_mask=mask)
        eager.append(cs)
    p_eager = [_np(q) for q in model.parameters()]
    # replayed
    dataset, model, opt = _setup_training()
    sb = dataset.static_batch(30)
    mask = sb.add_table(torch.ones(dataset.num_graphs, device="cuda"))
    sb.load(batches[0])
    step = train.GraphedTrainStep(model, opt, model.loss, sb, mask, mask, capture_assembly=True, graph_mask=mask)
    replayed = []
    for idx in batches:
        sb.stage(idx)
        cs, _ = step.replay()
        replayed.append(float(cs))
    torch.cuda.synchronize()
    assert replayed == eager, (replayed, eager)
    for a, b in zip(p_eager, [_np(q) for q in model.parameters()]):
        assert np.array_equal(a, b)
    assert len(set(replayed)) == k


def test_no_torch_operator_inside_the_captured_step():
    import torch
    from kgcn_amd import train
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from aten_in_step import log_step
    dataset, model, opt = _setup_training()
    sb = dataset.static_batch(30)
    mask = sb.add_table(torch.ones(dataset.num_graphs, device="cuda"))
    sb.load(np.arange(30))
    step = train.GraphedTrainStep(model, opt, model.loss, sb, mask, mask, capture_assembly=True, graph_mask=mask)
    seen = log_step(step._eager)
    assert not seen, dict(seen)
