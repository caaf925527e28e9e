"""models.SeqCNN (sample_protein/sequence/cnn.py) on the GPU against tests/seqcnn_oracle.model_fwd / model_bwd at the model's real
widths (505 / 200 / 100 / 1), L = 50, B in {1, 3}: logits, both losses, every parameter gradient and the gradient with respect
to the fed embedded layer; then GraphedTrainStep on the committed fixture tests/golden/g9_seqcnn.npz.

Bounds (max |err| / max |ref| per tensor) come from tests/golden/seqcnn_bounds.json.  As in test_gpu_conv1d.py, the parameters
of a case are drawn from the first seed for which the oracle's fp64 values are well conditioned: every relu pre-activation (the
three conv layers and the second batch normalisation) and every pool window's runner-up farther from the decision than the
forward bound times the layer's largest pre-activation; the test asserts that before it compares anything.

The closing tanh layer hands its backward the fp32 OUTPUT y, and the derivative 1 - y^2 is formed from it (the convention of
ops.activation_backward).  An error d in y moves 1 - y^2 by 2 |y| d, and d is at least the rounding of y (6e-8 near 1; the
kernel's tanh is good to a few ulp, about 2.4e-7): where every output of the layer is saturated, T3 = 2 positions per sequence
here, the whole gradient below it carries the relative error 2 |y| d / (1 - y^2), which at |y| = 0.999 is 2.4e-4 -- a property of
the fp32 output, not of the kernels.  So a case must also keep the tanh layer in its working range: max |y| <= TANH_MAX = 0.975,
where 2 |y| 2.4e-7 / (1 - y^2) = 9.5e-6 stays below the ceiling of the bounds (1e-5).  Asserted on the oracle like the rest."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_bounds  # noqa: E402
import seqcnn_oracle as O  # noqa: E402
from test_gpu_conv1d import well_conditioned  # noqa: E402

pytestmark = pytest.mark.gpu

FB = family_bounds.FAMILIES["seqcnn"]           # as in test_gpu_conv1d.py
S, E, L = 26, 25, 50
CLASS_WEIGHT = np.array([1.25, 5.0])
TANH_MAX = 0.975


def conditioned(c):
    """The preconditions of the module docstring on a model_fwd cache."""
    ok = all(well_conditioned(cc, FB.bound("forward"))[0] for cc in c["convs"])
    ok = ok and float(np.abs(c["n2"]).min()) > FB.bound("forward") * float(np.abs(c["n2"]).max())
    return ok and float(np.abs(c["s"]).max()) <= TANH_MAX


def _case(B, embedded):
    for seed in range(1000 * B + 500 * embedded, 1000 * B + 500 * embedded + 300):
        rng = np.random.default_rng(seed)
        p = O.init_params(rng, S, E, L)
        labels = np.eye(2, dtype=np.float32)[rng.integers(0, 2, B)]
        mask = np.ones(B, np.float32)
        if B > 1:
            mask[-1] = 0.5
        kw = dict(embedded=rng.standard_normal((B, L, E)).astype(np.float32)) if embedded else \
            dict(tokens=rng.integers(0, S - 2, (B, L)).astype(np.int32))
        c = O.model_fwd(p, labels, CLASS_WEIGHT, mask, **kw)
        if conditioned(c):
            return p, labels, mask, kw, c
    raise AssertionError("no well-conditioned seed")


def _model(p, B):
    import torch
    from kgcn_amd import models
    dev = torch.device("cuda:0")
    model = models.SeqCNN(S, embedding_dim=E, label_dim=2, class_weight=CLASS_WEIGHT).to(dev)
    model(None, None, sequences=torch.zeros((B, L), dtype=torch.int32, device=dev))          # lazy build
    names = model_params(model)
    with torch.no_grad():
        for k, q in names.items():
            q.copy_(torch.as_tensor(p[k], device=dev).reshape(q.shape))
    return model, names


def model_params(m):
    d = {"embeddings": m.embeddings, "w4": m.conv_out.conv_kernel, "b4": m.conv_out.conv_bias, "gamma1": m.bn1.gamma, "beta1": m.bn1.beta,
         "wh": m.hidden.kernel, "bh": m.hidden.bias, "gamma2": m.bn2.gamma, "beta2": m.bn2.beta, "wo": m.out.kernel, "bo": m.out.bias}
    for i, c in enumerate(m.convs, 1):
        d["w%d" % i], d["b%d" % i] = c.conv_kernel, c.conv_bias
    assert sorted(d) == sorted(O.PARAMS) and len(list(m.parameters())) == len(d)
    return d


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("embedded", [False, True], ids=["tokens", "embedded"])
def test_model_against_the_oracle(B, embedded):
    import torch
    from kgcn_amd import ops
    p, labels, mask, kw, c = _case(B, embedded)
    assert conditioned(c)
    g_opt, g_sum = 0.7, 0.3
    ref = O.model_bwd(c, g_opt, g_sum)
    dev = torch.device("cuda:0")
    model, names = _model(p, B)
    temb = None
    if embedded:
        temb = torch.as_tensor(kw["embedded"], device=dev).requires_grad_(True)
        logits = model(None, None, embedded=temb)
    else:
        logits = model(None, None, sequences=torch.as_tensor(kw["tokens"], device=dev))
    assert tuple(logits.shape) == (B, 2)
    cost_opt, cost_sum = model.loss(logits, torch.as_tensor(labels, device=dev), torch.as_tensor(mask, device=dev))
    root = g_opt * cost_opt + g_sum * cost_sum
    with ops.deferred_reductions(root=root):
        root.backward()
    torch.cuda.synchronize()
    FB.check("model_logits", logits.detach().cpu().numpy(), c["logits"])
    FB.hold("model_loss", max(abs(float(cost_opt) - c["cost_opt"]) / abs(c["cost_opt"]), abs(float(cost_sum) - c["cost_sum"]) / abs(c["cost_sum"])),
            figure="|ref|, the larger of cost_opt and cost_sum")
    for k, q in names.items():
        if k == "embeddings" and embedded:
            assert q.grad is None
            continue
        FB.check("model_grad", q.grad.cpu().numpy().reshape(ref[k].shape), ref[k], k)
    if embedded:
        FB.check("model_d_embedded", temb.grad.cpu().numpy(), ref["d_embedded"])


def _fixture_training(lr=1e-3, batch=8):
    import torch
    from kgcn_amd import data_util as D, models, train
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "g9_seqcnn.npz"))
    G = z["sequence"].shape[0]
    channels, _ = D.build_adjs({"dense_adj": np.tile(np.eye(2, dtype=np.float32), (G, 1, 1)), "max_node_num": 2})   # the dummy graph
    tokens, nsym = D.sequence_table({"sequence": z["sequence"], "sequence_symbol_num": z["sequence_symbol_num"]}, dev)
    dataset = D.DeviceGraphDataset(channels, np.zeros((G, 2, 2), np.float32), device=dev)
    torch.manual_seed(0)
    model = models.SeqCNN(nsym, embedding_dim=25, label_dim=2, class_weight=z["class_weight"]).to(dev)
    sb = dataset.static_batch(batch)
    seqs = sb.add_table(tokens)
    labels = sb.add_table(torch.as_tensor(z["label"], dtype=torch.float32, device=dev))
    mask = sb.add_table(torch.ones(G, device=dev))
    sb.load(np.arange(batch))
    model(sb.features, sb.adjacency, sequences=seqs)
    return model, train.TFAdam(model.parameters(), lr=lr), sb, seqs, labels, mask


def test_replays_lower_the_loss_and_equal_eager_steps():
    import torch
    from kgcn_amd import train
    batch, nbatch, epochs = 8, 4, 8                      # 32 steps over the same four batches
    model, opt, sb, seqs, labels, mask = _fixture_training(batch=batch)
    p0 = [q.detach().clone() for q in model.parameters()]
    order = [np.arange(i * batch, (i + 1) * batch) for i in range(nbatch)] * epochs
    eager = []
    for idx in order:
        sb.load(idx)
        cs, _ = train.train_step(model, opt, model.loss, sb.features, sb.adjacency, labels, mask, sequences=seqs)
        eager.append(cs)
    p_eager = [q.detach().cpu().numpy() for q in model.parameters()]
    with torch.no_grad():
        for q, q0 in zip(model.parameters(), p0):
            q.copy_(q0)
    opt2 = train.TFAdam(model.parameters(), lr=1e-3)
    step = train.GraphedTrainStep(model, opt2, model.loss, sb, labels, mask, capture_assembly=True, sequences=seqs)
    replayed = []
    for idx in order:
        sb.stage(idx)
        cs, _ = step.replay()
        replayed.append(float(cs))
    torch.cuda.synchronize()
    assert replayed == eager, (replayed[:4], eager[:4])
    for a, q in zip(p_eager, model.parameters()):
        assert np.array_equal(a, q.detach().cpu().numpy())
    first, last = sum(replayed[:nbatch]), sum(replayed[-nbatch:])
    print("SEQCNN_TRAIN cost_sum of the four batches: first epoch %.5f, last epoch %.5f" % (first, last))
    assert last < first
