"""Attribution loop of the reference's visualisation, on the HIP path.

kgcn/visualization.py:187-260 (CompoundVisualizer.cal_integrated_gradients): the inputs named in
`perturbation_target` (node features and / or the values of adjacency channel 0) are scaled by k/D for
k = 1..D, the gradient of the target prediction with respect to the `ig_modal_target` inputs is taken at
every step, and IG[modal] += grad * data / D; "grad_prod" and "grad" are the one-step variants.  The
consumer of the d values gradient of the batched SpMM (kgcn/bspmm_call.py:50-55) is exactly this loop.

score_fn(features, adjacency) -> scalar tensor (e.g. one softmax probability of one graph); `adjacency`
is a kgcn_amd.BatchedAdjacency whose channel-0 values arrive as a differentiable tensor
(BatchedAdjacency.with_values), features a [B, N, F] tensor.
"""
import torch


def integrated_gradients(score_fn, features, adjacency, divide_number=100, modal=("features", "adjs"),
                         perturbation=None, method="ig"):
    """Returns {"features": [B, N, F] tensor, "adjs": [nnz] tensor in the CSR order of channel 0,
    "sum_of_ig": float, "start_score": f(scale 0), "end_score": f(scale 1)} (only the requested modals).
    For method "ig" the completeness check of the reference (:262-275) is sum_of_ig ~ end - start."""
    modal = tuple(modal)
    pert = modal if perturbation is None else tuple(perturbation)
    base_vals = [c.values for c in adjacency.channels]
    x0 = features.detach()
    ig = {}
    if "features" in modal:
        ig["features"] = torch.zeros_like(x0)
    if "adjs" in modal:
        ig["adjs"] = torch.zeros_like(base_vals[0])

    def grads_at(scale):
        x = (x0 * scale if "features" in pert else x0).clone().requires_grad_("features" in modal)
        vals = [v.clone() for v in base_vals]
        if "adjs" in pert:
            vals[0] = vals[0] * scale
        vals[0] = vals[0].requires_grad_("adjs" in modal)
        score = score_fn(x, adjacency.with_values(vals))
        wrt = ([x] if "features" in modal else []) + ([vals[0]] if "adjs" in modal else [])
        g = torch.autograd.grad(score, wrt)
        out = {}
        if "features" in modal:
            out["features"] = g[0]
        if "adjs" in modal:
            out["adjs"] = g[-1]
        return out, float(score.detach())

    data = {"features": x0, "adjs": base_vals[0]}
    if method == "ig":
        for k in range(divide_number):
            g, _ = grads_at((k + 1) / float(divide_number))
            for m in ig:
                ig[m] += g[m] * data[m] / float(divide_number)
    elif method in ("grad_prod", "grad"):
        g, _ = grads_at(1.0)
        for m in ig:
            ig[m] += g[m] * data[m] if method == "grad_prod" else g[m]
    else:
        raise ValueError("unsupported method %r (ig, grad_prod, grad)" % (method,))
    with torch.no_grad():
        xs = x0 * 0.0 if "features" in pert else x0
        vs = [v.clone() for v in base_vals]
        if "adjs" in pert:
            vs[0] = vs[0] * 0.0
        start = float(score_fn(xs, adjacency.with_values(vs)))
        end = float(score_fn(x0, adjacency.with_values(base_vals)))
    res = dict(ig)
    res["sum_of_ig"] = float(sum(v.sum() for v in ig.values()))
    res["start_score"], res["end_score"] = start, end
    return res


def values_to_dense(csr, values):
    """sparse_to_dense_core of the reference (:208): per-entry values of channel 0 -> dense [T, M, K]."""
    rp = csr.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])
    dense = torch.zeros((csr.num_graphs * csr.rows, csr.cols), device=values.device, dtype=values.dtype)
    dense.index_put_((rows, csr.cv[:, 0].long()), values, accumulate=True)
    return dense.reshape(csr.num_graphs, csr.rows, csr.cols)


# -------------------------------------------------------------------------------------------------
# the multimodal model (example_model/model_multimodal.py built with feed_embedded_layer=True, gcn.py:637-656):
# kgcn/visualization.py:22-285 (CompoundVisualizer) and :442-574 (cal_feature_IG), batched
# -------------------------------------------------------------------------------------------------
IG_MODALS = ("features", "adjs", "embedded_layer")
IG_METHODS = ("ig", "grad_prod", "grad")
IG_ROWS_PER_CHUNK = 8192          # rows (compounds x copies) per forward + backward: the LSTM stash is 6 H T floats a row


def ig_scales(method, divide_number):
    """(scales, weights) of the copies of one compound.  'ig': k / D for k = 0 .. D, row 0 gives start_score with weight 0, rows
    1 .. D are the IG steps of :195-205 with weight 1 / D, row D gives end_score.  'grad_prod' / 'grad': scales 0 and 1, the
    gradient of the scale-1 row with weight 1 (:206-231)."""
    if method == "ig":
        D = int(divide_number)
        if D < 1:
            raise ValueError("divide_number must be >= 1")
        return [k / float(D) for k in range(D + 1)], [0.0] + [1.0 / D] * D
    if method in ("grad_prod", "grad"):
        return [0.0, 1.0], [0.0, 1.0]
    raise ValueError("unsupported method %r (%s; smooth_grad / smooth_ig draw host noise and are not supported)"
                     % (method, ", ".join(IG_METHODS)))


def ig_modal_targets(modal):
    """:58-71, 552-553: the same set is the IG target and the perturbation target."""
    if modal == "all":
        return IG_MODALS
    if modal not in IG_MODALS:
        raise ValueError("modal must be 'all' or one of %s, got %r" % (", ".join(IG_MODALS), modal))
    return (modal,)


def select_label_target(prediction, label_target, true_label=None):
    """:502-529 for one compound: prediction = softmax output [K] of the unscaled pass -> (target_index, target_score, class mask
    [K]) or None when 'correct' / 'uncorrect' skips the compound.  'all' targets the sum over classes."""
    import numpy as np
    pred = np.asarray(prediction, np.float64).reshape(-1)
    K = pred.shape[0]
    top = int(np.argmax(pred))
    if label_target in ("label", "correct", "uncorrect") and true_label is None:
        raise ValueError("label_target %r needs the labels" % (label_target,))
    if label_target == "all":
        return "all", float(pred.sum()), np.ones(K, np.float32)
    if label_target == "max":
        idx = top
    elif label_target == "correct":
        if top != int(true_label):
            return None
        idx = top
    elif label_target == "uncorrect":
        if top == int(true_label):
            return None
        idx = top
    elif label_target == "label":
        idx = int(true_label)
    else:
        idx = int(label_target)
    if not 0 <= idx < K:
        raise ValueError("target label %d outside 0..%d" % (idx, K - 1))
    mask = np.zeros(K, np.float32)
    mask[idx] = 1.0
    return idx, float(pred[idx]), mask


def assay_string(prediction, target_index):
    """:531-537: the assay part of the file name."""
    import numpy as np
    pred = np.asarray(prediction).reshape(-1)
    if pred.shape[0] > 2:
        return "class%s" % (target_index,)
    if pred.shape[0] == 2:
        return "active" if pred[1] > 0.5 else "inactive"
    return "active" if pred[0] > 0.5 else "inactive"


def ig_filename(header, compound_id, assay, modal, task=0):
    """:558 the name of one compound's dump."""
    return "%s_%04d_task_%d_%s_%s_scaling.jbl" % (header, int(compound_id), int(task), assay, modal)


DUMP_KEYS_FIXED = ("check_score", "sum_of_IG", "mol", "mol_smiles", "mol_id", "prediction_score", "target_label", "true_label")


def dump_record(result):
    """The dict CompoundVisualizer.dump writes (:133-160) for one result of multimodal_integrated_gradients."""
    return {k: v for k, v in result.items() if k not in ("compound_id", "assay")}


def _entry_graphs(csr):
    """Graph index of every stored entry of a batched CSR, in CSR order."""
    rp = csr.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])
    return torch.div(rows, csr.rows, rounding_mode="floor")


def _attribute(model, dataset, tokens, ids, scales, weights, targets, masks, method, table, conv_w, pool):
    """One forward + backward over len(ids) compounds x len(scales) copies -> per compound: IG arrays (unmultiplied by the data
    for 'grad'), start and end score.  masks [C, K] selects the target class(es) of each compound."""
    ids = [int(i) for i in ids]
    C, rep = len(ids), len(scales)
    dev = dataset.features.device
    sel = [i for i in ids for _ in range(rep)]
    adj, x = dataset.batch(sel)
    sc = torch.tensor(scales, dtype=torch.float32, device=dev).repeat(C)
    wt = torch.tensor(weights, dtype=torch.float32, device=dev).repeat(C)
    ones = torch.ones_like(sc)
    N, F = x.shape[1], x.shape[2]
    x_in = (x * sc.view(-1, 1, 1) if "features" in targets else x).requires_grad_("features" in targets)
    adj_in, v0 = adj, None
    if "adjs" in targets:                       # kgcn/feed.py:116-121: the values of every channel are scaled
        vals = [c.values * sc[_entry_graphs(c)] for c in adj.channels]
        v0 = vals[0].requires_grad_(True)
        adj_in = adj.with_values(vals)
    emb = "embedded_layer" in targets
    tok = tokens[torch.as_tensor(ids, device=tokens.device)]
    logits, pooled, arg = model.run(x_in, adj_in, tok, sc if emb else ones, rep, input_grad=emb)
    score = (torch.softmax(logits, dim=1) * torch.as_tensor(masks, device=dev).repeat_interleave(rep, 0)).sum(1)
    wrt = ([x_in] if "features" in targets else []) + ([v0] if "adjs" in targets else []) + ([pooled] if emb else [])
    grads = list(torch.autograd.grad(score.sum(), wrt))
    out = {}
    wv = wt.view(C, rep)
    if "features" in targets:
        g = grads.pop(0)
        ig = (g.view(C, rep, N, F) * wv.view(C, rep, 1, 1)).sum(1)
        out["features"] = ig if method == "grad" else ig * x.view(C, rep, N, F)[:, 0]
    if "adjs" in targets:
        g = grads.pop(0)
        c0 = adj.channels[0]
        dense_g = values_to_dense(c0, g).view(C, rep, c0.rows, c0.cols)
        ig = (dense_g * wv.view(C, rep, 1, 1)).sum(1)
        data = values_to_dense(c0, c0.values).view(C, rep, c0.rows, c0.cols)[:, 0]
        out["adjs"] = ig if method == "grad" else ig * data
        out["adjs_data"] = data
    if emb:
        from . import ops
        out["embedded_layer"] = ops.seq_conv_pool_input_grad(grads.pop(0), arg, tok, table, conv_w, pool, rep, row_weight=wt,
                                                             times_table=method != "grad")
    s = score.detach().view(C, rep)
    out["start"], out["end"] = s[:, 0], s[:, rep - 1]
    return out


def multimodal_integrated_gradients(model, features, adjacency, tokens, labels=None, divide_number=100, modal="all", method="ig",
                                    label_target="max", chunk=None, compounds=None, sequence_symbol=None, batched=True):
    """Integrated gradients of models.MultimodalGCN (kgcn visualize on example_model/model_multimodal.py, cal_feature_IG and
    CompoundVisualizer of kgcn/visualization.py) -> one dict per visualised compound with the keys the reference dumps:
    features [N, F], adjs [N, N] (channel 0, dense), embedded_layer [L, E] and their *_IG arrays (the modals named by `modal`),
    check_score (end - start), sum_of_IG, prediction_score, target_label, true_label, mol / mol_smiles / mol_id (None: no RDKit),
    amino_acid_seq (when sequence_symbol is given) -- plus compound_id and assay (dump_record drops them; ig_filename uses them).

    features [G, N, F] and adjacency (the channels of data_util.build_adjs), or a data_util.DeviceGraphDataset as `adjacency`
    (features None); tokens int32 [G, L] device tensor (data_util.sequence_table); labels [G, K] (needed by label_target 'label',
    'correct', 'uncorrect').  The target class comes from an unscaled forward pass, the score is its softmax probability.
    The D + 1 scaled copies of every compound (ig_scales) run as batch rows of ONE forward and ONE backward, `chunk` compounds
    (default IG_ROWS_PER_CHUNK // (D + 1)) at a time; this is valid only because the model mixes no rows, and any other model is
    refused.  The embedded-sequence attribution comes from the HIP input-gradient kernel (ops.seq_conv_pool_input_grad), which
    sums the copies in order.  batched=False runs the reference's loop instead: one batch-1 pass per compound and step through the
    same ops, summed on the host in step order."""
    import numpy as np
    import string
    from . import models
    from .data_util import DeviceGraphDataset
    if not isinstance(model, models.MultimodalGCN) or not getattr(model, "ROW_INDEPENDENT", False):
        raise TypeError("multimodal_integrated_gradients batches the scaled copies as rows: it needs a model whose rows never "
                        "mix (models.MultimodalGCN), got %s" % type(model).__name__)
    targets = ig_modal_targets(modal)
    scales, weights = ig_scales(method, divide_number)
    if isinstance(adjacency, DeviceGraphDataset):
        dataset = adjacency
    else:
        dataset = DeviceGraphDataset(adjacency, features.detach().cpu().numpy() if torch.is_tensor(features) else features,
                                     device=tokens.device)
    if dataset.features is None:
        raise ValueError("the dataset carries no node features")
    G = dataset.num_graphs
    if tokens.shape[0] != G:
        raise ValueError("%d token rows for %d graphs" % (tokens.shape[0], G))
    ids = list(range(G)) if compounds is None else [int(i) for i in compounds]
    lab = None if labels is None else np.asarray(labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels)
    rep = len(scales)
    chunk = max(1, IG_ROWS_PER_CHUNK // rep) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    seqm = model.sequence
    table, conv_w, pool = seqm.embeddings.detach(), seqm.conv_kernel.detach(), seqm.pool
    # the unscaled pass: the prediction the target class is read from (:479-485)
    preds = []
    with torch.no_grad():
        for i in range(0, len(ids), chunk):
            part = ids[i:i + chunk]
            adj, x = dataset.batch(part)
            preds.append(torch.softmax(model(x, adj, sequences=tokens[torch.as_tensor(part, device=tokens.device)]), 1).cpu().numpy())
    preds = np.concatenate(preds) if preds else np.zeros((0, 0), np.float32)
    jobs = []
    for j, cid in enumerate(ids):
        true_label = None if lab is None else int(np.argmax(lab[cid]))
        sel = select_label_target(preds[j], label_target, true_label)
        if sel is not None:
            jobs.append((cid, preds[j], true_label) + sel)
    frozen = [(p, p.requires_grad) for p in model.parameters()]
    res = {}
    try:
        for p, _ in frozen:
            p.requires_grad_(False)
        if batched:
            for i in range(0, len(jobs), chunk):
                part = jobs[i:i + chunk]
                out = _attribute(model, dataset, tokens, [j[0] for j in part], scales, weights, targets,
                                 np.stack([j[5] for j in part]), method, table, conv_w, pool)
                for k, j in enumerate(part):
                    res[j[0]] = {m: out[m][k] for m in out if m not in ("start", "end")}
                    res[j[0]]["start"], res[j[0]]["end"] = float(out["start"][k]), float(out["end"][k])
        else:
            for j in jobs:
                acc = {}
                for s, w in zip(scales, weights):
                    out = _attribute(model, dataset, tokens, [j[0]], [s], [w], targets, j[5][None], method, table, conv_w, pool)
                    for m in out:
                        if m in ("start", "end"):
                            continue
                        acc[m] = out[m][0] if m not in acc or m == "adjs_data" else acc[m] + out[m][0]
                    if s == scales[0]:
                        start = float(out["start"][0])
                    if s == scales[-1]:
                        end = float(out["end"][0])
                acc["start"], acc["end"] = start, end
                res[j[0]] = acc
    finally:
        for p, r in frozen:
            p.requires_grad_(r)
    results = []
    for cid, pred, true_label, tidx, tscore, _ in jobs:
        r = res[cid]
        rec = {"compound_id": cid, "assay": assay_string(pred, tidx)}
        if sequence_symbol is not None:
            rec["amino_acid_seq"] = "".join(string.ascii_uppercase[int(t)] for t in np.asarray(sequence_symbol[cid]).reshape(-1))
        data = {"features": lambda: dataset.features[cid].cpu().numpy(),
                "adjs": lambda: r["adjs_data"].cpu().numpy(),
                "embedded_layer": lambda: table[tokens[cid].long()].cpu().numpy()}
        total = 0.0
        for m in targets:
            rec[m] = data[m]()
            rec[m + "_IG"] = r[m].detach().cpu().numpy()
            total += float(rec[m + "_IG"].astype(np.float64).sum())
        rec["check_score"] = r["end"] - r["start"]
        rec["sum_of_IG"] = total
        rec.update({"mol": None, "mol_smiles": None, "mol_id": None, "prediction_score": tscore, "target_label": tidx,
                    "true_label": true_label})
        results.append(rec)
    return results
