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
import collections
import contextlib

import torch


def integrated_gradients(score_fn, features, adjacency, divide_number=100, modal=("features", "adjs"),
                         perturbation=None, method="ig", noise_scale=0.1, seed=1234):
    """Returns {"features": [B, N, F] tensor, "adjs": [nnz] tensor in the CSR order of channel 0,
    "sum_of_ig": float, "start_score": f(scale 0), "end_score": f(scale 1)} (only the requested modals).
    For method "ig" the completeness check of the reference (:262-275) is sum_of_ig ~ end - start.
    "smooth_grad" / "smooth_ig" (:235-259): D noisy steps, step k at scale 1 (smooth_grad) or (k + 1) / D (smooth_ig) plus N(0, noise_scale) noise drawn
    on the device (ops.ig_perturb / ops.ig_perturb_values, the noise of include/kgcn_hip.h with compound g = the batch row
    and sample k = the step, streams 0 and 1); the mean gradient, for smooth_ig times the clean data.  start_score and end_score
    come from clean inputs."""
    modal = tuple(modal)
    pert = modal if perturbation is None else tuple(perturbation)
    base_vals = [c.values for c in adjacency.channels]
    x0 = features.detach()
    ig = {}
    if "features" in modal:
        ig["features"] = torch.zeros_like(x0)
    if "adjs" in modal:
        ig["adjs"] = torch.zeros_like(base_vals[0])

    def grads_at(scale, sample=None):
        vals = [v.clone() for v in base_vals]
        if sample is None:
            x = (x0 * scale if "features" in pert else x0).clone().requires_grad_("features" in modal)
            if "adjs" in pert:
                vals[0] = vals[0] * scale
        else:                                            # step `sample` of a smooth method: scale and noise in one launch
            from . import ops
            B = x0.shape[0]
            sc = torch.full((B,), float(scale), device=x0.device, dtype=torch.float32)
            smp, rows = [int(sample)] * B, list(range(B))
            x = (ops.ig_perturb(x0, sc, noise_scale, smp, rows, 1, ops.IG_STREAM_FEATURES, seed) if "features" in pert
                 else x0.clone()).requires_grad_("features" in modal)
            if "adjs" in pert:
                vals[0] = ops.ig_perturb_values(adjacency.channels[0], base_vals[0], sc, noise_scale, smp, rows,
                                                ops.IG_STREAM_ADJACENCY, seed)
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
    elif method in SMOOTH_METHODS:
        D = int(divide_number)
        if D < 1:
            raise ValueError("divide_number must be >= 1")
        if not float(noise_scale) >= 0.0:
            raise ValueError("noise_scale must be >= 0, got %r" % (noise_scale,))
        for k in range(D):
            g, _ = grads_at((k + 1) / float(D) if method == "smooth_ig" else 1.0, sample=k)
            for m in ig:
                ig[m] += g[m] * data[m] / float(D) if method == "smooth_ig" else g[m] / float(D)
    else:
        raise ValueError("unsupported method %r (%s)" % (method, ", ".join(IG_METHODS + SMOOTH_METHODS)))
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


def _entry_rows(csr):
    """Row index (graph * rows + row) of every stored entry of a batched CSR, in CSR order."""
    rp = csr.rowptr.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])


def _entry_graphs(csr):
    """Graph index of every stored entry of a batched CSR, in CSR order."""
    return torch.div(_entry_rows(csr), csr.rows, rounding_mode="floor")


def values_to_dense(csr, values):
    """sparse_to_dense_core of the reference (:208): per-entry values of channel 0 -> dense [T, M, K]."""
    dense = torch.zeros((csr.num_graphs * csr.rows, csr.cols), device=values.device, dtype=values.dtype)
    dense.index_put_((_entry_rows(csr), csr.cv[:, 0].long()), values, accumulate=True)
    return dense.reshape(csr.num_graphs, csr.rows, csr.cols)


# -------------------------------------------------------------------------------------------------
# the compound drivers (multimodal_, vecmodal_ and cpi_integrated_gradients) and the host protocol they share:
# kgcn/visualization.py:22-285 (CompoundVisualizer) and :442-574 (cal_feature_IG), batched.  What holds for all three:
#   inputs   features [G, N, F] and adjacency (the channels of data_util.build_adjs), or a data_util.DeviceGraphDataset as
#            `adjacency` (features None); labels, needed by label_target 'label', 'correct' and 'uncorrect'; compounds: dataset
#            indices (default all).  The modals named by `modal` are both scaled and attributed (:58-71, :552-553).
#   methods  'ig', 'grad_prod', 'grad' (ig_scales) and, where the driver takes them, 'smooth_grad' / 'smooth_ig' (:235-259,
#            smooth_rows): D noisy samples beside two clean copies, the targeted inputs being x * scale + N(0, noise_scale)
#            (kgcn/feed.py:88, gcn.py:661 default 0.1; the values of EVERY adjacency channel when 'adjs' is a target, feed.py:116-121).
#            smooth_grad returns the mean gradient, smooth_ig the mean gradient times the clean data; check_score comes from the
#            two clean copies.
#   targets  every compound's target is read from an unscaled forward pass through select_label_target (_ig_jobs).
#   copies   the copies of one compound -- its scaled or perturbed inputs, ig_row_plan -- are batch rows of ONE forward and ONE
#            backward, `chunk` compounds (default IG_ROWS_PER_CHUNK // copies) at a time with the parameters frozen
#            (frozen_parameters); this is valid only because the model mixes no rows, and any other model is refused.  The graph
#            branch of the copies is _graph_copies', their weighted sum _reduce_graph_copies'.  Chunking and `compounds` subsets do
#            not change a bit of a compound's result: the noise of the smooth methods is drawn on the device from (seed, dataset
#            index of the compound, sample number) -- include/kgcn_hip.h.
#   records  one dict per job with the keys the reference dumps (_ig_record): features / features_IG [N, F], adjs / adjs_IG [N, N]
#            (channel 0, dense) for the targeted modals, check_score (end - start), sum_of_IG, prediction_score, target_label,
#            true_label, mol / mol_smiles / mol_id (None: no RDKit) -- plus compound_id and assay, which dump_record drops and
#            ig_filename uses.
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
    raise ValueError("unsupported method %r (%s; the rows of smooth_grad / smooth_ig come from smooth_rows)"
                     % (method, ", ".join(IG_METHODS)))


SMOOTH_METHODS = ("smooth_grad", "smooth_ig")


def smooth_rows(method, divide_number, noise_scale):
    """The copies of one compound for 'smooth_grad' / 'smooth_ig' (:235-259) -> (scales, sigmas, samples, weights, start_row,
    end_row), D + 2 rows: row 0 (scale 0) and row 1 (scale 1) are clean and carry weight 0 -- they give start_score and end_score,
    which the reference takes from clean feeds (:279-286); row 2 + k is sample k with noise N(0, noise_scale), weight 1 / D and
    scale 1 (smooth_grad) or (k + 1) / D (smooth_ig)."""
    if method not in SMOOTH_METHODS:
        raise ValueError("smooth_rows: method must be one of %s, got %r" % (", ".join(SMOOTH_METHODS), method))
    D = int(divide_number)
    if D < 1:
        raise ValueError("divide_number must be >= 1")
    ns = float(noise_scale)
    if not ns >= 0.0:
        raise ValueError("noise_scale must be >= 0, got %r" % (noise_scale,))
    scales = [0.0, 1.0] + [1.0 if method == "smooth_grad" else (k + 1) / float(D) for k in range(D)]
    return scales, [0.0, 0.0] + [ns] * D, [0, 0] + list(range(D)), [0.0, 0.0] + [1.0 / D] * D, 0, 1


IG_RAW_METHODS = ("grad", "smooth_grad")          # the summed gradient itself, not multiplied by the clean data
IGRowPlan = collections.namedtuple("IGRowPlan", "scales weights noise method start_row end_row")


def ig_row_plan(method, divide_number, noise_scale=0.1, seed=1234):
    """The copies of one compound for any method, as the chunk functions take them -> IGRowPlan: scales and weights per copy,
    noise = None (ig_scales: 'ig', 'grad_prod', 'grad') or (sigmas, samples, seed) per copy (smooth_rows), the method, and the
    copies whose scores are start_score and end_score."""
    if method in SMOOTH_METHODS:
        scales, sigmas, samples, weights, start_row, end_row = smooth_rows(method, divide_number, noise_scale)
        return IGRowPlan(scales, weights, (sigmas, samples, int(seed)), method, start_row, end_row)
    if method in IG_METHODS:
        scales, weights = ig_scales(method, divide_number)
        return IGRowPlan(scales, weights, None, method, 0, len(scales) - 1)
    raise ValueError("unsupported method %r (%s)" % (method, ", ".join(IG_METHODS + SMOOTH_METHODS)))


def ig_plan_row(plan, row):
    """The one-copy plan of copy `row`: what a per-step loop hands the chunk functions, one batch-1 pass per copy."""
    noise = None if plan.noise is None else ([plan.noise[0][row]], [plan.noise[1][row]], plan.noise[2])
    return plan._replace(scales=[plan.scales[row]], weights=[plan.weights[row]], noise=noise, start_row=0, end_row=0)


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


def _host_array(a):
    """A host array of labels or sizes given as a tensor or anything numpy takes; None stays None."""
    import numpy as np
    return None if a is None else np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)


def _parameter_device(model):
    return next(model.parameters(), torch.zeros(0, device="cuda")).device


def _compound_dataset(features, adjacency, device):
    """The compounds as a data_util.DeviceGraphDataset: `adjacency` itself when it is one (features None), else one built from
    features [G, N, F] and the channels of data_util.build_adjs on device(), which is called only then."""
    from .data_util import DeviceGraphDataset
    if isinstance(adjacency, DeviceGraphDataset):
        dataset = adjacency
    else:
        dev = device()
        dataset = DeviceGraphDataset(adjacency, features.detach().cpu().numpy() if torch.is_tensor(features) else features, device=dev)
    if dataset.features is None:
        raise ValueError("the dataset carries no node features")
    return dataset


def _compounds_per_chunk(chunk, default):
    """`chunk` as given, or the driver's default; at least one compound."""
    chunk = max(1, default) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    return chunk


def _ig_jobs(predict, ids, step, label_target, entries):
    """The unscaled pass (:479-485) and the choice of targets (:502-529).  predict(part) -> the predictions of the compounds `part`
    as a host array [len(part), K]; it runs without autograd, `step` compounds at a time (and builds a freshly made model).
    entries(cid, row) -> (key, prediction, true_label) of every attribution of compound cid, whose row of predictions is `row`.
    Yields (key, prediction, true_label, target_index, target_score, class mask) for those select_label_target does not skip."""
    import numpy as np
    with torch.no_grad():
        preds = [predict(ids[i:i + step]) for i in range(0, len(ids), step)]
    preds = np.concatenate(preds) if preds else np.zeros((0, 0), np.float32)
    for cid, row in zip(ids, preds):
        for key, pred, true_label in entries(cid, row):
            sel = select_label_target(pred, label_target, true_label)
            if sel is not None:
                yield (key, pred, true_label) + sel


def _one_job_per_compound(lab):
    """entries of _ig_jobs for one attribution per compound: the whole row of predictions, true_label = argmax of the label row."""
    import numpy as np
    return lambda cid, row: [(cid, row, None if lab is None else int(np.argmax(lab[cid])))]


@contextlib.contextmanager
def frozen_parameters(model):
    """Inside the block no parameter of `model` requires a gradient (the attribution differentiates with respect to inputs alone);
    on exit, after an exception too, every parameter has its own requires_grad back."""
    frozen = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in frozen:
            p.requires_grad_(False)
        yield
    finally:
        for p, r in frozen:
            p.requires_grad_(r)


GraphCopies = collections.namedtuple("GraphCopies", "adj x x_in adj_in v0 sc wt noise")


def _graph_copies(dataset, ids, plan, targets, need_grad=True):
    """The graph branch of len(ids) compounds x len(plan.scales) copies -> GraphCopies: the repeated clean batch (adj, x); what
    the model is fed, x_in and adj_in -- a targeted input is x * scale on the clean path and x * scale + sigma * z on the noisy
    one (ops.ig_perturb, ops.ig_perturb_values), an input that is no target is fed as it is; v0, the values of channel 0 the
    gradient is taken at (None unless 'adjs' is a target); the scale and the weight of every row, sc and wt [B] (formed before
    the model runs: a host-to-device copy later would wait for it); and the noise operands (sigmas [B], samples [B], dataset
    indices [C], seed) or None.  x_in and v0 are leaves that require a gradient iff need_grad."""
    C, rep = len(ids), len(plan.scales)
    dev = dataset.features.device
    adj, x = dataset.batch([i for i in ids for _ in range(rep)])
    sc = torch.tensor(plan.scales, dtype=torch.float32, device=dev).repeat(C)
    wt = torch.tensor(plan.weights, dtype=torch.float32, device=dev).repeat(C)
    noise = None
    if plan.noise is not None:
        from . import ops
        sg = torch.tensor(plan.noise[0], dtype=torch.float32, device=dev).repeat(C)
        smp = torch.tensor(plan.noise[1], dtype=torch.int32, device=dev).repeat(C)
        cid = torch.tensor(ids, dtype=torch.int32, device=dev)
        seed = plan.noise[2]
        noise = (sg, smp, cid, seed)
    x_in = x
    if "features" in targets:
        if noise is None:
            x_in = x * sc.view(-1, 1, 1)
        else:
            x_in = ops.ig_perturb(x.view(C, rep, x.shape[1], x.shape[2])[:, 0], sc, sg, smp, cid, rep, ops.IG_STREAM_FEATURES, seed)
        x_in.requires_grad_(need_grad)
    adj_in, v0 = adj, None
    if "adjs" in targets:                       # kgcn/feed.py:116-121: the values of every channel are scaled
        if noise is None:
            vals = [c.values * sc[_entry_graphs(c)] for c in adj.channels]
        else:
            rows = cid.repeat_interleave(rep)
            vals = [ops.ig_perturb_values(c, c.values, sc, sg, smp, rows, ops.IG_STREAM_ADJACENCY + ch, seed)
                    for ch, c in enumerate(adj.channels)]
        v0 = vals[0].requires_grad_(need_grad)
        adj_in = adj.with_values(vals)
    return GraphCopies(adj, x, x_in, adj_in, v0, sc, wt, noise)


def _copies_data(g, targets):
    """What _reduce_graph_copies needs of the copies g beside their gradients and scores: the clean features 'x', the weights
    'weight' and, where 'adjs' is a target, channel 0 dense as 'adjs_data' [B, N, N]."""
    gr = {"x": g.x, "weight": g.wt}
    if "adjs" in targets:
        gr["adjs_data"] = values_to_dense(g.adj.channels[0], g.adj.channels[0].values)
    return gr


def _copies_grads(data, g, targets, grads):
    """_copies_data plus the per-copy gradients of the targeted graph inputs, taken off the front of `grads` (what autograd returned
    for [x_in, v0]; None = a forward-only pass, the gradients zero): 'features' [B, N, F], 'adjs' channel 0 dense [B, N, N]."""
    gr = dict(data)
    if "features" in targets:
        gr["features"] = torch.zeros_like(g.x) if grads is None else grads.pop(0)
    if "adjs" in targets:
        gr["adjs"] = torch.zeros_like(data["adjs_data"]) if grads is None else values_to_dense(g.adj.channels[0], grads.pop(0))
    return gr


def _reduce_graph_copies(gr, C, plan, targets):
    """The per-copy quantities of _copies_grads beside 'score' [B] (C compounds x B / C copies, or as many one-copy results
    concatenated) -> per compound: 'features' and 'adjs', the sums over the copies weighted by 'weight', in one fixed order for
    the batched and the per-step form alike, times the clean data unless plan.method is one of IG_RAW_METHODS; 'adjs_data';
    'start' and 'end', the scores of the copies plan.start_row and plan.end_row."""
    rep = gr["score"].shape[0] // C
    wv = gr["weight"].view(C, rep, 1, 1)
    raw = plan.method in IG_RAW_METHODS
    out = {}
    if "features" in targets:
        N, F = gr["x"].shape[1], gr["x"].shape[2]
        ig = (gr["features"].view(C, rep, N, F) * wv).sum(1)
        out["features"] = ig if raw else ig * gr["x"].view(C, rep, N, F)[:, 0]
    if "adjs" in targets:
        M, K = gr["adjs"].shape[1], gr["adjs"].shape[2]
        ig = (gr["adjs"].view(C, rep, M, K) * wv).sum(1)
        data = gr["adjs_data"].view(C, rep, M, K)[:, 0]
        out["adjs"] = ig if raw else ig * data
        out["adjs_data"] = data
    s = gr["score"].view(C, rep)
    out["start"], out["end"] = s[:, plan.start_row], s[:, plan.end_row]
    return out


def _rows_to_host(res, keys, out):
    """res[key] = row k of every tensor of `out` as a host array, for the k-th of `keys`; returns the host arrays."""
    host = {m: t.detach().cpu().numpy() for m, t in out.items()}
    for k, key in enumerate(keys):
        res[key] = {m: a[k] for m, a in host.items()}
    return host


def _ig_record(rec, job, targets, data, ig, start, end, sum_of_ig=None):
    """Completes the record of one job of _ig_jobs with the keys every compound driver dumps: for each target m the clean data
    data[m]() as m and the attribution ig[m] as m + '_IG', and DUMP_KEYS_FIXED -- check_score = end - start; sum_of_IG, the fp64
    sum of the record's own *_IG arrays, modal after modal (sum_of_ig where the driver has formed exactly that already); mol,
    mol_smiles and mol_id None (no RDKit); the job's prediction_score, target_label and true_label."""
    import numpy as np
    _, _, true_label, tidx, tscore, _ = job
    total = 0.0
    for m in targets:
        rec[m] = data[m]()
        rec[m + "_IG"] = ig[m]
        if sum_of_ig is None:
            total += float(ig[m].astype(np.float64).sum())
    rec["check_score"] = float(end) - float(start)
    rec["sum_of_IG"] = total if sum_of_ig is None else float(sum_of_ig)
    rec.update({"mol": None, "mol_smiles": None, "mol_id": None, "prediction_score": tscore, "target_label": tidx,
                "true_label": true_label})
    return rec


# -------------------------------------------------------------------------------------------------
# the multimodal model (example_model/model_multimodal.py built with feed_embedded_layer=True, gcn.py:637-656): the embedded
# sequence is the third modal, attributed by the HIP input-gradient kernel of the conv-pool
# -------------------------------------------------------------------------------------------------
def _copy_grads(model, dataset, tokens, ids, plan, targets, masks, need_grad=True):
    """One forward + backward over len(ids) compounds x len(plan.scales) copies -> the per-copy quantities _reduce_copies sums:
    those of _copies_grads, 'pooled' d pooled with its arg-max bytes 'arg' for the embedded sequence (perturbed, on the noisy
    path, by ops.seq_conv_pool_perturbed), the token rows and the score [B].  masks [C, K] selects the target class(es) of each
    compound.  need_grad=False: the forward alone (a copy of weight 0, run for its score), the gradients zero and the arg-max
    bytes 0xFF."""
    ids = [int(i) for i in ids]
    rep = len(plan.scales)
    g = _graph_copies(dataset, ids, plan, targets, need_grad)
    emb = "embedded_layer" in targets
    tok = tokens[torch.as_tensor(ids, device=tokens.device)]
    with torch.set_grad_enabled(need_grad):
        logits, pooled, arg = model.run(g.x_in, g.adj_in, tok, g.sc if emb else torch.ones_like(g.sc), rep, input_grad=need_grad and emb,
                                        sequence_noise=g.noise if emb else None)
        score = (torch.softmax(logits, dim=1) * torch.as_tensor(masks, device=g.x.device).repeat_interleave(rep, 0)).sum(1)
    grads = None
    if need_grad:
        wrt = ([g.x_in] if "features" in targets else []) + ([g.v0] if g.v0 is not None else []) + ([pooled] if emb else [])
        grads = list(torch.autograd.grad(score.sum(), wrt))
    gr = _copies_grads(_copies_data(g, targets), g, targets, grads)
    gr["tok"], gr["score"] = tok, score.detach()
    if emb:
        gr["pooled"] = grads.pop(0) if need_grad else torch.zeros_like(pooled)
        gr["arg"] = arg if need_grad else torch.full(pooled.shape, 0xFF, dtype=torch.uint8, device=g.x.device)
    return gr


def _reduce_copies(gr, C, plan, targets, table, conv_w, pool):
    """_reduce_graph_copies plus 'embedded_layer', which ops.seq_conv_pool_input_grad sums over the copies in order."""
    out = _reduce_graph_copies(gr, C, plan, targets)
    if "embedded_layer" in targets:
        from . import ops
        out["embedded_layer"] = ops.seq_conv_pool_input_grad(gr["pooled"], gr["arg"], gr["tok"], table, conv_w, pool,
                                                             gr["score"].shape[0] // C, row_weight=gr["weight"],
                                                             times_table=plan.method not in IG_RAW_METHODS)
    return out


def multimodal_integrated_gradients(model, features, adjacency, tokens, labels=None, divide_number=100, modal="all", method="ig",
                                    label_target="max", chunk=None, compounds=None, sequence_symbol=None, batched=True,
                                    noise_scale=0.1, seed=1234):
    """Integrated gradients of models.MultimodalGCN (kgcn visualize on example_model/model_multimodal.py), by the protocol of the
    section above -> its records, with embedded_layer [L, E] / embedded_layer_IG as the third modal and amino_acid_seq (when
    sequence_symbol is given).

    tokens int32 [G, L] device tensor (data_util.sequence_table); labels [G, K], true_label = argmax.  The score is the softmax
    probability of the target class.  All five methods.  The embedded-sequence attribution comes from the HIP input-gradient
    kernel (ops.seq_conv_pool_input_grad), which sums the copies in order; on the noisy path the embedded sequence is perturbed
    inside the conv-pool's window staging (ops.seq_conv_pool_perturbed).  batched=False runs the reference's loop instead: one
    batch-1 pass per compound and step through the same ops (forward only for a copy of weight 0), the per-step gradients summed
    by the reduction the batched form uses; it sees the same noise."""
    import numpy as np
    import string
    from . import models
    if not isinstance(model, models.MultimodalGCN) or not getattr(model, "ROW_INDEPENDENT", False):
        raise TypeError("multimodal_integrated_gradients batches the scaled copies as rows: it needs a model whose rows never "
                        "mix (models.MultimodalGCN), got %s" % type(model).__name__)
    targets = ig_modal_targets(modal)
    plan = ig_row_plan(method, divide_number, noise_scale, seed)
    dataset = _compound_dataset(features, adjacency, lambda: tokens.device)
    G = dataset.num_graphs
    if tokens.shape[0] != G:
        raise ValueError("%d token rows for %d graphs" % (tokens.shape[0], G))
    ids = list(range(G)) if compounds is None else [int(i) for i in compounds]
    chunk = _compounds_per_chunk(chunk, IG_ROWS_PER_CHUNK // len(plan.scales))
    seqm = model.sequence
    table, conv_w, pool = seqm.embeddings.detach(), seqm.conv_kernel.detach(), seqm.pool

    def predict(part):
        adj, x = dataset.batch(part)
        return torch.softmax(model(x, adj, sequences=tokens[torch.as_tensor(part, device=tokens.device)]), 1).cpu().numpy()

    jobs = list(_ig_jobs(predict, ids, chunk, label_target, _one_job_per_compound(_host_array(labels))))
    res = {}
    with frozen_parameters(model):
        if batched:
            for i in range(0, len(jobs), chunk):
                part = jobs[i:i + chunk]
                gr = _copy_grads(model, dataset, tokens, [j[0] for j in part], plan, targets, np.stack([j[5] for j in part]))
                _rows_to_host(res, [j[0] for j in part], _reduce_copies(gr, len(part), plan, targets, table, conv_w, pool))
        else:
            for j in jobs:                                   # one batch-1 pass per copy; a copy of weight 0 runs forward only
                rows = [_copy_grads(model, dataset, tokens, [j[0]], ig_plan_row(plan, r), targets, j[5][None], need_grad=w != 0.0)
                        for r, w in enumerate(plan.weights)]
                gr = {k: rows[0][k] if k == "tok" else torch.cat([p[k] for p in rows]) for k in rows[0]}
                _rows_to_host(res, [j[0]], _reduce_copies(gr, 1, plan, targets, table, conv_w, pool))
    results = []
    for job in jobs:
        cid, r = job[0], res[job[0]]
        rec = {"compound_id": cid, "assay": assay_string(job[1], job[3])}
        if sequence_symbol is not None:
            rec["amino_acid_seq"] = "".join(string.ascii_uppercase[int(t)] for t in np.asarray(sequence_symbol[cid]).reshape(-1))
        data = {"features": lambda: dataset.features[cid].cpu().numpy(), "adjs": lambda: r["adjs_data"],
                "embedded_layer": lambda: table[tokens[cid].long()].cpu().numpy()}
        results.append(_ig_record(rec, job, targets, data, r, r["start"], r["end"]))
    return results


# -------------------------------------------------------------------------------------------------
# the vector-modality models (example_model/model_multimodal_vec.py, vector `profeat`; model_multimodal_regression.py, vector
# `dragon`): kgcn/visualization.py:106-111, :128-132 and kgcn/feed.py:201-206 treat the per-graph vector like any other modality.
# The vector branch is fused over the copies (csrc/vecig.hip)
# -------------------------------------------------------------------------------------------------
VECMODAL_VECTOR_NAMES = {"MultimodalVecGCN": "profeat", "MultimodalRegressionGCN": "dragon"}
# The default of `fused` per model follows the measurement (tools/vecmodal_ig_bench.py, profiles/vecmodal_ig_bench.json: 256 compounds,
# N = 50, F = 81, D = 100 on the MI355X).  The fused route was NOT ahead at either model: the whole call took 16.0 ms fused against
# 15.5 ms composed for MultimodalVecGCN (Dv = 1437 -> 300; 29.2 against 28.7 ms with every modal) and 12.7 against 12.7 ms for
# MultimodalRegressionGCN (Dv = 37 -> 8), differences inside the run-to-run spread of 3-4 %.  The D + 1 copies of the GRAPH branch
# (1.3 million node rows), which both routes run through the same layers, and the host side of the call carry the time; the first
# vector layer's GEMM over all copies, which the fused route removes, is a small part of it.  So both models default to the
# composed route, as ops.short_dense_fusion is off: the fused route stays available (fused=True), tested to the same bounds.
VECMODAL_IG_FUSED = {"MultimodalVecGCN": False, "MultimodalRegressionGCN": False}


def vecmodal_ig_targets(model, modal, vector_name=None):
    """-> (targets, vector name): the modals `modal` names for a vector-modality model.  'features', 'adjs' and the vector's own
    name ('profeat' / 'dragon', or vector_name) are the modals; 'all' is every modal the model differentiates.
    MultimodalRegressionGCN never reads the adjacency -- the reference drops a target whose tf.gradients is None (:80-87) -- so
    'adjs' is not in its 'all', and asking for it raises."""
    from . import models
    if not isinstance(model, (models.MultimodalVecGCN, models.MultimodalRegressionGCN)) or not getattr(model, "ROW_INDEPENDENT", False):
        raise TypeError("vecmodal_integrated_gradients batches the scaled copies as rows and feeds the vector branch's first layer: "
                        "it needs a models.MultimodalVecGCN or models.MultimodalRegressionGCN, got %s" % type(model).__name__)
    name = VECMODAL_VECTOR_NAMES[type(model).__name__] if vector_name is None else str(vector_name)
    if name in ("features", "adjs", "all"):
        raise ValueError("vector_name %r is the name of another modal" % (name,))
    regression = isinstance(model, models.MultimodalRegressionGCN)
    modals = ("features", name) if regression else ("features", "adjs", name)
    if modal == "all":
        return modals, name
    if modal == "adjs" and regression:
        raise ValueError("models.MultimodalRegressionGCN never reads the adjacency: its prediction has no gradient with respect to "
                         "'adjs' (modal must be 'all' or one of %s)" % ", ".join(modals))
    if modal not in modals:
        raise ValueError("modal must be 'all' or one of %s, got %r" % (", ".join(modals), modal))
    return (modal,), name


def _vecmodal_first_layer(model):
    """The vector branch's first Dense + BatchNormalization + relu and what the fused route needs of it, formed once per call."""
    from . import models
    layer = model.vec if isinstance(model, models.MultimodalRegressionGCN) else model.tower[0]
    W = layer.kernel.detach().contiguous()
    par = {"layer": layer, "W": W, "Wt": W.t().contiguous(), "bias": layer.bias.detach(), "act": layer.activation, "bn": {}, "scale": None}
    if layer.batch_norm:
        par["bn"] = {"gamma": layer.gamma.detach(), "beta": layer.beta.detach(), "moving_mean": layer.moving_mean,
                     "moving_variance": layer.moving_variance, "eps": layer.eps}
        par["scale"] = layer.gamma.detach() / torch.sqrt(layer.moving_variance + layer.eps)
    return par


def _vecmodal_chunk(model, dataset, vtab, sizes, ids, plan, targets, vname, masks, first, fused, need_grad=True):
    """One forward + backward over len(ids) compounds x len(plan.scales) copies -> per compound what _reduce_graph_copies returns
    and the vector's weighted sum over the copies [C, 1, Dv] (unmultiplied by the data for IG_RAW_METHODS).  The graph branch is
    _graph_copies': the copies are batch rows of the model's own layers.  The vector branch, fused: P = v W once per compound
    (ops.dense), the first layer of every clean copy from ops.ig_copies_expand (of every noisy copy from the layer itself,
    without a graph), handed to the model as vector_first; the gradient arriving there goes through ops.ig_copies_reduce and ONE
    [C, H] x W^T product.  Not fused: the scaled or perturbed vectors go in as vectors= and the per-copy gradients are summed.
    need_grad=False: the forward alone, the sums zero."""
    from . import models, ops
    ids = [int(i) for i in ids]
    C, rep = len(ids), len(plan.scales)
    regression = isinstance(model, models.MultimodalRegressionGCN)
    g = _graph_copies(dataset, ids, plan, targets, need_grad)
    sc, dev = g.sc, g.x.device
    idt = torch.as_tensor(ids, device=dev)
    v = vtab[idt]
    Dv = v.shape[1]
    leaf = None
    if vname not in targets:                    # kgcn/feed.py:205: not a target, fed as it is
        kw = {"vectors": v.repeat_interleave(rep, 0)}
    else:
        with torch.no_grad():
            if g.noise is not None:
                sg, smp, cid, seed = g.noise
                fed = ops.ig_perturb(v.view(C, 1, Dv), sc, sg, smp, cid, rep, ops.IG_STREAM_VECTOR, seed).view(C * rep, Dv)
                leaf = first["layer"](fed) if fused else fed
            elif fused:
                P = _cpi_dense(v, first["W"], 1)
                leaf = ops.ig_copies_expand(P, plan.scales, first["bias"], activation=first["act"], **first["bn"])
            else:
                leaf = v.repeat_interleave(rep, 0) * sc.view(-1, 1)
        leaf = leaf.detach().requires_grad_(need_grad)
        kw = {"vector_first" if fused else "vectors": leaf}
    if regression and sizes is not None:
        kw["enabled_node_nums"] = sizes[idt].repeat_interleave(rep)
    with torch.set_grad_enabled(need_grad):
        out = model(g.x_in, g.adj_in, **kw)
        pred = out if regression else torch.softmax(out, dim=1)
        score = (pred * torch.as_tensor(masks, device=dev).repeat_interleave(rep, 0)).sum(1)
    grads = None
    if need_grad:
        wrt = ([g.x_in] if "features" in targets else []) + ([g.v0] if g.v0 is not None else []) + ([leaf] if leaf is not None else [])
        grads = list(torch.autograd.grad(score.sum(), wrt))
    with torch.no_grad():
        gr = _copies_grads(_copies_data(g, targets), g, targets, grads)
        gr["score"] = score.detach()
        res = _reduce_graph_copies(gr, C, plan, targets)
        if vname in targets:
            if not need_grad:
                dv = torch.zeros_like(v)
            elif fused:
                S = ops.ig_copies_reduce(grads.pop(0), leaf, g.wt[:rep], first["scale"], first["act"])
                dv = _cpi_dense(S, first["Wt"], 1)
            else:
                dv = (grads.pop(0).view(C, rep, Dv) * g.wt.view(C, rep, 1)).sum(1)
            res[vname] = (dv if plan.method in IG_RAW_METHODS else dv * v).view(C, 1, Dv)
    return res


def vecmodal_integrated_gradients(model, features, adjacency, vectors, labels=None, divide_number=100, modal="all", method="ig",
                                  label_target="max", vector_name=None, chunk=None, compounds=None, fused=None, noise_scale=0.1,
                                  seed=1234, enabled_node_nums=None):
    """`kgcn visualize` of the vector-modality models (kgcn/visualization.py:22-285 and :442-574 with info.vector_modal_name set,
    :106-111 and :128-132) for a models.MultimodalVecGCN (vector `profeat`) or models.MultimodalRegressionGCN (vector `dragon`)
    by the protocol of the section above -> its records, with <vector name> [Dv] / <vector name>_IG [1, Dv] (the reference
    accumulates into zeros((1, Dv))) as the third modal.

    vectors [G, Dv] (data_util.vector_table, or a host array); labels [G, K], true_label = argmax; enabled_node_nums [G]: the
    node counts MultimodalRegressionGCN's GraphBatchNormalization masks with (None: every row counts; the other model ignores
    them).  modal: 'all', 'features', 'adjs' or the vector's name (vecmodal_ig_targets; vector_name defaults to the model's); a
    vector that is not a target is fed unscaled (kgcn/feed.py:205).  All five methods: the vector is perturbed as a [1, Dv] row
    set on the stream ops.IG_STREAM_VECTOR.
    Score: the softmax probability of the target class (MultimodalVecGCN); the prediction column itself
    (MultimodalRegressionGCN: predictions = logits, one task of label_dim entries, cal_feature_IG :488-499).

    fused=True: the vector branch's first layer --
    Dense(Dv -> 300), respectively Dense(Dv -> 8), by far the largest of the tower -- is not run per copy: a clean copy's
    pre-activation is alpha_k (v W) + b, so v W is formed once per compound and ops.ig_copies_expand sweeps the copies; the
    gradient with respect to the fed vector is dpre_k W^T, linear in dpre_k for the smooth methods too, so
    ops.ig_copies_reduce sums the copies and ONE [C, H] x W^T product follows.  No per-copy [C K, Dv] gradient is formed.
    fused=False: the scaled or perturbed vectors go through the model as vectors=, with autograd to them.  fused=None (the
    default): the route the measurement favours for the model, VECMODAL_IG_FUSED -- at present the composed one for both, see
    there."""
    import numpy as np
    from . import models
    targets, vname = vecmodal_ig_targets(model, modal, vector_name)
    regression = isinstance(model, models.MultimodalRegressionGCN)
    plan = ig_row_plan(method, divide_number, noise_scale, seed)
    chunk = _compounds_per_chunk(chunk, IG_ROWS_PER_CHUNK // len(plan.scales))
    if vectors is None:
        raise ValueError("the vector modality %r is missing (vectors [G, Dv])" % (vname,))
    fused = VECMODAL_IG_FUSED[type(model).__name__] if fused is None else bool(fused)
    dataset = _compound_dataset(features, adjacency, lambda: _parameter_device(model))
    dev = dataset.features.device
    G = dataset.num_graphs
    vtab = (vectors.detach() if torch.is_tensor(vectors) else torch.as_tensor(np.asarray(vectors, np.float32))).to(dev, torch.float32)
    if vtab.dim() != 2 or vtab.shape[0] != G:
        raise ValueError("vectors %s for %d graphs: expected [G, Dv]" % (tuple(vtab.shape), G))
    vtab = vtab.contiguous()
    sizes = None
    if enabled_node_nums is not None:
        sizes = torch.as_tensor(_host_array(enabled_node_nums).astype(np.int32).reshape(-1), device=dev)
        if sizes.numel() != G:
            raise ValueError("%d enabled_node_nums for %d graphs" % (sizes.numel(), G))
    ids = list(range(G)) if compounds is None else [int(i) for i in compounds]

    def predict(part):
        adj, x = dataset.batch(part)
        idt = torch.as_tensor(part, device=dev)
        kw = {"vectors": vtab[idt]}
        if regression and sizes is not None:
            kw["enabled_node_nums"] = sizes[idt]
        out = model(x, adj, **kw)
        return (out if regression else torch.softmax(out, 1)).cpu().numpy()

    jobs = list(_ig_jobs(predict, ids, chunk, label_target, _one_job_per_compound(_host_array(labels))))
    res = {}
    with frozen_parameters(model):
        first = _vecmodal_first_layer(model) if jobs else None
        for i in range(0, len(jobs), chunk):
            part = jobs[i:i + chunk]
            _rows_to_host(res, [j[0] for j in part], _vecmodal_chunk(model, dataset, vtab, sizes, [j[0] for j in part], plan, targets,
                                                                     vname, np.stack([j[5] for j in part]), first, fused))
    results = []
    for job in jobs:
        cid, r = job[0], res[job[0]]
        data = {"features": lambda: dataset.features[cid].cpu().numpy(), "adjs": lambda: r["adjs_data"],
                vname: lambda: vtab[cid].cpu().numpy()}
        results.append(_ig_record({"compound_id": cid, "assay": assay_string(job[1], job[3])}, job, targets, data, r, r["start"], r["end"]))
    return results


# -------------------------------------------------------------------------------------------------
# the protein-sequence CNN (sample_protein/sequence/cnn.py; 03run.sh: kgcn visualize --config config_cnn.pos.json
# --ig_label_target 1): the embedded sequence is the one modal, the sample's graph a dummy the model never reads.  The first
# conv-pool layer is fused over the copies (csrc/convig.hip)
# -------------------------------------------------------------------------------------------------
SEQCNN_IG_ROWS_PER_CHUNK = 2048   # rows (proteins x copies) per forward + backward: the first layer's output is L / 4 x 505 floats a row
# The default of `fused` follows the measurement (tools/seqcnn_ig_bench.py, profiles/seqcnn_ig_bench.json: L = 1000, E = 25, D = 100
# on the MI355X, both routes in the same run, median of 10 calls with smallest - largest).  The fused route IS ahead, by far more than
# the run-to-run spread: 18.0 ms (17.9 - 18.5) against 32.8 ms (32.7 - 33.5) composed at 16 proteins, 70.0 ms (69.8 - 70.2) against
# 129.0 ms (128.8 - 129.3) at 64, and 2.8 against 3.4 ms at one protein -- 1.83x, 1.84x and 1.25x; the per-step loop takes 99 ms a
# protein.  Here, unlike in the vector-modality models, the layer the fused route takes out of the per-copy work is about 39 % of
# the per-copy arithmetic and no graph branch runs beside it.  So the default is the fused route; fused=False stays available under
# the same tests.
SEQCNN_IG_FUSED = True


def _seqcnn_scores(model, masks, rep, dev, **fed):
    """The softmax probability of every row's target class(es): masks [C, K] selects them per protein, rep rows each."""
    logits = model(None, None, **fed)
    return (torch.softmax(logits, dim=1) * torch.as_tensor(masks, device=dev).repeat_interleave(rep, 0)).sum(1)


def _seqcnn_copy_grads(model, e, ids, plan, masks, need_grad=True):
    """The composed route: one forward + backward over len(ids) proteins x len(plan.scales) copies of their clean embedded rows
    e [C, L, E] -> the per-copy quantities _seqcnn_reduce sums: 'grad' [B, L, E] with respect to the fed rows -- e * scale, or on
    the noisy path ops.ig_perturb's e * scale + sigma z on the stream the multimodal conv-pool draws from
    (ops.IG_STREAM_SEQUENCE, row l, column e, the protein's dataset index, the sample number) -- 'score' [B] and 'weight' [B].
    need_grad=False: the forward alone (a copy of weight 0, run for its score), the gradient zero."""
    from . import ops
    C, rep, dev = e.shape[0], len(plan.scales), e.device
    sc = torch.tensor(plan.scales, dtype=torch.float32, device=dev).repeat(C)
    wt = torch.tensor(plan.weights, dtype=torch.float32, device=dev).repeat(C)
    if plan.noise is None:
        fed = e.repeat_interleave(rep, 0) * sc.view(-1, 1, 1)
    else:
        sg = torch.tensor(plan.noise[0], dtype=torch.float32, device=dev).repeat(C)
        smp = torch.tensor(plan.noise[1], dtype=torch.int32, device=dev).repeat(C)
        cid = torch.tensor([int(i) for i in ids], dtype=torch.int32, device=dev)
        fed = ops.ig_perturb(e, sc, sg, smp, cid, rep, ops.IG_STREAM_SEQUENCE, plan.noise[2])
    fed = fed.detach().requires_grad_(need_grad)
    with torch.set_grad_enabled(need_grad):
        score = _seqcnn_scores(model, masks, rep, dev, embedded=fed)
    grad = torch.autograd.grad(score.sum(), [fed])[0] if need_grad else torch.zeros_like(fed)
    return {"grad": grad, "score": score.detach(), "weight": wt}


def _seqcnn_reduce(gr, e, plan):
    """The per-copy quantities of _seqcnn_copy_grads (C proteins x B / C copies, or as many one-copy results concatenated) -> per
    protein 'embedded_layer', the sum over the copies weighted by 'weight' in one fixed order for the batched and the per-step
    form alike, times the clean rows e unless plan.method is one of IG_RAW_METHODS; 'start' and 'end'."""
    C, L, E = e.shape
    rep = gr["score"].shape[0] // C
    ig = (gr["grad"].view(C, rep, L, E) * gr["weight"].view(C, rep, 1, 1)).sum(1)
    s = gr["score"].view(C, rep)
    return {"embedded_layer": ig if plan.method in IG_RAW_METHODS else ig * e, "start": s[:, plan.start_row], "end": s[:, plan.end_row]}


def _seqcnn_fused_chunk(model, tok, e, plan, masks):
    """The fused route over the proteins tok [C, L] (clean rows e) x len(plan.scales) clean copies: Pm = the window maxima of the
    bias-free first convolution and their arg-max ONCE per protein (ops.conv1d_pool_window_max), the first layer of every copy
    from ops.conv1d_ig_expand, handed to the model as first=; the gradient arriving there is summed over the copies by
    ops.conv1d_ig_reduce and ONE input-gradient pass (ops.conv1d_pool_window_grad) follows.  Neither the [C K, L, E] scaled rows
    nor a per-copy gradient of them is formed.  -> what _seqcnn_reduce returns."""
    from . import ops
    C, rep, dev = tok.shape[0], len(plan.scales), tok.device
    conv = model.convs[0]
    table, w = model.embeddings.detach(), conv.conv_kernel.detach()
    Pm, arg = ops.conv1d_pool_window_max(tok, table, w, conv.pool)
    first = ops.conv1d_ig_expand(Pm, plan.scales, conv.conv_bias).requires_grad_(True)
    score = _seqcnn_scores(model, masks, rep, dev, first=first)
    dout = torch.autograd.grad(score.sum(), [first])[0]
    r = ops.conv1d_ig_reduce(dout, first, plan.weights)
    G = ops.conv1d_pool_window_grad(r, arg, Pm, tok, table, w, conv.pool)
    s = score.detach().view(C, rep)
    return {"embedded_layer": G if plan.method in IG_RAW_METHODS else G * e, "start": s[:, plan.start_row], "end": s[:, plan.end_row]}


def seqcnn_integrated_gradients(model, tokens, labels=None, divide_number=100, method="ig", label_target="max", chunk=None,
                                proteins=None, sequence_symbol=None, fused=None, batched=True, noise_scale=0.1, seed=1234):
    """`kgcn visualize` of sample_protein/sequence (03run.sh step 2) for a models.SeqCNN by the protocol of the compound drivers
    above -> their records with embedded_layer [L, E] / embedded_layer_IG [L, E] as the one modal (the dummy graph is not
    attributed) and amino_acid_seq when sequence_symbol is given.

    tokens int32 [G, L] device tensor (data_util.sequence_table); labels [G, K], true_label = argmax; proteins: dataset indices
    (default all).  The score is the softmax probability of the target class; label_target as select_label_target takes it (the
    sample uses 1).  All five methods.
    fused=True ('ig', 'grad_prod', 'grad'): the first layer, Conv1D(505, 4, relu) -> MaxPooling1D(4), is not run per copy.  It is
    linear in the scale before its bias and the window maximum commutes with a non-negative scale, so the bias-free convolution
    and its window maxima are formed ONCE per protein and ops.conv1d_ig_expand sweeps the copies; the convolution's input
    gradient is linear in the pre-activation's, so ops.conv1d_ig_reduce sums the copies and ONE input-gradient pass follows
    (_seqcnn_fused_chunk; include/kgcn_hip.h states the arithmetic and the one deviation, ties created by rounding).
    fused=False: the scaled rows go through the model as embedded=, with autograd to them.  fused=None (the default): the route
    the measurement favours, SEQCNN_IG_FUSED.  The smooth methods always take the composed route -- every sample has its own
    noise, drawn by ops.ig_perturb on the embedded rows -- and fused=True with one of them is refused.
    batched=False runs the reference's loop instead: one batch-1 pass per protein and copy through the composed route's ops
    (forward only for a copy of weight 0), the per-copy gradients summed by the reduction the batched form uses; it sees the same
    noise."""
    import numpy as np
    import string
    from . import models
    if not isinstance(model, models.SeqCNN) or not getattr(model, "ROW_INDEPENDENT", False):
        raise TypeError("seqcnn_integrated_gradients batches the scaled copies as rows and feeds the first conv-pool layer: it needs "
                        "a models.SeqCNN, got %s" % type(model).__name__)
    plan = ig_row_plan(method, divide_number, noise_scale, seed)
    if method in SMOOTH_METHODS:
        if fused:
            raise ValueError("method %r draws its own noise for every copy: it has no fused route (fused=True)" % (method,))
        fused = False
    else:
        fused = SEQCNN_IG_FUSED if fused is None else bool(fused)
    if not (torch.is_tensor(tokens) and tokens.dim() == 2 and tokens.dtype == torch.int32):
        raise ValueError("tokens must be an int32 [G, L] tensor")
    rep = len(plan.scales)
    chunk = _compounds_per_chunk(chunk, SEQCNN_IG_ROWS_PER_CHUNK // rep)
    G, dev = tokens.shape[0], tokens.device
    ids = list(range(G)) if proteins is None else [int(i) for i in proteins]

    def rows_of(part):
        return tokens[torch.as_tensor([int(i) for i in part], device=dev)]

    def predict(part):
        return torch.softmax(model(None, None, sequences=rows_of(part)), 1).cpu().numpy()

    jobs = list(_ig_jobs(predict, ids, chunk * rep, label_target, _one_job_per_compound(_host_array(labels))))
    table = model.embeddings.detach()
    res = {}
    with frozen_parameters(model):
        if batched:
            for i in range(0, len(jobs), chunk):
                part = jobs[i:i + chunk]
                cids, masks = [j[0] for j in part], np.stack([j[5] for j in part])
                tok = rows_of(cids)
                e = table[tok.long()]
                out = _seqcnn_fused_chunk(model, tok, e, plan, masks) if fused else \
                    _seqcnn_reduce(_seqcnn_copy_grads(model, e, cids, plan, masks), e, plan)
                _rows_to_host(res, cids, out)
        else:
            for j in jobs:                                   # one batch-1 pass per copy; a copy of weight 0 runs forward only
                e = table[rows_of([j[0]]).long()]
                rows = [_seqcnn_copy_grads(model, e, [j[0]], ig_plan_row(plan, r), j[5][None], need_grad=w != 0.0)
                        for r, w in enumerate(plan.weights)]
                _rows_to_host(res, [j[0]], _seqcnn_reduce({k: torch.cat([p[k] for p in rows]) for k in rows[0]}, e, plan))
    results = []
    for job in jobs:
        cid, r = job[0], res[job[0]]
        rec = {"compound_id": cid, "assay": assay_string(job[1], job[3])}
        if sequence_symbol is not None:
            rec["amino_acid_seq"] = "".join(string.ascii_uppercase[int(t)] for t in np.asarray(sequence_symbol[cid]).reshape(-1))
        data = {"embedded_layer": lambda: table[tokens[cid].long()].cpu().numpy()}
        results.append(_ig_record(rec, job, ("embedded_layer",), data, r, r["start"], r["end"]))
    return results


# -------------------------------------------------------------------------------------------------
# the link-prediction model (sample_kg/network_prediction/model_py/{gcn,distmult,ip}.py): kgcn/visualization.py:289-439
# (KnowledgeGraphVisualizer, cal_feature_IG_for_kg), many targets per launch
# -------------------------------------------------------------------------------------------------
KG_VISUALIZE_TYPES = ("edge_score", "edge_loss", "node")
KG_IG_NODE_BYTES = 512 << 20          # default bound of one launch's node_ig [T, N] (reduce='node')
KG_IG_FULL_BYTES = 256 << 20          # ... and of one launch's u [T, N, C] (reduce=None)


def _kg_targets(visualize_type, label_list, target, num_nodes):
    """-> the target indices: `target` (an int or a sequence), or every label row / every node (:401-407)."""
    import numpy as np
    n = num_nodes if visualize_type == "node" else len(label_list)
    if target is None:
        return np.arange(n, dtype=np.int64)
    ids = np.atleast_1d(np.asarray(target, np.int64)).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= n):
        raise ValueError("visualize target outside 0..%d" % (n - 1))
    return ids


def _kg_table_ig(model, label_list, visualize_type, ids, scales, weights, method, reduce):
    """distmult / ip: s = sum_d e_a e_b w_r is bilinear in the table, so IG[a] = e_a w e_b sum_k w_k alpha_k in closed form."""
    import numpy as np
    if visualize_type != "edge_score":
        raise ValueError("visualize_type %r is not defined for the %r model: the reference's model.loss[target] and "
                         "prediction[:, target, idx] exist for model_py/gcn.py only (distmult.py / ip.py set model.score alone)"
                         % (visualize_type, model.variant))
    E = model.embedding.detach()
    f = float(sum(s * w for s, w in zip(scales, weights)))
    rows = np.asarray(label_list)[ids]
    results = []
    for tid, row in zip(ids, rows):
        a, r, b = int(row[0]), int(row[1]), int(row[2])
        w = model.distmult.w[0][r].detach() if model.distmult is not None else torch.ones_like(E[0])
        ga, gb = E[b] * w * f, E[a] * w * f                       # sum_k w_k d s / d (alpha_k E) rows a and b
        ig = torch.zeros_like(E)
        ig[a] += ga if method == "grad" else ga * E[a]
        ig[b] += gb if method == "grad" else gb * E[b]
        s = float((E[a] * E[b] * w).sum())
        rec = {"target": int(tid), "vis_nodes": [a, b], "node_ig": ig.sum(-1).cpu().numpy(), "start_score": 0.0, "end_score": s}
        if reduce is None:
            rec["ig"] = ig.cpu().numpy()
        rec["sum_of_ig"] = float(rec["node_ig"].astype(np.float64).sum())
        results.append(rec)
    return results


def linkpred_ig_stash(model, adj, scales):
    """What linkpred_integrated_gradients computes ONCE for all targets of a models.LinkPredictionNet('gcn') on the one-graph
    BatchedAdjacency `adj`: E, w1, b1, w2, p = E W1, g1 = A p, rowsum = A 1 (fp64 on the host, rounded once) and
    h2 [K, N, C] = conv2(relu(scales[k] * g1 + rowsum (x) b1)), the layer-2 output at every scale -- the operands of ops.kg_ig.
    Layer 1 is affine in the scale, so its K forwards are K scaled adds; layer 2 runs K times through the model's own layer."""
    import numpy as np
    from . import ops
    csr = adj.channels[0]
    N = model.num_nodes
    with torch.no_grad():
        if not model.conv1.built or not model.conv2.built:
            model.node_rows(adj)
        E = model.embedding.detach().contiguous()
        w1, b1 = model.conv1.w[0].detach(), model.conv1.bias[0].detach().reshape(-1)
        w2 = model.conv2.w[0].detach()
        p = ops.dense(E, w1)
        g1 = ops.bspmm(csr, p)
        rp = csr.rowptr.cpu().numpy().astype(np.int64)
        vals = csr.values.cpu().numpy().astype(np.float64)
        rowsum = torch.from_numpy(np.bincount(np.repeat(np.arange(N), np.diff(rp)), weights=vals, minlength=N)).to(torch.float32).to(E.device)
        bias_rows = rowsum[:, None] * b1[None, :]
        h2 = torch.empty((len(scales), N, w2.shape[1]), device=E.device, dtype=torch.float32)
        for k, al in enumerate(scales):
            z1 = g1 * float(np.float32(al)) + bias_rows
            h2[k] = model.conv2(torch.relu(z1).view(1, N, -1), adj=adj).view(N, -1)
    return dict(E=E, w1=w1, b1=b1, w2=w2, p=p, g1=g1, rowsum=rowsum, h2=h2)


def linkpred_integrated_gradients(model, adjs, label_list, visualize_type="edge_score", target=None, divide_number=30, method="ig",
                                  reduce="node", chunk=None):
    """`kgcn visualize` of sample_kg/network_prediction (cal_feature_IG_for_kg, KnowledgeGraphVisualizer): integrated gradients
    with respect to the embedded layer of
      edge_score  model.score[target] = s1 of label row `target` (columns 0 and 2),
      edge_loss   model.loss[target]  = -log(sigmoid(s1 - s2) + 1e-10) of the row (columns 0, 2 against 3, 5),
      node        prediction[:, target, argmax_j prediction[:, target, j]]: node `target` paired with its best partner at scale 1.
    target: an index, a sequence of them, or None = every label row (every node for 'node'), as --visualize_target unset.
    Returns one dict per target: target, vis_nodes (and partner for 'node'), node_ig [N] (the attribution summed over the embedding axis: all that
    _dump_dml reads), sum_of_ig, start_score / end_score (the attributed quantity at scale 0 and 1: the reference's check),
    and with reduce=None also ig [N, De].

    gcn: models.LinkPredictionNet('gcn').  The K scaled forwards are run ONCE for all targets (layer 1 is affine in the scale,
    layer 2 is stashed as [K, N, 128]); the per-target work is one launch of ops.kg_ig over `chunk` targets (default: as many as
    keep one launch's output under KG_IG_NODE_BYTES, or KG_IG_FULL_BYTES of u for reduce=None).  reduce=None forms the full
    attribution E (.) ((A^T u) W1^T) with the existing SpMM and dense ops: meant for a handful of targets.
    distmult / ip: edge_score only, in closed form.
    The attribution multiplies by the TRAINED table (the reference's model.embedding(sess, ...) re-initialises it)."""
    import numpy as np
    from . import models, ops
    from .batched_csr import as_batched_adjacency
    if not isinstance(model, models.LinkPredictionNet):
        raise TypeError("linkpred_integrated_gradients needs a models.LinkPredictionNet, got %s" % type(model).__name__)
    if visualize_type not in KG_VISUALIZE_TYPES:
        raise ValueError("visualize_type must be one of %s, got %r" % (", ".join(KG_VISUALIZE_TYPES), visualize_type))
    if reduce not in ("node", None):
        raise ValueError("reduce must be 'node' or None")
    scales, weights = ig_scales(method, divide_number)
    if method == "grad" and reduce == "node":
        raise ValueError("method 'grad' is not multiplied by the table: it has no node-reduced form (use reduce=None)")
    label_list = np.asarray(label_list)
    if visualize_type != "node" and (label_list.ndim != 2 or label_list.shape[1] != 6):
        raise ValueError("label_list must be [M, 6]")
    N = model.num_nodes
    ids = _kg_targets(visualize_type, label_list, target, N)
    if model.variant != "gcn":
        return _kg_table_ig(model, label_list, visualize_type, ids, scales, weights, method, reduce)
    if adjs is None:
        raise ValueError("the gcn variant needs the graph (adjs)")
    adj = as_batched_adjacency(adjs)
    if adj.num_channels != 1 or adj.num_graphs != 1 or adj.n_nodes != N:
        raise ValueError("the link-prediction graph is one adjacency channel of one %d-node graph" % N)
    csr = adj.channels[0]
    K = len(scales)
    with torch.no_grad():
        st = linkpred_ig_stash(model, adj, scales)
        E, w1, b1, w2, p, g1, rowsum, h2 = (st[k] for k in ("E", "w1", "b1", "w2", "p", "g1", "rowsum", "h2"))
        dev = E.device
        # the targets as (a, b, a', b') rows
        if visualize_type == "node":
            pred, _ = model.predict(adj)
            partner = pred[0][torch.as_tensor(ids, device=dev)].argmax(dim=1).cpu().numpy()
            tg = np.stack([ids, partner, np.full_like(ids, -1), np.full_like(ids, -1)], 1)
            vis = [[int(t)] for t in ids]
            partners = [int(j) for j in partner]
        else:
            rows = label_list[ids].astype(np.int64)
            if visualize_type == "edge_loss":
                tg = rows[:, [0, 2, 3, 5]]
            else:
                tg = np.concatenate([rows[:, [0, 2]], np.full((len(ids), 2), -1, np.int64)], 1)
            vis = [[int(r[0]), int(r[2])] for r in rows]
            partners = None
        mode = "loss" if visualize_type == "edge_loss" else "score"
        if chunk is None:
            per = 4 * N * (1 if reduce == "node" else w2.shape[0] + 1)
            chunk = max(1, (KG_IG_NODE_BYTES if reduce == "node" else KG_IG_FULL_BYTES) // per)
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        sc = torch.tensor(np.asarray(scales, np.float32), device=dev)
        wt = torch.tensor(np.asarray(weights, np.float32), device=dev)
        results = []
        for c0 in range(0, len(ids), chunk):
            part = tg[c0:c0 + chunk].astype(np.int32)
            node_ig, score, u = ops.kg_ig(csr, g1, rowsum, b1, w2, h2, p, sc, wt, part, mode=mode, want_u=reduce is None)
            nig = node_ig.cpu().numpy()
            s = score.cpu().numpy().astype(np.float64)
            if mode == "loss":                                   # the attributed quantity is the cost of s1 - s2
                with np.errstate(over="ignore"):
                    s = -np.log(1.0 / (1.0 + np.exp(-s)) + 1e-10)
            full = None
            if reduce is None:
                T = part.shape[0]
                full = []
                w1t = w1.t().contiguous()
                for t in range(T):
                    de = ops.dense(ops.bspmm(csr.transpose(), u[t]), w1t)
                    full.append((de if method == "grad" else de * E).cpu().numpy())
            for t in range(part.shape[0]):
                rec = {"target": int(ids[c0 + t]), "vis_nodes": vis[c0 + t], "node_ig": nig[t],
                       "start_score": float(s[t, 0]), "end_score": float(s[t, K - 1])}
                if partners is not None:
                    rec["partner"] = partners[c0 + t]
                if full is not None:
                    rec["ig"] = full[t]
                    rec["sum_of_ig"] = float(full[t].astype(np.float64).sum())
                else:
                    rec["sum_of_ig"] = float(nig[t].astype(np.float64).sum())
                results.append(rec)
    return results


def kg_undirected_edges(indptr, indices):
    """The distinct undirected edges (u <= v, sorted, self loops included) of a CSR pattern -> int64 [E, 2]."""
    import numpy as np
    indptr = np.asarray(indptr, np.int64).reshape(-1)
    indices = np.asarray(indices, np.int64).reshape(-1)
    rows = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    return np.unique(np.stack([lo, hi], 1), axis=0) if rows.size else np.zeros((0, 2), np.int64)


def kg_subgraph(indptr, indices, vis_nodes, graph_distance, und=None):
    """_dump_dml (:364-374) without networkx: the graph is undirected there (nx.from_scipy_sparse_matrix: an edge wherever A or
    A^T has an entry, self loops included), the node set grows by `graph_distance` rounds of neighbours from vis_nodes (a BFS
    over the CSR and its transpose), and the subgraph is the one induced on it -> (nodes ascending, edges (u, v) with u <= v,
    sorted).  networkx's own node and edge order (insertion order) is not reproduced."""
    import numpy as np
    N = np.asarray(indptr).reshape(-1).shape[0] - 1
    und = kg_undirected_edges(indptr, indices) if und is None else und
    inside = np.zeros(N, bool)
    inside[np.asarray(list(vis_nodes), np.int64)] = True
    for _ in range(int(graph_distance)):
        touch = inside[und[:, 0]] | inside[und[:, 1]]
        inside[und[touch, 0]] = True
        inside[und[touch, 1]] = True
    keep = inside[und[:, 0]] & inside[und[:, 1]]
    return np.nonzero(inside)[0], und[keep]


def kg_dump_name(visualize_type, vis_nodes):
    """:425, :433."""
    if visualize_type == "node":
        return "nodepred-%d" % int(vis_nodes[0])
    return "edgepred-%d-%d" % (int(vis_nodes[0]), int(vis_nodes[1]))


def dump_kg(result, adjs, outdir, graph_distance, visualize_type=None):
    """KnowledgeGraphVisualizer.dump / _dump_dml (:348-386) for the dicts of linkpred_integrated_gradients (one or a list):
    <name>-edge.csv holds the `u,v` lines of the subgraph within graph_distance hops of the vis_nodes, <name>-node.csv starts with
    `label,ig` and has one line per subgraph node with ig = (node_ig - mean) / std over ALL nodes.  name = edgepred-{n1}-{n2} for
    two vis_nodes, nodepred-{t} for one (or as visualize_type says).  adjs: the graph (BatchedAdjacency / BatchedCSR, read back
    once) or a host (indptr, indices) pair.  Edges are written u <= v, sorted, nodes ascending: networkx's order is not
    reproduced.  Returns the list of (edge file, node file)."""
    import os
    import numpy as np
    results = [result] if isinstance(result, dict) else list(result)
    if isinstance(adjs, (tuple, list)) and len(adjs) == 2 and not hasattr(adjs[0], "rowptr"):
        indptr, indices = adjs
    else:
        from .batched_csr import as_batched_adjacency
        csr = as_batched_adjacency(adjs).channels[0]
        indptr, indices = csr.rowptr.cpu().numpy(), csr.cv[:, 0].cpu().numpy()
    os.makedirs(outdir, exist_ok=True)
    und = kg_undirected_edges(indptr, indices)
    files = []
    for rec in results:
        vis = list(rec["vis_nodes"])
        kind = visualize_type if visualize_type is not None else ("node" if len(vis) == 1 else "edge_score")
        name = kg_dump_name(kind, vis)
        ig = np.asarray(rec["node_ig"], np.float64).reshape(-1)
        norm = (ig - ig.mean()) / ig.std()
        nodes, edges = kg_subgraph(indptr, indices, vis, graph_distance, und)
        ef, nf = os.path.join(outdir, name + "-edge.csv"), os.path.join(outdir, name + "-node.csv")
        with open(ef, "w") as f:
            for u, v in edges:
                f.write("%d,%d\n" % (u, v))
        with open(nf, "w") as f:
            f.write("label,ig\n")
            for n in nodes:
                f.write("%d,%s\n" % (n, repr(float(norm[n]))))
        files.append((ef, nf))
    return files


# -------------------------------------------------------------------------------------------------
# the compound-protein interaction multitask network (sample_chem/compound-protein_interaction/multitask.py:35-51, run_viz.sh
# block name=mt): kgcn/visualization.py:187-286 and :442-574, fused over the scaled copies (csrc/cpiig.hip)
# -------------------------------------------------------------------------------------------------
CPI_IG_MODALS = ("features", "adjs")
CPI_IG_FULL_BYTES = 256 << 20         # default bound of one sweep's G tensors [C, T, N, Wd] (one or two of them)
CPI_IG_DENSE_ROWS = 1023              # rows of one dense call of the fused route: below the dense op's 1,024-row table routes


def cpi_ig_coefficients(modal, method, divide_number=100):
    """The per-copy coefficients of the fused route for one modal set and method -> dict:
      targets        the inputs that are scaled and attributed: ('features', 'adjs') for 'all', else the one named
      scales, weights  ig_scales(method, divide_number): s_k and w_k, K = len(scales) copies
      alpha, gamma   copy k's pre-activation is alpha[k] P + gamma[k] Q: alpha = a c, gamma = c with a = s where the features
                     are a target (else 1) and c = s where the adjacency values are (else 1; kgcn/feed.py:116-121 scales the
                     values of EVERY channel)
      wA, wB         the copy weights of the two G tensors of ops.cpi_ig (wB None: one tensor): G^A = sum_k w_k beta_k G_k with
                     beta = c for the features and beta = a for the Y0 term of the adjacency values -- for 'all' both are s,
                     for a single modal both are 1 -- and G^B = sum_k w_k G_k, the bias term of the adjacency values, which
                     is G^A itself unless both modals are targets
      bias_from      'A' or 'B': the tensor that carries that bias term.
    Refused: 'embedded_layer' (the network has none) and the smooth methods (per-element noise leaves the two-parameter family
    alpha P + gamma Q)."""
    if modal == "all":
        targets = CPI_IG_MODALS
    elif modal in CPI_IG_MODALS:
        targets = (modal,)
    else:
        raise ValueError("modal must be 'all', 'features' or 'adjs' for the compound-protein interaction network, got %r" % (modal,))
    if method in SMOOTH_METHODS:
        raise ValueError("method %r adds per-element noise: the scaled copies are no longer alpha P + gamma Q (use "
                         "integrated_gradients, the per-step loop)" % (method,))
    scales, weights = ig_scales(method, divide_number)
    both = len(targets) == 2
    a = list(scales) if "features" in targets else [1.0] * len(scales)
    c = list(scales) if "adjs" in targets else [1.0] * len(scales)
    return {"targets": targets, "scales": list(scales), "weights": list(weights),
            "alpha": [ak * ck for ak, ck in zip(a, c)], "gamma": c,
            "wA": [w * s for w, s in zip(weights, scales)] if both else list(weights),
            "wB": list(weights) if both else None, "bias_from": "B" if both else "A"}


def cpi_dump_record(result):
    """The dict CompoundVisualizer.dump writes (:133-160) for one result of cpi_integrated_gradients."""
    return {k: v for k, v in result.items() if k not in ("compound_id", "task", "assay", "start_score", "end_score")}


def _cpi_dense(x2d, w, rows_per_graph):
    """x2d @ w through ops.dense in slices of whole compounds of at most CPI_IG_DENSE_ROWS rows: every compound takes the same
    GEMM kernel however many share the chunk (the dense op picks another kernel from 1,024 rows on), so that chunking leaves
    the bits alone."""
    from . import ops
    m = x2d.shape[0]
    per = max(1, CPI_IG_DENSE_ROWS // int(rows_per_graph)) * int(rows_per_graph)
    if m <= per:
        return ops.dense(x2d, w)
    return torch.cat([ops.dense(x2d[i:i + per], w) for i in range(0, m, per)])


def _cpi_fused_chunk(dataset, part, par, coef, method):
    """The fused route for the compounds `part` and the tasks of par['u'] -> {features [C, T, N, F], adjs / adjs_data, start, end}."""
    import numpy as np
    from . import ops
    targets = coef["targets"]
    adj, x = dataset.batch(part)
    C, N, F = x.shape
    W, b, u, e = par["W"], par["b"], par["u"], par["e"]
    Wd, Tn = W[0].shape[1], u.shape[0]
    x2d = x.reshape(C * N, F)
    ones = torch.ones((C * N, 4), device=x.device, dtype=torch.float32)
    P = Q = Y0 = None
    for ch, csr in enumerate(adj.channels):                  # the two aggregated products, once per compound
        y = _cpi_dense(x2d, W[ch], N)
        Y0 = y if ch == 0 else Y0
        pc = ops.bspmm(csr, y)
        qc = ops.bspmm(csr, ones)[:, :1] * b[ch].view(1, Wd)
        P, Q = (pc, qc) if P is None else (P + pc, Q + qc)
    p, GA, GB = ops.cpi_ig(P.view(C, N, Wd), Q.view(C, N, Wd), u, e, coef["alpha"], coef["gamma"], coef["wA"], coef["wB"])
    # the contraction: one ordinary GraphConv backward per (compound, task) -- the adjacency of every compound batched T times
    rows = np.repeat(np.asarray(part, np.int64), Tn)
    g2d = GA.view(C * Tn * N, Wd)
    raw = method == "grad"
    out = {"start": p[:, 0, :], "end": p[:, -1, :], "features_data": x}
    chT = [c.gather(rows) for c in (dataset.channels if "features" in targets else dataset.channels[:1])]
    if "features" in targets:
        dx = None
        for ch, csr in enumerate(chT):
            d = _cpi_dense(ops.bspmm(csr.transpose(), g2d), par["Wt"][ch], N)
            dx = d if dx is None else dx + d
        dx = dx.view(C, Tn, N, F)
        out["features"] = dx if raw else dx * x.view(C, 1, N, F)
    if "adjs" in targets:
        csr0 = chT[0]
        y0 = Y0.view(C, 1, N, Wd).expand(C, Tn, N, Wd).reshape(C * Tn * N, Wd)
        gb = g2d if coef["bias_from"] == "A" else GB.view(C * Tn * N, Wd)
        dv = ops.spmm_values_grad(csr0, g2d, y0) + ops.spmm_values_grad(csr0, gb, b[0].reshape(-1), rhs_ld=0, rhs_gs=0)
        out["adjs"] = values_to_dense(csr0, dv if raw else dv * csr0.values).view(C, Tn, N, N)
        out["adjs_data"] = values_to_dense(adj.channels[0], adj.channels[0].values)
    return out


def _cpi_composed_chunk(model, dataset, part, tasks, plan, targets):
    """The composed route: the copies of every compound as batch rows of one forward through the model (_graph_copies), one
    autograd backward per task, the copies summed in order (_reduce_graph_copies) and the tasks stacked -> what _cpi_fused_chunk
    returns."""
    C, rep = len(part), len(plan.scales)
    g = _graph_copies(dataset, part, plan, targets)
    p1 = torch.softmax(model(g.x_in, g.adj_in), dim=1)[:, 1, :]                   # prediction[:, t, 0] of every task
    wrt = ([g.x_in] if "features" in targets else []) + ([g.v0] if g.v0 is not None else [])
    data = _copies_data(g, targets)
    per_task = []
    for j, t in enumerate(tasks):
        gr = _copies_grads(data, g, targets, list(torch.autograd.grad(p1[:, t].sum(), wrt, retain_graph=j + 1 < len(tasks))))
        gr["score"] = p1[:, t].detach()
        per_task.append(_reduce_graph_copies(gr, C, plan, targets))
    out = {m: torch.stack([r[m] for r in per_task], 1) for m in targets + ("start", "end")}
    out["features_data"] = g.x.view(C, rep, g.x.shape[1], g.x.shape[2])[:, 0]
    if "adjs" in targets:
        out["adjs_data"] = per_task[0]["adjs_data"]
    return out


def cpi_integrated_gradients(model, features, adjacency, labels=None, divide_number=100, modal="all", method="ig",
                             label_target="max", tasks=None, compounds=None, chunk=None, fused=True):
    """`kgcn visualize` of the compound-protein interaction sample (run_viz.sh, block name=mt) for a models.CPIMultitaskNet: integrated
    gradients of every task's prediction[:, t, 0] -- the two-way softmax's second entry, sigmoid(h . u_t + e_t) -- with respect to
    the node features and / or the values of adjacency channel 0 (modal 'all', 'features', 'adjs'), by the protocol of the section
    above -> its records, one per (compound, task), which also hold task, start_score and end_score (the prediction of the first
    and the last copy; cpi_dump_record drops these beside compound_id and assay; ig_filename(..., task=t) uses task).

    labels [G, T]: the true label of task t is labels[cid, t] for T > 1, argmax(labels[cid]) for one task.  The target is chosen on
    the one-entry prediction [p1] (:497-529), so label_target 'label' with label 1 indexes outside it and raises, as it would in
    the reference.  tasks: the tasks to visualise (default all).  method 'ig', 'grad_prod' or 'grad'.

    fused=True: the network is one GraphConv, a sigmoid, a sum and one Dense, so copy k's pre-activation is
    alpha_k P + gamma_k Q (cpi_ig_coefficients): P, Q and Y0 = X W_0 are formed once per compound by the dense and SpMM ops,
    ops.cpi_ig sweeps the copies, and the sums it returns go through ONE GraphConv input gradient (A^T G W^T) and SpMM values
    gradient per (compound, task).  Compounds run `chunk` at a time (default: as many as keep the G tensors under
    CPI_IG_FULL_BYTES); chunking does not change a bit of any compound's rows.
    fused=False: the copies run as batch rows through the model itself with one autograd backward per task (`chunk` defaults to
    IG_ROWS_PER_CHUNK // copies).

    Unlike the reference, every (compound, task) differentiates its OWN prediction: the reference builds its gradient graph for
    the first visualised compound and task and reuses it (tf_grads, :466 and :555)."""
    import numpy as np
    from . import models
    if not isinstance(model, models.CPIMultitaskNet):
        raise TypeError("cpi_integrated_gradients needs a models.CPIMultitaskNet (the closed form is that network's), got %s"
                        % type(model).__name__)
    coef = cpi_ig_coefficients(modal, method, divide_number)
    targets, plan = coef["targets"], ig_row_plan(method, divide_number)
    dataset = _compound_dataset(features, adjacency, lambda: _parameter_device(model))
    G, T = dataset.num_graphs, model.label_dim
    ids = list(range(G)) if compounds is None else [int(i) for i in compounds]
    tasks = list(range(T)) if tasks is None else [int(t) for t in np.atleast_1d(tasks)]
    if not tasks or min(tasks) < 0 or max(tasks) >= T:
        raise ValueError("tasks must name some of the network's %d tasks" % T)
    lab = _host_array(labels)
    N, Wd = dataset.features.shape[1], model.conv.output_dim
    chunk = _compounds_per_chunk(chunk, CPI_IG_FULL_BYTES // (4 * len(tasks) * N * Wd * (1 if coef["wB"] is None else 2)) if fused
                                 else IG_ROWS_PER_CHUNK // len(plan.scales))

    def predict(part):
        adj, x = dataset.batch(part)
        return torch.softmax(model(x, adj), dim=1)[:, 1, :].cpu().numpy()

    def entries(cid, row):                                   # one attribution per task, of the one-entry prediction [p1]
        return [((cid, t), row[t:t + 1], None if lab is None else int(lab[cid, t]) if T > 1 else int(np.argmax(lab[cid])))
                for t in tasks]

    jobs = list(_ig_jobs(predict, ids, max(1, IG_ROWS_PER_CHUNK // 8), label_target, entries))
    wanted = sorted({j[0][0] for j in jobs}, key=ids.index)
    res = {}
    with frozen_parameters(model):
        if fused and wanted:
            V, c = model.out.kernel.detach(), model.out.bias.detach()
            ts = torch.as_tensor(tasks, device=V.device)
            par = {"W": [w.detach().contiguous() for w in model.conv.w], "b": [b.detach().reshape(-1) for b in model.conv.bias],
                   "u": (V[:, T:] - V[:, :T]).t()[ts].contiguous(), "e": (c[T:] - c[:T])[ts].contiguous()}
            par["Wt"] = [w.t().contiguous() for w in par["W"]]
        for i in range(0, len(wanted), chunk):
            part = wanted[i:i + chunk]
            with torch.set_grad_enabled(not fused):
                out = _cpi_fused_chunk(dataset, part, par, coef, method) if fused else \
                    _cpi_composed_chunk(model, dataset, part, tasks, plan, targets)
            host = _rows_to_host(res, part, out)
            # sum_of_IG of every (compound, task) at once: the fp64 sum of the record's own arrays, one modal after the other
            total = sum(host[m].astype(np.float64).reshape(len(part), len(tasks), -1).sum(-1) for m in targets)
            for k, cid in enumerate(part):
                res[cid]["total"] = total[k]
    results = []
    for job in jobs:
        (cid, t), pred, tidx = job[0], job[1], job[3]
        r, k = res[cid], tasks.index(t)
        rec = {"compound_id": cid, "task": t, "assay": assay_string(pred, tidx),
               "start_score": float(r["start"][k]), "end_score": float(r["end"][k])}
        data = {"features": lambda: r["features_data"], "adjs": lambda: r["adjs_data"]}
        results.append(_ig_record(rec, job, targets, data, {m: r[m][k] for m in targets}, rec["start_score"], rec["end_score"],
                                  sum_of_ig=r["total"][k]))
    return results
