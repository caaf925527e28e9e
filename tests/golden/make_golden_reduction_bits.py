#!/usr/bin/env python3
"""Generate tests/golden/reduction_bits.npz: the BITS every loss head and metric that sums over a workgroup gave before those
sums were gathered into csrc/block_reduce.h.  Run once on the GPU with the library of the commit BEFORE that change
(KGCN_HIP_LIB=<its libkgcn_hip.so>); tests/test_gpu_reduction_bits.py replays the stored inputs and wants the stored bits.

  <case>/in_*    the inputs: N(0, 3) logits from a fixed numpy seed, labels, masks with about 80 % ones, ...  Real-valued inputs
                 are drawn as float16 and 0 / 1 arrays kept as uint8 (half and a quarter of the bytes); both are fed as float32
  <case>/out_*   raw uint32 views of what the head returned: sums / stats, the gradient of the summed cost with respect to the
                 logits, predictions, the accumulator block after two calls

Cases: the sigmoid, dense-softmax and sparse-softmax heads (csrc/train.hip; one case feeds all three the same logits) on both
sides of the 256-row workgroup, i.e. with and without the finishing launch; the softmax2 head (cvloss.hip) and the squared-error head (regress.hip) with many rows and
with more tasks than the finish kernel has threads; regression_metrics; the KL sum of vae_sample and the sums of vae_recon
(vae.hip); the sums of linkpred_loss in every mode on one label list (linkpred.hip).

    KGCN_HIP_LIB=/path/to/the/older/libkgcn_hip.so python tests/golden/make_golden_reduction_bits.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "reduction_bits.npz")

CASES = ([("train_heads_b%d" % B, "train", (B, 3)) for B in (255, 256, 257, 513)]
         + [("%s_b%d_t%d" % (head, B, T), head, (B, T)) for head in ("softmax2", "sqerr") for B, T in ((257, 3), (2, 257))]
         + [("regression_metrics_n257_t3", "regression_metrics", (257, 3))]
         + [("vae_kl_d%d" % D, "vae_kl", (3, 5, D)) for D in (1, 64)]
         + [("vae_recon", "vae_recon", (3, 5, 1, 4))]
         + [("linkpred_l%d" % L, "linkpred", (L,)) for L in (7, 257)])
LINKPRED_MODES = ("gcn", "distmult", "ip")


def _ones80(rng, shape):
    return (rng.random(shape) < 0.8).astype(np.uint8)


def inputs(head, p, rng):
    """-> {name: array}, everything the case feeds its head"""
    n3 = lambda *shape: (rng.standard_normal(shape) * 3.0).astype(np.float16)          # noqa: E731
    coin = lambda p, *shape: (rng.random(shape) < p).astype(np.uint8)                  # noqa: E731
    if head == "train":                                             # the three heads of train.hip on one set of logits
        B, W = p
        return {"logits": n3(B, W), "labels": coin(0.5, B, W), "label_idx": rng.integers(0, W, B).astype(np.uint8), "mask": _ones80(rng, B),
                "mask_label": _ones80(rng, (B, W)), "pos_weight": np.array([0.5, 2.0, 7.5], np.float32)[:W]}
    if head == "softmax2":
        B, T = p
        return {"logits": n3(B, 2, T), "labels": coin(0.5, B, T), "mask_label": _ones80(rng, (B, T))}
    if head == "sqerr":
        B, T = p
        return {"pred": n3(B, T), "labels": n3(B, T), "mask_label": _ones80(rng, (B, T))}
    if head == "regression_metrics":
        n, T = p
        y = (rng.random((n, T)) * 3.0 + 0.1).astype(np.float16)
        return {"label": y, "pred": (y * np.exp(0.2 * rng.standard_normal((n, T)))).astype(np.float16), "mask": _ones80(rng, (n, T))}
    if head == "vae_kl":
        B, N, D = p
        return {"ms": n3(B, 2 * D), "eps": rng.standard_normal((B, N, D)).astype(np.float16)}
    if head == "vae_recon":
        B, N, C, F = p
        D = 8
        return {"adj": coin(0.4, B, C, N, N), "y": rng.random((C, B, N, D)).astype(np.float16),
                "w": rng.uniform(-0.3, 0.3, (C, D)).astype(np.float16), "feat_logits": n3(B, N, F), "feat_target": coin(0.4, B, N, F),
                "mask": np.array([1] * (B - 1) + [0], np.uint8), "kl": rng.standard_normal(B).astype(np.float16)}
    if head == "linkpred":
        L, N, D, R = p[0], 24, 8, 3
        lab = np.stack([rng.integers(0, N, L), rng.integers(0, R, L), rng.integers(0, N, L), rng.integers(0, N, L),
                        rng.integers(0, R, L), rng.integers(0, N, L)], 1).astype(np.uint8)
        return {"label_list": lab, "h": rng.standard_normal((N, D)).astype(np.float16), "w": rng.standard_normal((R, D)).astype(np.float16)}
    raise ValueError(head)


def bits(*tensors):
    """the raw 32-bit words of the tensors, one after the other, as a CPU int32 tensor"""
    import torch
    return torch.cat([t.detach().contiguous().reshape(-1).view(torch.int32).cpu() for t in tensors])


def run(head, p, inp):
    """-> {name: int32 CPU tensor of bits}, what the case's head returns for these inputs on cuda:0"""
    import torch
    from kgcn_amd import data_util, ops
    from kgcn_amd.batched_csr import as_batched_adjacency
    t = {k: torch.as_tensor(v.astype(np.float32) if v.dtype in (np.float16, np.uint8) else v, device="cuda:0") for k, v in inp.items()}
    if head == "train":
        out = {}
        for kind in ("sigmoid", "softmax", "sparse"):
            x = t["logits"].clone().requires_grad_(True)
            if kind == "sigmoid":
                cost_opt, cost_sum = ops.masked_sigmoid_ce(x, t["labels"], t["mask"], t["mask_label"], pos_weight=t["pos_weight"])
            elif kind == "softmax":
                onehot = torch.nn.functional.one_hot(t["label_idx"].long(), p[1]).float()
                cost_opt, cost_sum = ops.masked_softmax_ce(x, onehot, t["mask"])
            else:
                cost_opt = cost_sum = ops.sparse_softmax_ce_sum(x, t["label_idx"].long())
            cost_sum.backward()                                     # an upstream gradient of exactly 1: x.grad is the kernel's dlogits
            out[kind + "_sums"], out[kind + "_dlogits"] = bits(cost_sum, cost_opt), bits(x.grad)
        return out
    if head == "softmax2":
        T = p[1]
        x = t["logits"].requires_grad_(True)
        accum = torch.zeros(3 * T + 1, device="cuda:0")
        cost, each_cost, each_correct, each_count, pred = ops.multitask_softmax2_ce(x, t["labels"], t["mask_label"], accum=accum)
        cost.backward()
        ops.multitask_softmax2_ce(x.detach(), t["labels"], t["mask_label"], accum=accum)
        return {"stats": bits(each_cost, each_correct, each_count, cost), "pred": bits(pred), "dlogits": bits(x.grad), "accum": bits(accum)}
    if head == "sqerr":
        T = p[1]
        x = t["pred"].requires_grad_(True)
        accum = torch.zeros(2 * T + 1, device="cuda:0")
        cost_opt, cost_sum, err, cnt = ops.masked_squared_error(x, t["labels"], t["mask_label"], accum=accum)
        cost_sum.backward()
        ops.masked_squared_error(x.detach(), t["labels"], t["mask_label"], accum=accum)
        return {"stats": bits(err, cnt, cost_sum, cost_opt), "dlogits": bits(x.grad), "accum": bits(accum)}
    if head == "regression_metrics":
        return {"stats": bits(torch.as_tensor(ops.regression_metrics(t["pred"], t["label"], t["mask"])))}
    if head == "vae_kl":
        kl, _ = ops.vae_sample(t["ms"], p[1], t["eps"])
        return {"sums": bits(kl)}
    if head == "vae_recon":
        B, N, C, F = p
        adjs = [[(np.argwhere(inp["adj"][b, c]).astype(np.int32), np.ones(int(inp["adj"][b, c].sum()), np.float32), [N, N])
                 for c in range(C)] for b in range(B)]
        sums = ops.vae_recon(as_batched_adjacency(adjs, n_nodes=N, device="cuda:0"), [t["y"][c] for c in range(C)],
                             [t["w"][c] for c in range(C)], t["feat_logits"], t["feat_target"], t["mask"], t["kl"])
        return {"sums": bits(*sums)}
    if head == "linkpred":
        feed = data_util.LinkPredFeed(inp["label_list"], batch=p[0], device="cuda:0")
        step = torch.tensor(2, dtype=torch.int64, device="cuda:0")
        out = {}
        for mode in LINKPRED_MODES:
            c_opt, c_sum, correct, _, _, _ = ops.linkpred_loss(t["h"], feed, mode, w=t["w"] if mode == "distmult" else None, seed=11, step=step)
            out[mode + "_sums"] = bits(c_opt, c_sum, correct)
        return out
    raise ValueError(head)


def main():
    sys.path.insert(0, ROOT)
    out = {}
    for i, (name, head, p) in enumerate(CASES):
        inp = inputs(head, p, np.random.default_rng(1400 + i))
        got = run(head, p, inp)
        out.update({"%s/in_%s" % (name, k): v for k, v in inp.items()})
        out.update({"%s/out_%s" % (name, k): v.numpy().view(np.uint32) for k, v in got.items()})
        print("%-28s %s" % (name, "  ".join("%s[%d]" % (k, v.numel()) for k, v in got.items())))
    np.savez_compressed(PATH, **out)
    from kgcn_amd import _lib
    print("wrote %s: %d cases, %d bytes, library %s" % (os.path.basename(PATH), len(CASES), os.path.getsize(PATH), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
