"""fp64 restatement of the smooth attribution methods of the multimodal model (kgcn/visualization.py:235-259 smooth_grad and
smooth_ig, CompoundVisualizer on example_model/model_multimodal.py) and of the noise the HIP kernels draw for them.

  noise()   the contract of include/kgcn_hip.h: one N(0, 1) per (seed, stream s, compound g, sample k, row r, column w) of a 2-D
            array [R, W] = normal number w & 3 of the Philox4x64-10 block with counter (r ceil(W / 4) + (w >> 2), k, g, s) and key
            (seed, 0); Philox and Box-Muller are vae_oracle's (imported, not edited).
  smooth()  the reference's literal loop: one batch-1 pass per step through add_perturbation (kgcn/feed.py:88-89), with the
            host's np.random.normal replaced by noise(); forward and backward are multimodal_ig_oracle's.
Streams: 0 the node features [N, F]; 1 + ch the stored values of adjacency channel ch as [1, nnz] in CSR order; 0x100 the embedded
sequence [L, E]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multimodal_ig_oracle as IG  # noqa: E402
import vae_oracle as VO  # noqa: E402

F64 = np.float64
STREAM_FEATURES, STREAM_ADJACENCY, STREAM_SEQUENCE = 0, 1, 0x100
METHODS = ("smooth_grad", "smooth_ig")


def noise_words(seed, s, g, k, first, count):
    """Philox words of blocks first .. first + count - 1 of (seed, s, g, k): counter (block, k, g, s), key (seed, 0)."""
    ctr = np.zeros((count, 4), np.uint64)
    ctr[:, 0] = np.arange(first, first + count, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.uint64(k), np.uint64(g), np.uint64(s)
    key = np.zeros((count, 2), np.uint64)
    key[:, 0] = np.uint64(seed % 2 ** 64)
    return VO.philox4x64_10(ctr, key)


def noise(seed, s, g, k, R, W):
    """-> fp64 [R, W]."""
    W4 = (W + 3) // 4
    if R * W4 == 0:
        return np.zeros((R, W), F64)
    return VO.normals(noise_words(seed, s, g, k, 0, R * W4)).reshape(R, 4 * W4)[:, :W]


def add_perturbation(x, scaling, z, noise_scale):
    """kgcn/feed.py:88-89 with enabled_noise: x * scaling + N(0, noise_scale), the normal being noise_scale * z."""
    return x * scaling + noise_scale * z


def csr_entries(S):
    """The stored entries of the mask S [C, N, N] per channel, in row-major order (the CSR order of a sorted COO list)."""
    return [np.argwhere(S[c]) for c in range(S.shape[0])]


def perturbed_inputs(x, A, S, emb, pert, scaling, noise_scale, seed, g, k, entries=None):
    """The feeds of step k: every input named in pert through add_perturbation (the values of every adjacency channel)."""
    xs, As, es = x, A, emb
    if "features" in pert:
        xs = add_perturbation(x, scaling, noise(seed, STREAM_FEATURES, g, k, *x.shape), noise_scale)
    if "adjs" in pert:
        entries = csr_entries(S) if entries is None else entries
        As = A.copy()
        for ch, idx in enumerate(entries):
            idx = np.asarray(idx).reshape(-1, 2)
            z = noise(seed, STREAM_ADJACENCY + ch, g, k, 1, len(idx))[0]
            As[ch][idx[:, 0], idx[:, 1]] = add_perturbation(A[ch][idx[:, 0], idx[:, 1]], scaling, z, noise_scale)
    if "embedded_layer" in pert:
        es = add_perturbation(emb, scaling, noise(seed, STREAM_SEQUENCE, g, k, *emb.shape), noise_scale)
    return xs, As, es


def smooth(p, x, A, S, emb, mask, D, modal, method, noise_scale, seed, g, act="hard_sigmoid", pool=4, entries=None):
    """cal_integrated_gradients (:235-259) and check_IG (:279-286) for compound g: x [N, F], A [C, N, N] with its stored-entry
    mask S, emb [L, E] -> {modal + '_IG', 'start_score', 'end_score', 'check_score', 'sum_of_IG'}.  entries: per channel the
    [nnz, 2] stored entries in the order the noise of the values is indexed by (default row-major, no repeated entry)."""
    if method not in METHODS:
        raise ValueError(method)
    x, A, emb = np.asarray(x, F64), np.asarray(A, F64), np.asarray(emb, F64)
    pert = list(IG.MODALS) if modal == "all" else [modal]
    data = {"features": x, "adjs": A[0], "embedded_layer": emb}
    IGs = {m: np.zeros(data[m].shape, F64) for m in pert}
    for k in range(D):
        scaling_coef = 1.0 if method == "smooth_grad" else (k + 1) / float(D)
        xs, As, es = perturbed_inputs(x, A, S, emb, pert, scaling_coef, noise_scale, seed, g, k, entries)
        _, out_grads = IG.input_grads(p, xs, As, S, es, mask, 1.0, (), act, pool)
        for m in IGs:
            if method == "smooth_grad":
                IGs[m] += out_grads[m] / float(D)
            else:
                IGs[m] += out_grads[m] * data[m] / float(D)
    start = IG.input_grads(p, x, A, S, emb, mask, 0.0, pert, act, pool)[0]
    end = IG.input_grads(p, x, A, S, emb, mask, 1.0, pert, act, pool)[0]
    out = {m + "_IG": v for m, v in IGs.items()}
    out["start_score"], out["end_score"], out["check_score"] = start, end, end - start
    out["sum_of_IG"] = float(sum(v.sum() for v in IGs.values()))
    return out
