"""The inputs and bounds of tests/test_gpu_loss_heads.py and tests/test_gpu_adam_forms.py, generated in numpy alone so that
tests/test_step_tail_oracle.py can run the fp64 reference (tests/step_tail_oracle.py) and its deliberately wrong variants on the
very same arrays without a GPU.

Batch sizes follow the 256-row workgroup of the loss kernels: 1 and 2, 255 / 256 (one workgroup: it writes the sums itself), 257
(the finishing launch, one live lane in the last workgroup), 513 and 1025 (three and five workgroups).

Logit regimes:
  normal  N(0, 3)
  grid    the exact values 0, +-1e-6, +-20, +-88, +-120, walked so that every column meets every value within nine rows: where
          1 / (1 + __expf(-x)) and log1pf(__expf(-|x|)) saturate, and (+-88) where __expf is next to its overflow
  equal   rows whose entries are all equal (a softmax row of 1 / C; the value N(0, 3) on even rows, a grid value on odd rows)
  spread  softmax only, C >= 2: N(0, 3) rows with one entry raised by 100 and another lowered by 100
"""
import zlib

import numpy as np

BATCHES = (1, 2, 255, 256, 257, 513, 1025)
GRID = np.array([0.0, 1e-6, -1e-6, 20.0, -20.0, 88.0, -88.0, 120.0, -120.0], np.float32)

# the bounds of the GPU comparisons (the issue of this work sets them; test_gpu_large_sizes.py uses the same for these kernels)
ARRAY_TOL = 2e-6          # cost, dlogits: error <= ARRAY_TOL * max(1, max |reference|) per compared array
SUM_TOL = 1e-6            # sums[0], sums[1]: relative; absolute where the reference is 0
# Largest errors measured on an MI355X over all batch sizes, in the units of the two bounds above (cost and dlogits: error /
# max(1, max |ref|); sums: relative error), after the three corrections of csrc/train.hip that these tests brought about:
#   head      regime   cost      dlogits   sums
#   sigmoid   normal   1.4e-7    1.6e-7    1.1e-7
#   sigmoid   grid     1.5e-7    3.7e-8    1.2e-7        (saturated logits: no worse than N(0, 3))
#   sigmoid   equal    2.7e-7    1.2e-7    2.7e-7
#   softmax   normal   2.4e-7    2.7e-7    1.2e-7
#   softmax   grid     2.2e-7    1.8e-7    1.3e-7
#   softmax   equal    2.4e-7    6.8e-8    2.3e-7
#   softmax   spread   2.9e-7    2.6e-7    1.5e-7
#   sparse    normal   7.8e-8    1.2e-7    7.8e-8
#   sparse    grid     3.6e-8    4.0e-8    1.0e-7
#   sparse    equal    2.4e-8    2.9e-8    9.2e-8
#   sparse    spread   3.9e-8    0         9.2e-8        (the softmax is one-hot in float32: dlogits are exact)
#   autograd (loss_grad_kernel, B = 257): sigmoid 8.3e-8, softmax 1.6e-7, sparse 1.1e-7 of max(1, max |ref|)
# Before the corrections: sigmoid sums 6.6e-5 relative (B = 1, T = 5, scalar weight, equal rows of -5.7), sigmoid dlogits
# 2.6e-6 (B = 2, T = 12, per-task weights, N(0, 3)), sparse sums 2.1e-6 relative (B = 1, C = 2, N(0, 3)).
ADAM_ATOL = ADAM_RTOL = 2e-6
# TF-Adam against fp64, largest over all sizes, counters and steps: p 3.0e-7 absolute (15 % of its bound where it came closest),
# v 6.4e-8 relative, m 42 % of its rounding bound (tests/test_gpu_adam_forms.py); train.TFAdam p 8.3e-8

SIGMOID_TASKS = (1, 5, 12)
SIGMOID_WEIGHTS = ("off", "scalar", "per_task")
SIGMOID_LABEL_MASKS = ("none", "p80", "task_off")
GRAPH_MASKS = ("tail", "zero")
SOFTMAX_CLASSES = (1, 2, 5, 33)
SOFTMAX_LABELS = ("onehot", "soft1", "soft_scaled", "zero_rows")
SPARSE_MASKS = ("none", "tail", "zero")
REGIMES = ("normal", "grid", "equal")
SOFTMAX_REGIMES = REGIMES + ("spread",)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_logits(regime, B, W, rng):
    b, t = np.arange(B)[:, None], np.arange(W)[None, :]
    if regime == "normal":
        x = rng.standard_normal((B, W)) * 3
    elif regime == "grid":
        x = GRID[(b + 2 * t) % 9]
    elif regime == "equal":
        row = np.where(np.arange(B) % 2 == 0, rng.standard_normal(B) * 3, GRID[np.arange(B) % 9])
        x = np.repeat(row[:, None], W, axis=1)
    elif regime == "spread":
        assert W >= 2
        x = rng.standard_normal((B, W)) * 3
        base = rng.standard_normal(B) * 3
        x[np.arange(B), np.arange(B) % W] = base + 100
        x[np.arange(B), (np.arange(B) + 1) % W] = base - 100
    else:
        raise KeyError(regime)
    return np.ascontiguousarray(x, dtype=np.float32)


def graph_mask(kind, B):
    """tail: the padded last batch (the last quarter of the rows, at least one where B >= 2, are dummies); zero: no live graph."""
    mk = np.zeros(B, np.float32)
    if kind == "tail":
        mk[:max(1, B - max(1, B // 4))] = 1
    elif kind == "ones":
        mk[:] = 1
    elif kind != "zero":
        raise KeyError(kind)
    return mk


def pos_weight_of(kind, T):
    """-> (weighted flag, scalar, per-task float32 vector or None) as kgcn_masked_sigmoid_ce_f32 takes them."""
    if kind == "off":
        return 0, 0.0, None
    if kind == "scalar":
        return 1, 2.5, None
    return 1, 0.0, np.geomspace(0.2, 40.0, T).astype(np.float32)             # T = 1: [0.2]


def sigmoid_case(B, T, weights, label_mask, mask, regime):
    rng = _rng("sigmoid", B, T, weights, label_mask, mask, regime)
    d = dict(B=B, T=T, weights=weights, label_mask=label_mask, mask_kind=mask, regime=regime)
    d["logits"] = make_logits(regime, B, T, rng)
    d["labels"] = (rng.random((B, T)) < 0.3).astype(np.float32)
    d["mask"] = graph_mask(mask, B)
    if label_mask == "none":
        d["mask_label"] = None
    elif label_mask == "p80":
        d["mask_label"] = (rng.random((B, T)) < 0.8).astype(np.float32)
    else:
        d["mask_label"] = np.ones((B, T), np.float32)
        d["mask_label"][:, (T - 1) // 2] = 0
    d["weighted"], d["q"], d["qvec"] = pos_weight_of(weights, T)
    d["pos_weight"] = None if not d["weighted"] else (d["q"] if d["qvec"] is None else d["qvec"])
    return d


def sigmoid_cases(B):
    for T in SIGMOID_TASKS:
        for w in SIGMOID_WEIGHTS:
            for lm in SIGMOID_LABEL_MASKS:
                for mk in GRAPH_MASKS:
                    for regime in REGIMES:
                        yield sigmoid_case(B, T, w, lm, mk, regime)


def soft_labels(kind, B, C, rng):
    hot = np.eye(C, dtype=np.float32)[rng.integers(0, C, B)]
    if kind == "onehot":
        return hot
    if kind == "zero_rows":                       # every third row (row 0 among them) carries no label at all
        hot[::3] = 0
        return hot
    z = rng.random((B, C)) + 0.05
    z /= z.sum(axis=1, keepdims=True)
    if kind == "soft_scaled":                     # rows that sum to 0.3 and to 2: the softmax gradient's sum_c z factor is not 1
        z *= np.where(np.arange(B) % 2 == 0, 0.3, 2.0)[:, None]
    elif kind != "soft1":
        raise KeyError(kind)
    return z.astype(np.float32)


def softmax_case(B, C, labels, mask, regime):
    rng = _rng("softmax", B, C, labels, mask, regime)
    d = dict(B=B, C=C, label_kind=labels, mask_kind=mask, regime=regime)
    d["logits"] = make_logits(regime, B, C, rng)
    d["labels"] = soft_labels(labels, B, C, rng)
    d["mask"] = graph_mask(mask, B)
    return d


def softmax_cases(B):
    for C in SOFTMAX_CLASSES:
        for lab in SOFTMAX_LABELS:
            for mk in GRAPH_MASKS:
                for regime in SOFTMAX_REGIMES:
                    if regime == "spread" and C < 2:
                        continue                  # one class has no spread
                    yield softmax_case(B, C, lab, mk, regime)


def sparse_case(B, C, mask, regime):
    rng = _rng("sparse", B, C, mask, regime)
    d = dict(B=B, C=C, mask_kind=mask, regime=regime)
    d["logits"] = make_logits(regime, B, C, rng)
    idx = rng.integers(0, C, B).astype(np.int64)
    idx[0] = 0                                    # the first and the last class are both asked for
    idx[-1] = C - 1
    d["idx"] = idx
    d["mask"] = None if mask == "none" else graph_mask(mask, B)
    return d


def sparse_cases(B):
    for C in SOFTMAX_CLASSES:
        for mk in SPARSE_MASKS:
            for regime in SOFTMAX_REGIMES:
                if regime == "spread" and C < 2:
                    continue
                yield sparse_case(B, C, mk, regime)


# ---- autograd through the ops wrappers: B = 257 (two workgroups, the finishing launch), both upstream gradients ----------------
AUTOGRAD_B = 257
AUTOGRAD_UPSTREAM = ((1.0, 0.0), (0.0, 1.0), (0.7, -1.3))            # (a, b) of a cost_opt + b cost_sum


def autograd_sigmoid_case(regime):
    return sigmoid_case(AUTOGRAD_B, 5, "per_task", "p80", "tail", regime)


def autograd_softmax_case(regime):
    return softmax_case(AUTOGRAD_B, 5, "soft_scaled", "tail", regime)


def autograd_sparse_case(regime):
    return sparse_case(AUTOGRAD_B, 5, "none", regime)


# ---- TF-Adam ----------------------------------------------------------------------------------------------------------------
ADAM_PACKED_THREADS = 256 * 8 * 256                # the packed kernels' grid cap: more elements (float4s) than this take a second trip
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, ADAM_PACKED_THREADS + 257, 4 * ADAM_PACKED_THREADS + 1028)
ADAM_COUNTERS = (0, 1, 999, 100_000)
ADAM_STEPS = 3
ADAM_HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)
ADAM_SEGMENT_COUNTS = (1, 3, 33)


def adam_case(n, counter):
    """Parameters N(0, 1); one gradient per step: a fifth exact zeros, the rest of either sign with magnitudes 10^U(-12, 4), so g^2
    stays a normal float32 and the fp64 reference is the right answer.  counter 0: zero moments.  A restored run (counter > 0):
    m ~ 0.01 N(0, 1), v = the square of such a value, and both zero on the half of the elements that never saw a gradient.
    Element 0 always starts from zero moments with a first gradient of 1e-6: sqrt(v) = 3e-8 is then next to epsilon = 1e-8, where
    an epsilon under the root instead of outside it moves the parameter by 0.001 lr_t instead of 2.4 lr_t, whatever n is
    (tests/test_step_tail_oracle.py shows it)."""
    rng = _rng("adam", n, counter)
    d = dict(n=n, counter=counter)
    d["p"] = rng.standard_normal(n).astype(np.float32)
    grads = []
    for _ in range(ADAM_STEPS):
        g = np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-12, 4, n)
        g[rng.random(n) < 0.2] = 0
        grads.append(g.astype(np.float32))
    grads[0][0] = 1e-6
    d["grads"] = grads
    if counter == 0:
        d["m"], d["v"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        live = rng.random(n) < 0.5
        live[0] = False
        d["m"] = (0.01 * rng.standard_normal(n) * live).astype(np.float32)
        d["v"] = ((0.01 * rng.standard_normal(n)) ** 2 * live).astype(np.float32)
    return d


def adam_segments(n, k):
    """n floats cut into k consecutive segments of uneven lengths -> [(offset, length)]; from k = 3 on, one of them is empty."""
    rng = _rng("segments", n, k)
    cuts = sorted(int(c) for c in rng.integers(0, n + 1, k - 1))
    if k >= 3:
        cuts[1] = cuts[0]
    edges = [0] + cuts + [n]
    return [(edges[i], edges[i + 1] - edges[i]) for i in range(k)]
