"""Plain numpy fp64 reference of the tail of a training step, operation by operation: the loss heads of kgcn_amd/csrc/train.hip
(masked sigmoid cross entropy, masked softmax cross entropy with dense or sparse labels, the backward of both) and the TF-Adam
update.  TEST INFRASTRUCTURE ONLY.  tests/test_step_tail_oracle.py checks it against oracle/kgcn_model_oracle.py and
oracle/kgcn_nets_oracle.py and against central differences; tests/test_gpu_loss_heads.py and tests/test_gpu_adam_forms.py
compare the kernels with it.

Every loss returns (cost [B], dlogits [B, W] = d cost_sum / d logits, cost_sum, cost_opt); cost_opt is the mean over the PADDED
batch (reduce_mean over all B rows, masked or not -- quirk Q5), never over the unmasked count.  Inputs are widened to fp64 as
they are: a float32 label row that sums to 0.99999994 is used with that sum.
"""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sigmoid(x):
    """1 / (1 + exp(-x)) without overflow and without cancellation at either end."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _finish(cost, dlogits):
    s = float(cost.sum())
    return cost, dlogits, s, s / cost.shape[0]


def sigmoid_ce(logits, labels, mask, mask_label=None, pos_weight=None):
    """example_model/model_multitask.py:66-79: cost[b] = mask[b] sum_t mask_label[b, t] ce(x[b, t], z[b, t]) with
         ce  = max(x, 0) - x z + log(1 + exp(-|x|))                             (pos_weight None)
         wce = (1 - z) x + (1 + (q - 1) z) (log(1 + exp(-|x|)) + max(-x, 0))    (pos_weight q: a scalar, or q[t] per TASK)."""
    x, z, mk = _f64(logits), _f64(labels), _f64(mask).reshape(-1)
    ml = np.ones_like(x) if mask_label is None else _f64(mask_label)
    sp = np.log1p(np.exp(-np.abs(x)))
    if pos_weight is None:
        ce = np.maximum(x, 0.0) - x * z + sp
        dce = _sigmoid(x) - z
    else:
        q = _f64(pos_weight)
        q = q.reshape(1, -1) if q.ndim else q                   # per task = per COLUMN of the logits
        lw = 1.0 + (q - 1.0) * z
        ce = (1.0 - z) * x + lw * (sp + np.maximum(-x, 0.0))
        dce = (1.0 - z) - lw * _sigmoid(-x)                     # 1 - sigmoid(x) = sigmoid(-x)
    return _finish(mk * (ml * ce).sum(axis=1), mk[:, None] * ml * dce)


def softmax_ce(logits, labels, mask):
    """example_model/model.py:56-61: cost[b] = mask[b] * -(sum_c z[b, c] log_softmax(x[b])[c]); the labels may be soft and need
    not sum to 1: d cost / d x = mask (softmax(x) sum_c z - z)."""
    x, z, mk = _f64(logits), _f64(labels), _f64(mask).reshape(-1)
    s = x - x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(s).sum(axis=1, keepdims=True))
    logp = s - lse
    cost = mk * -(z * logp).sum(axis=1)
    return _finish(cost, mk[:, None] * (np.exp(logp) * z.sum(axis=1, keepdims=True) - z))


def sparse_softmax_ce(logits, idx, mask=None):
    """tf.nn.sparse_softmax_cross_entropy_with_logits (example_model/sparse.py:112): the label of row b is the class idx[b]."""
    x = _f64(logits)
    z = np.zeros_like(x)
    z[np.arange(x.shape[0]), np.asarray(idx, dtype=np.int64)] = 1.0
    return softmax_ce(x, z, np.ones(x.shape[0]) if mask is None else mask)


def loss_grad(dlogits, g_opt, g_sum, batch):
    """Backward of a head: d (g_opt cost_opt + g_sum cost_sum) / d logits = dlogits (g_sum + g_opt / batch); None = no such
    upstream gradient."""
    return _f64(dlogits) * ((0.0 if g_sum is None else float(g_sum)) + (0.0 if g_opt is None else float(g_opt)) / batch)


def adam_hyper(lr, b1, b2, eps):
    """The hyper-parameters as the kernels see them: each rounded to float32 (they cross the C ABI as floats) and widened, and
    1 - beta formed IN float32 (c1 = 1.0f - b1) before widening -> (lr, b1, b2, eps, c1, c2) as Python floats."""
    lr, b1, b2, eps = np.float32(lr), np.float32(b1), np.float32(b2), np.float32(eps)
    c1, c2 = np.float32(1.0) - b1, np.float32(1.0) - b2
    return tuple(float(a) for a in (lr, b1, b2, eps, c1, c2))


def adam_lr_t(t, lr, b1, b2):
    """lr sqrt(1 - b2^t) / (1 - b1^t) with the float32-rounded lr, b1, b2; t counts from 1."""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    return lr * np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))


def tf_adam(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """One tf.train.AdamOptimizer update (kgcn/core.py:124), t = the number of this step (the counter before it, plus one):
         m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr_t m / (sqrt(v) + eps)       -- epsilon OUTSIDE the root
    -> (p, m, v), new arrays."""
    lr_, b1_, b2_, eps_, c1, c2 = adam_hyper(lr, b1, b2, eps)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    m = b1_ * m + c1 * g
    v = b2_ * v + c2 * (g * g)
    return p - adam_lr_t(t, lr, b1, b2) * m / (np.sqrt(v) + eps_), m, v
