"""fp64 reference of the cross-layer stack (csrc/stack.hip, csrc/stack_tile.hip): a LIST of layers

    kind 0  H <- act(A (H W + b))                                  GraphConv, one channel
    kind 1  H <- act(H W + b)                                      GraphDense
    kind 2  H <- act(gamma (H - mean) / sqrt(var + eps) + beta)    GraphBatchNormalization with its moving statistics on the
                 rows < sizes[t]; act(0) on the others, which pass no gradient into the layer

followed by GraphGather (the sum over ALL N rows) or by nothing (per-node output), in plain numpy on the layer functions of
oracle/kgcn_oracle.py.  Forward, and for a given cotangent of the final output the gradient of the input and the parameter
gradients in the flat order of the ABI (dW | db per matrix layer, dgamma | dbeta per normalisation).

Activation derivatives are expressed in the layer OUTPUT a, as include/kgcn_hip.h states them: sigmoid a (1 - a), relu a > 0
(0 at exactly 0, as TF), tanh 1 - a^2.
"""
import numpy as np

from oracle import kgcn_oracle as K

ACT_NONE, ACT_SIGMOID, ACT_RELU, ACT_TANH = 0, 1, 2, 3       # KGCN_ACT_* of include/kgcn_hip.h
CONV, DENSE, NORM = 0, 1, 2                                  # kgcn_stack_layer.kind


def act_fwd(v, act):
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    if act == ACT_RELU:
        return np.where(v > 0, v, np.zeros_like(v))
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def act_dout(a, act):
    if act == ACT_SIGMOID:
        return a * (1.0 - a)
    if act == ACT_RELU:
        return (a > 0).astype(a.dtype)
    if act == ACT_TANH:
        return 1.0 - a * a
    return np.ones_like(a)


def stack_forward(spec, params, buffers, x, adjs, sizes=None, gather=True, dtype=np.float64):
    """spec: (kind, act_code, din, dout, eps) per layer, as ops.gcn_stack takes it; params: flat, two arrays (or None for a
    bias) per layer (w, b | gamma, beta); buffers: per layer (moving mean, moving variance) or None; x [T, N, d0]; adjs[t] =
    [(idx, val, shape)]; sizes [T] or None (every row valid).  -> (pre, outs, out): every layer's pre-activation and output
    [T, N, dout] and the final output (gather: [T, d_last], else outs[-1])."""
    h = np.asarray(x, dtype)
    pre, outs = [], []
    for l, (kind, act, din, dout, eps) in enumerate(spec):
        w, b = params[2 * l], params[2 * l + 1]
        assert h.shape[2] == din, (l, h.shape, din)
        if kind == NORM:
            mean, var = buffers[l]
            z = K.graph_bn_fwd(h, w, b, mean, var, enabled_node_nums=sizes, eps=eps, training=False, dtype=dtype)[0]
        else:
            w = np.asarray(w, dtype).reshape(din, dout)
            b = np.zeros(dout, dtype) if b is None else np.asarray(b, dtype).reshape(dout)
            z = K.graphconv_fwd_fast(h, adjs, [w], [b], dtype=dtype) if kind == CONV else K.graphdense_fwd(h, w, b, dtype=dtype)
        h = act_fwd(z, act)
        pre.append(z)
        outs.append(h)
    return pre, outs, (K.gather_fwd(h, dtype=dtype) if gather else h)


def stack_reference(spec, params, buffers, x, adjs, sizes=None, gather=True, cotangent=None, dtype=np.float64):
    """-> dict: pre, outs, out as stack_forward; with a cotangent of `out` also dx [T, N, d0], grads (one array or None per
    entry of params, in its shape) and dparams (the flat layout of the ABI; a missing bias still takes its dout floats)."""
    x = np.asarray(x, dtype)
    pre, outs, out = stack_forward(spec, params, buffers, x, adjs, sizes, gather, dtype)
    res = {"pre": pre, "outs": outs, "out": out}
    if cotangent is None:
        return res
    N = x.shape[1]
    g = np.asarray(cotangent, dtype)
    assert g.shape == out.shape, (g.shape, out.shape)
    if gather:
        g = K.gather_bwd(g, N, dtype=dtype)
    grads, flat = [None] * len(params), [None] * len(spec)
    for l in range(len(spec) - 1, -1, -1):
        kind, act, din, dout, eps = spec[l]
        hin = x if l == 0 else outs[l - 1]
        dpre = g * act_dout(outs[l], act)
        w, b = params[2 * l], params[2 * l + 1]
        if kind == NORM:
            mean, var = buffers[l]
            # (graph_bn_bwd masks the rows >= sizes[t]: their act(0) passes nothing into the layer)
            g, dgamma, dbeta = K.graph_bn_bwd(hin, w, mean, var, dpre, enabled_node_nums=sizes, eps=eps, training=False, dtype=dtype)
            grads[2 * l], grads[2 * l + 1] = dgamma.reshape(np.shape(w)), dbeta.reshape(np.shape(b))
            flat[l] = np.concatenate([dgamma.ravel(), dbeta.ravel()])
            continue
        wm = np.asarray(w, dtype).reshape(din, dout)
        if kind == CONV:
            g, dw, db = K.graphconv_bwd_fast(hin, adjs, [wm], dpre, dtype=dtype)
            dw, db = dw[0], db[0].ravel()
        else:
            g, dw, db = K.graphdense_bwd(hin, wm, dpre, dtype=dtype)
        grads[2 * l] = dw.reshape(np.shape(w))
        grads[2 * l + 1] = None if b is None else db.reshape(np.shape(b))
        flat[l] = np.concatenate([dw.ravel(), db.ravel()])
    res.update(dx=g, grads=grads, dparams=np.concatenate(flat))
    return res
