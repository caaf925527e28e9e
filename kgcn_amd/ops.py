"""Functional ops of the hot path on torch (ROCm) tensors, each a torch.autograd.Function whose
forward and backward are calls into libkgcn_hip.so through the C ABI.  No arithmetic of the
path is done by torch here: torch provides device memory, the stream and the autograd tape.

Gradients follow the reference's registered gradients:
  Bspmm  kgcn/bspmm_call.py:22-57   d rhs = A^T g ; d values[e] = <g[row_e], rhs[col_e]>
  Bconv  kgcn/bconv_call.py:30-70   the output gradient fans out to every channel
  Bspmdt kgcn/batched_call.py:33-75 d rhs is the stacked [T*K, D] tensor
and TF's MatMul / BiasAdd gradients for the dense part.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr, require_gpu
from .batched_csr import BatchedAdjacency, BatchedCSR


# Every limit and code below is read from include/kgcn_hip.h (_lib.K: its constants by name); none is restated here.
ACT_CODES = {None: _lib.K["KGCN_ACT_NONE"], "none": _lib.K["KGCN_ACT_NONE"], "linear": _lib.K["KGCN_ACT_NONE"],
             "sigmoid": _lib.K["KGCN_ACT_SIGMOID"], "relu": _lib.K["KGCN_ACT_RELU"], "tanh": _lib.K["KGCN_ACT_TANH"]}
# A/B switch: d pre-activation inside the wide weight-gradient GEMM when the layer input needs no gradient
wgrad_dact_fusion = True
# OPTION (off): weight gradients of the big dense layers on a SIDE HIP stream.  In a backward pass dW / dbias hang off the
# critical chain (d pre-activation -> d inputs -> adjoint aggregation -> the layer below); the chain's aggregation kernels are
# bound by HBM, the weight-gradient GEMMs by the matrix pipe, so overlapping them looked free.  Measured (tools/gpu_round3_i.sh,
# same box, two rounds): cfg4 1.756 / 1.773 ms with the side stream vs 1.747 / 1.751 without, cfg5 3.03 / 3.04 vs 2.98 / 2.99 --
# the step runs at the package power limit (DESIGN.md lesson 4c), so concurrency buys nothing and costs the fork / join.
# The mechanism stays for experiments: the side stream forks from the calling stream when d pre-activation is ready and is
# joined by an autograd end-of-backward callback (inside a hipGraph capture fork and join become graph edges).
side_stream_wgrad = False
side_wgrad_min_rows = 16384
_side_streams = {}
_side_pending = set()


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


# ---- deferred second stages of the parameter gradients (kgcn_reduce_defer / kgcn_reduce_flush, include/kgcn_hip.h) -----------
_deferred_keep = []            # workspaces whose partials are still queued


class deferred_reductions:
    """with ops.deferred_reductions(root=loss): loss.backward()  -- the weight-gradient calls inside queue their second stages;
    leaving the block adds all of them in ONE launch.  Parameter gradients are valid only after the block (kgcn_amd.train uses
    it around the backward pass of a training step; plain autograd code never sees deferral).

    A gradient may only wait when NOTHING reads it inside the backward pass.  `root` (the tensor(s) backward() is about to be
    called on) lets the block check that on the autograd graph itself: a parameter whose AccumulateGrad node has more than one
    incoming edge (used twice -- by kgcn ops, by plain torch ops such as an L2 penalty or a tied torch.matmul, or both: autograd
    ADDS the contributions inside the pass), that carries a tensor hook, or whose .grad already exists (accumulated in place
    inside the pass) is excluded from deferral for this backward pass.  Without `root` only uses by kgcn ops are known
    (_record_params): pass it whenever the model may contain anything else."""

    def __init__(self, root=None):
        self.root = root

    def __enter__(self):
        _no_defer_params.clear()
        if self.root is not None:
            _no_defer_params.update(_readers_inside_backward(self.root))
        self.prev = lib.kgcn_reduce_defer(1)
        return self

    def __exit__(self, *exc):
        try:
            flush_reductions()
        finally:
            lib.kgcn_reduce_defer(self.prev)
            _no_defer_params.clear()
        return False


_no_defer_params = set()       # id() of parameters whose gradient is read inside the backward pass now running


def _readers_inside_backward(root):
    """id()s of the leaf tensors under `root` whose gradient contribution from a deferring op could be READ before the flush:
    AccumulateGrad nodes with several incoming edges, tensor hooks, an existing .grad."""
    roots = root if isinstance(root, (list, tuple)) else (root,)
    edges, seen, stack = {}, set(), [t.grad_fn for t in roots if t is not None and t.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn in seen:
            continue
        seen.add(fn)
        for nxt, _ in fn.next_functions:
            if nxt is None:
                continue
            if hasattr(nxt, "variable"):                 # AccumulateGrad
                edges[nxt] = edges.get(nxt, 0) + 1
            elif nxt not in seen:
                stack.append(nxt)
    out = set()
    for acc, n in edges.items():
        v = acc.variable
        if n > 1 or v.grad is not None or getattr(v, "_backward_hooks", None) or getattr(v, "_post_accumulate_grad_hooks", None):
            out.add(id(v))
    return out


def flush_reductions():
    check(lib.kgcn_reduce_flush(current_stream()), "kgcn_reduce_flush")
    _deferred_keep.clear()


# How often each parameter tensor entered a deferral-capable op since the step began: a parameter used TWICE receives two
# gradient contributions that autograd adds INSIDE the backward pass -- before the flush -- so only single-use parameters may wait
# (model_multitask.py's ragged execution runs dense2 on the valid rows and once more on the padding representative).
_param_uses = {}


def _record_params(ctx, *params, when=True):
    """Forward half of every op whose backward C call writes parameter gradients through the deferrable second stage: records
    those parameters (None entries skipped) and counts one use of each.  stack_rows' operand is a fresh tensor on every call and
    stands for the parameters behind it: those are counted and checked.  when=False: this call's backward never defers."""
    ps = []
    for p in params:
        if p is not None:
            ps.extend(getattr(p, "_kgcn_defer_params", (p,)))
    for p in ps:
        _param_uses[id(p)] = _param_uses.get(id(p), 0) + 1
    ctx.defer_params = tuple(ps) if when else ()


class _param_grad_stage:
    """with _param_grad_stage(ctx, nbytes, device) as ws: <the op's C call>  -- the backward half of _record_params; ws is the
    call's partials workspace (at least nbytes), kept alive until the flush.  Deferral stays on around the call only if nothing
    reads or drops the recorded parameters' gradients before the flush: each one is a leaf (a computed weight's gradient is read
    right away), requires a gradient (autograd drops an unwanted one when backward returns, and the flush would then write into
    reused memory), is used once this step and not read inside the pass (deferred_reductions' root check); grad mode is off
    (backward(create_graph=True) turns it on, and AccumulateGrad then copies each gradient before the flush); `when` holds."""

    __slots__ = ("ok", "ws", "prev")

    def __init__(self, ctx, nbytes, device, when=True):
        self.ws = _lib.workspace(nbytes, device)
        ps = ctx.defer_params
        self.ok = bool(when and ps and not torch.is_grad_enabled() and all(
            p.is_leaf and p.requires_grad and _param_uses.get(id(p), 0) == 1 and id(p) not in _no_defer_params for p in ps))

    def __enter__(self):
        self.prev = None if self.ok else lib.kgcn_reduce_defer(0)
        return self.ws

    def __exit__(self, *exc):
        if self.prev is not None:
            lib.kgcn_reduce_defer(self.prev)
        if lib.kgcn_reduce_pending() > 0:
            _deferred_keep.append(self.ws)
        return False


def join_side_streams():
    """Make the current stream wait for every weight gradient still running on a side stream."""
    for key in list(_side_pending):
        torch.cuda.current_stream(torch.device(*key)).wait_stream(_side_streams[key])
    _side_pending.clear()


def _fork_side(device):
    """-> the side stream, forked from the current one; the join is queued for the end of this backward pass."""
    side = _side_stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    key = (device.type, device.index)
    if key not in _side_pending:
        _side_pending.add(key)
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)
        except RuntimeError:                     # not inside a backward pass (a direct call of .backward of the Function)
            pass
    return side


def act_code(activation):
    """KGCN_ACT_* code of an activation given by name (the ones the reference's models use: tf.sigmoid, tf.nn.relu,
    tf.tanh) or None."""
    try:
        return ACT_CODES[activation]
    except KeyError:
        raise ValueError("unsupported activation %r (None, 'sigmoid', 'relu', 'tanh')" % (activation,)) from None


def _f32c(t, name):
    require_gpu(t, name)
    if t.dtype != torch.float32:
        raise _lib.KgcnHipError("%s must be float32 (the path computes in fp32), got %s" % (name, t.dtype))
    return t.contiguous()


# -------------------------------------------------------------------------------------------------
# raw (non-differentiable) launches
# -------------------------------------------------------------------------------------------------
def bspmm_raw(csr, rhs2d, d, out2d, rhs_ld=None, rhs_gs=None, out_ld=None, out_gs=None, beta=0.0,
              rhs_col=0, out_col=0):
    """out[t] = beta*out[t] + A[t] @ rhs[t] on strided views of 2-D tensors.
    rhs2d: [T*K, rhs_ld] (block t starts at row t*K), columns rhs_col .. rhs_col+d."""
    rhs_ld = rhs2d.stride(0) if rhs_ld is None else rhs_ld
    out_ld = out2d.stride(0) if out_ld is None else out_ld
    rhs_gs = csr.cols * rhs_ld if rhs_gs is None else rhs_gs
    out_gs = csr.rows * out_ld if out_gs is None else out_gs
    check(lib.kgcn_bspmm_f32(csr.desc(), rhs2d.data_ptr() + 4 * rhs_col, rhs_ld, rhs_gs, d,
                             out2d.data_ptr() + 4 * out_col, out_ld, out_gs, float(beta),
                             current_stream()), "kgcn_bspmm_f32")
    return out2d


# -------------------------------------------------------------------------------------------------
# Bspmm / Bspmdt
# -------------------------------------------------------------------------------------------------
class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rhs, values, csr):
        # rhs: [T*K, D] contiguous.  values: None or differentiable [nnz] (CSR order)
        rhs = _f32c(rhs, "rhs")
        if values is not None:
            csr = csr.with_values(_f32c(values, "values"))
        T, M, K = csr.num_graphs, csr.rows, csr.cols
        if rhs.dim() != 2 or rhs.shape[0] != T * K:
            raise _lib.KgcnHipError("rhs must be [T*K, D] = [%d, D], got %s" % (T * K, tuple(rhs.shape)))
        d = rhs.shape[1]
        out = torch.empty((T * M, d), device=rhs.device, dtype=torch.float32)
        bspmm_raw(csr, rhs, d, out)
        ctx.csr = csr
        ctx.has_values = values is not None
        ctx.save_for_backward(rhs)
        return out

    @staticmethod
    def backward(ctx, g):
        (rhs,) = ctx.saved_tensors
        csr = ctx.csr
        g = _f32c(g, "grad")
        d = rhs.shape[1]
        d_rhs = d_val = None
        if ctx.needs_input_grad[0]:
            d_rhs = torch.empty_like(rhs)
            bspmm_raw(csr.transpose(), g, d, d_rhs)
        if ctx.has_values and ctx.needs_input_grad[1]:
            d_val = torch.empty((csr.nnz,), device=rhs.device, dtype=torch.float32)
            check(lib.kgcn_spmm_values_grad_f32(csr.desc(), ptr(g), d, csr.rows * d, ptr(rhs), d,
                                                csr.cols * d, d, ptr(d_val), current_stream()),
                  "kgcn_spmm_values_grad_f32")
        return d_rhs, d_val, None


def bspmm(csr, rhs, values=None):
    """Batched SpMM.  rhs [T, K, D] or [T*K, D] -> same rank ([T, M, D] or [T*M, D])."""
    if rhs.dim() == 3:
        T, K, D = rhs.shape
        return _SpMM.apply(rhs.reshape(T * K, D), values, csr).reshape(T, csr.rows, D)
    return _SpMM.apply(rhs, values, csr)


# -------------------------------------------------------------------------------------------------
# [W_0 | W_1 | ...] and [b_0 | b_1 | ...] of a multi-channel GraphConv: ONE launch (kgcn_copy2d_multi_f32) instead of two torch.cat,
# and in the backward ONE launch that splits the operand's gradient into a fresh contiguous tensor per parameter (the narrowed
# views a cat's backward returns are cloned by AccumulateGrad: 2 C more launches per step)
# -------------------------------------------------------------------------------------------------
def _copy2d(jobs):
    import ctypes
    arr = (_lib.Copy2dJob * len(jobs))(*[_lib.Copy2dJob(*j) for j in jobs])
    check(lib.kgcn_copy2d_multi_f32(ctypes.cast(arr, ctypes.c_void_p), len(jobs), current_stream()), "kgcn_copy2d_multi_f32")


class _CatChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *tensors):
        C = len(tensors) // 2
        ws = [_f32c(t, "kernel") for t in tensors[:C]]
        bs = [_f32c(t, "bias") for t in tensors[C:]]
        din, dout = ws[0].shape
        if any(tuple(w.shape) != (din, dout) for w in ws) or any(b.numel() != dout for b in bs):
            raise _lib.KgcnHipError("cat_channels: the kernels / biases of the channels differ in shape")
        wcat = torch.empty((din, C * dout), device=ws[0].device, dtype=torch.float32)
        bcat = torch.empty((1, C * dout), device=ws[0].device, dtype=torch.float32)
        jobs = [(w.data_ptr(), wcat.data_ptr() + 4 * c * dout, din, dout, dout, C * dout) for c, w in enumerate(ws)]
        jobs += [(b.data_ptr(), bcat.data_ptr() + 4 * c * dout, 1, dout, dout, C * dout) for c, b in enumerate(bs)]
        _copy2d(jobs)
        ctx.shapes = [tuple(t.shape) for t in tensors]
        ctx.dims = (C, din, dout)
        return wcat, bcat

    @staticmethod
    def backward(ctx, gw, gb):
        C, din, dout = ctx.dims
        gw, gb = _f32c(gw, "grad"), _f32c(gb, "grad")
        dws = [torch.empty(ctx.shapes[c], device=gw.device, dtype=torch.float32) for c in range(C)]
        dbs = [torch.empty(ctx.shapes[C + c], device=gw.device, dtype=torch.float32) for c in range(C)]
        jobs = [(gw.data_ptr() + 4 * c * dout, dws[c].data_ptr(), din, dout, C * dout, dout) for c in range(C)]
        jobs += [(gb.data_ptr() + 4 * c * dout, dbs[c].data_ptr(), 1, dout, C * dout, dout) for c in range(C)]
        _copy2d(jobs)
        return tuple(dws) + tuple(dbs)


class _StackChannelRows(torch.autograd.Function):
    """[W_0; b_0; 0; W_1; b_1; 0; ...]  [C dp, dout]: the operand of an aggregate-first multi-channel GraphConv
    ([A_0 X' | A_1 X' | ...] [W_0; b_0; 0; ...], X' = [X | 1 | 0]) in one launch; `pad` = the constant zero rows."""

    @staticmethod
    def forward(ctx, pad, *tensors):
        C = len(tensors) // 2
        ws = [_f32c(t, "kernel") for t in tensors[:C]]
        bs = [_f32c(t, "bias") for t in tensors[C:]]
        din, dout = ws[0].shape
        npad = pad.shape[0]
        dp = din + 1 + npad
        wa = torch.empty((C * dp, dout), device=ws[0].device, dtype=torch.float32)
        jobs = []
        for c in range(C):
            base = wa.data_ptr() + 4 * c * dp * dout
            jobs.append((ws[c].data_ptr(), base, din, dout, dout, dout))
            jobs.append((bs[c].data_ptr(), base + 4 * din * dout, 1, dout, dout, dout))
            if npad:
                jobs.append((pad.data_ptr(), base + 4 * (din + 1) * dout, npad, dout, dout, dout))
        _copy2d(jobs)
        ctx.shapes = [tuple(t.shape) for t in tensors]
        ctx.dims = (C, din, dout, dp)
        return wa

    @staticmethod
    def backward(ctx, gwa):
        C, din, dout, dp = ctx.dims
        gwa = _f32c(gwa, "grad")
        dws = [torch.empty(ctx.shapes[c], device=gwa.device, dtype=torch.float32) for c in range(C)]
        dbs = [torch.empty(ctx.shapes[C + c], device=gwa.device, dtype=torch.float32) for c in range(C)]
        jobs = []
        for c in range(C):
            base = gwa.data_ptr() + 4 * c * dp * dout
            jobs.append((base, dws[c].data_ptr(), din, dout, dout, dout))
            jobs.append((base + 4 * din * dout, dbs[c].data_ptr(), 1, dout, dout, dout))
        _copy2d(jobs)
        return (None,) + tuple(dws) + tuple(dbs)


def stack_channel_rows(ws, bs, pad):
    return _StackChannelRows.apply(pad, *(list(ws) + list(bs)))


class _FanOut(torch.autograd.Function):
    """z[:, c d : (c + 1) d] = A_c @ x for every channel c: ONE launch that reads x once (kgcn_bconv_fanout_f32 on the channels'
    own containers); backward d x = sum_c A_c^T gz_c: the multi-channel aggregation over the transposed containers."""

    @staticmethod
    def forward(ctx, x, adj):
        x = _f32c(x, "inputs")
        C = adj.num_channels
        T, M, K = adj.num_graphs, adj.n_nodes, adj.channels[0].cols
        d = x.shape[1]
        if x.shape[0] != T * K:
            raise _lib.KgcnHipError("inputs must be [T*K, d] = [%d, d], got %s" % (T * K, tuple(x.shape)))
        z = torch.empty((T * M, C * d), device=x.device, dtype=torch.float32)
        check(lib.kgcn_bconv_fanout_f32(adj.desc_array(False), C, ptr(x), None, d, K * d, d, 0, ptr(z), C * d, M * C * d, d,
                                        current_stream()), "kgcn_bconv_fanout_f32")
        ctx.adj, ctx.d = adj, d
        return z

    @staticmethod
    def backward(ctx, gz):
        adj, d = ctx.adj, ctx.d
        if not ctx.needs_input_grad[0]:
            return None, None
        gz = _f32c(gz, "grad")
        C = adj.num_channels
        T, M, K = adj.num_graphs, adj.n_nodes, adj.channels[0].cols
        dx = torch.empty((T * K, d), device=gz.device, dtype=torch.float32)
        check(lib.kgcn_bconv_act_f32(adj.desc_array(True), C, ptr(gz), C * d, M * C * d, d, d, ptr(dx), d, K * d, 0, current_stream()),
              "kgcn_bconv_act_f32")
        return dx, None


def fan_out(adj, x2d):
    """[A_0 x | A_1 x | ...]  [T*M, C d]"""
    return _FanOut.apply(x2d, adj)


def cat_channels(ws, bs):
    """-> ([W_0 | W_1 | ...] [din, C dout], [b_0 | b_1 | ...] [1, C dout]) as differentiable functions of the 2 C parameters."""
    return _CatChannels.apply(*(list(ws) + list(bs)))


# -------------------------------------------------------------------------------------------------
# Bconv: out[t] = sum_c A_c[t] @ rhs_c[t], rhs given as ONE [T*K, C*D] tensor (channel c = columns
# c*D..(c+1)*D) -- exactly what one GEMM with the concatenated kernels produces.
# -------------------------------------------------------------------------------------------------
class _BConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rhs, adj, d, act, *values):
        # values: nothing, or one tensor per channel -- the channel's adjacency values as differentiable inputs
        # (fp32 [nnz_c], CSR order), None for a channel whose stored values are used
        # act: KGCN_ACT_* code applied to the aggregated output inside the kernel (its derivative, expressed in the
        # output, rides in the adjoint aggregation of the backward)
        rhs = _f32c(rhs, "rhs")
        C = adj.num_channels
        T, M, K = adj.num_graphs, adj.n_nodes, adj.channels[0].cols
        if rhs.shape != (T * K, C * d):
            raise _lib.KgcnHipError("rhs must be [T*K, C*D] = [%d, %d], got %s" % (T * K, C * d, tuple(rhs.shape)))
        if values:
            if len(values) != C:
                raise _lib.KgcnHipError("one value tensor (or None) per adjacency channel is required")
            adj = BatchedAdjacency([ch if v is None else ch.with_values(_f32c(v, "values"))
                                    for ch, v in zip(adj.channels, values)])
        out = torch.empty((T * M, d), device=rhs.device, dtype=torch.float32)
        check(lib.kgcn_bconv_act_f32(adj.desc_array(False), C, ptr(rhs), C * d, K * C * d, d, d,
                                     ptr(out), d, M * d, int(act), current_stream()), "kgcn_bconv_act_f32")
        ctx.adj, ctx.d, ctx.act = adj, d, int(act)
        ctx.nvalues = len(values)
        # rhs (the [T*K, C*D] GEMM output) is only read by the d values gradient; without differentiable adjacency values
        # it is NOT retained (one activation-sized tensor per GraphConv layer until backward otherwise)
        ctx.keeps_rhs = bool(values) and any(ctx.needs_input_grad[4:])
        ctx.save_for_backward(*(([rhs] if ctx.keeps_rhs else []) + ([out] if act else [])))
        return out

    @staticmethod
    def backward(ctx, g):
        adj, d, act = ctx.adj, ctx.d, ctx.act
        saved = list(ctx.saved_tensors)
        rhs = saved.pop(0) if ctx.keeps_rhs else None
        aout = saved.pop(0) if act else None
        g = _f32c(g, "grad")
        C = adj.num_channels
        T, M, K = adj.num_graphs, adj.n_nodes, adj.channels[0].cols
        d_rhs = None
        if ctx.needs_input_grad[0]:
            d_rhs = torch.empty((T * K, C * d), device=g.device, dtype=torch.float32)
            # addn_grad: g fans out to every channel -- ONE launch reads it once and writes every channel's column block
            # (d pre-activation = g * act'(out) is formed while the block is staged)
            check(lib.kgcn_bconv_fanout_f32(adj.desc_array(True), C, ptr(g), ptr(aout) if act else None, d, M * d, d, int(act),
                                            ptr(d_rhs), C * d, K * C * d, d, current_stream()), "kgcn_bconv_fanout_f32")
        if act and ctx.nvalues and any(ctx.needs_input_grad[4:]):
            g = activation_backward(aout, g, act)        # d values needs d pre-activation as a tensor
        d_vals = []
        for c in range(ctx.nvalues):
            # kgcn/bconv_call.py:55-67: d values[t][e] = <addn_grad[t][row_e], b[t][col_e]> per graph-channel -- one
            # gather-multiply-reduce launch per channel over the whole batch, the channel's columns of rhs as b
            if not ctx.needs_input_grad[4 + c]:
                d_vals.append(None)
                continue
            ch = adj.channels[c]
            dv = torch.empty((ch.nnz,), device=g.device, dtype=torch.float32)
            check(lib.kgcn_spmm_values_grad_f32(ch.desc(), ptr(g), d, M * d, rhs.data_ptr() + 4 * c * d, C * d,
                                                K * C * d, d, ptr(dv), current_stream()),
                  "kgcn_spmm_values_grad_f32(bconv)")
            d_vals.append(dv)
        return (d_rhs, None, None, None) + tuple(d_vals)


def bconv(adj, rhs_cat, d, values=None, activation=None):
    """values: optional list with one differentiable fp32 [nnz_c] tensor (CSR order) or None per channel.
    activation: None / 'sigmoid' / 'relu' / 'tanh' applied to the aggregated output inside the kernel."""
    act = act_code(activation)
    if values is None:
        return _BConv.apply(rhs_cat, adj, d, act)
    return _BConv.apply(rhs_cat, adj, d, act, *values)


# -------------------------------------------------------------------------------------------------
# stand-alone activation (where no producer kernel can carry it) and the backward of every fused activation
# -------------------------------------------------------------------------------------------------
def activation_backward(act_out, grad, act):
    """grad * act'(.) with the derivative expressed in the activation OUTPUT; returns a new tensor."""
    act_out, grad = _f32c(act_out, "activation output"), _f32c(grad, "grad")
    dpre = torch.empty_like(grad)
    check(lib.kgcn_act_bwd_f32(ptr(act_out), ptr(grad), grad.numel(), int(act), ptr(dpre), current_stream()),
          "kgcn_act_bwd_f32")
    return dpre


class _Activation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        x = _f32c(x, "inputs")
        y = torch.empty_like(x)
        check(lib.kgcn_act_fwd_f32(ptr(x), x.numel(), int(act), ptr(y), current_stream()), "kgcn_act_fwd_f32")
        ctx.act = int(act)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return activation_backward(y, g, ctx.act), None


def activation(x, name):
    """tf.sigmoid / tf.nn.relu / tf.tanh as one HIP elementwise kernel (forward) and one (backward)."""
    act = act_code(name)
    return x if act == 0 else _Activation.apply(x, act)


# -------------------------------------------------------------------------------------------------
# dense contraction
# -------------------------------------------------------------------------------------------------
class WeightTables:
    """bf16 fragment tables of the weight operands of wide dense layers (csrc/wtable.hip), split ONCE per training step.

    dense() registers every weight it sees that has a table route (both orientations: W for the forward, W^T for d input).
    refresh() -- called at the start of a step by kgcn_amd.train (train_step / GraphedTrainStep) -- splits all registered
    operands with one launch and stamps them with the current epoch; invalidate() -- called by TFAdam.step, which rewrites the
    weights through raw pointers -- starts a new epoch.  A lookup returns a table only if it was refreshed in this epoch AND
    the weight's torch version counter is the one seen at the refresh (copy_ / load_state_dict bump it); otherwise dense()
    splits on its own as before.  Only weights a dense() call touched since the previous refresh are split again (a second live
    model costs nothing).  Inside a captured hipGraph the refresh is part of the graph, so every replay rebuilds the
    tables from the weights it is about to use.
    WHO MUST CALL invalidate(): anything that writes a registered weight WITHOUT bumping its version counter between refresh() and
    the forward pass of the same step -- writes through `.data` (p.data.copy_, dist.broadcast(p.data)), custom optimisers working on raw
    pointers.  kgcn_amd.train.TFAdam does; torch.optim optimisers and copy_ / load_state_dict on the parameter itself bump the
    counter.  A write that does neither makes dense() multiply with the tables of the OLD weights, with no error."""

    def __init__(self):
        self.epoch = 0
        self.entries = {}          # (data_ptr, shape) -> entry

    class _Entry:
        __slots__ = ("ref", "tables", "epoch", "version", "used", "ref2", "rows")

    def _entry(self, w, create):
        import weakref
        key = (w.data_ptr(), tuple(w.shape))
        e = self.entries.get(key)
        if e is not None and e.ref() is None:
            del self.entries[key]
            e = None
        if e is None and create and isinstance(w, torch.nn.Parameter):
            din, dout = w.shape
            sizes = [int(lib.kgcn_dense_fwd_workspace_bytes(din, dout)), int(lib.kgcn_dense_fwd_workspace_bytes(dout, din))]
            if max(sizes) <= 0:
                return None
            e = WeightTables._Entry()
            e.ref = weakref.ref(w)
            e.tables = [None if b <= 0 else _lib.workspace(b, w.device) for b in sizes]
            e.epoch, e.version, e.used = -1, -1, False
            self.entries[key] = e
        if e is not None:
            e.used = True
        return e

    def register(self, w):
        if enabled_weight_tables and w.dim() == 2 and w.is_cuda and w.is_contiguous():
            self._entry(w, True)

    def lookup(self, w, trans):
        """-> (table tensor, bytes) ready for (w, trans) or (None, 0)."""
        if not enabled_weight_tables:
            return None, 0
        e = self._entry(w, False)
        if e is None or e.epoch != self.epoch or e.tables[trans] is None:
            return None, 0
        p = e.ref()
        if p is None or p._version != e.version:
            return None, 0
        return e.tables[trans], e.tables[trans].numel() * 4

    # ---- stacked operands [w; bias; 0] of the aggregate-first GraphConv (layers.py): split straight from the two parameters by a
    # table job with an extra row -- no torch.cat per step, no table split of its own in front of the layer's GEMM
    def _stacked_key(self, w, bias, rows):
        return ("stacked", w.data_ptr(), bias.data_ptr(), int(rows), tuple(w.shape))

    def register_stacked(self, w, bias, rows):
        if not (enabled_weight_tables and isinstance(w, torch.nn.Parameter) and isinstance(bias, torch.nn.Parameter) and w.is_cuda and
                w.is_contiguous() and bias.is_contiguous() and bias.numel() == w.shape[1] and rows > w.shape[0]):
            return
        key = self._stacked_key(w, bias, rows)
        e = self.entries.get(key)
        if e is None or e.ref() is None or e.ref2() is None:
            import weakref
            b = int(lib.kgcn_dense_fwd_workspace_bytes(rows, w.shape[1]))
            if b <= 0:
                return
            e = WeightTables._Entry()
            e.ref, e.ref2 = weakref.ref(w), weakref.ref(bias)
            e.tables = [_lib.workspace(b, w.device), None]
            e.epoch, e.version, e.used, e.rows = -1, (-1, -1), False, int(rows)
            self.entries[key] = e
        e.used = True

    def lookup_stacked(self, w, bias, rows):
        """-> (table tensor, bytes) of [w; bias; 0] with `rows` rows, refreshed in this epoch for these parameter versions, or (None, 0)."""
        if not enabled_weight_tables:
            return None, 0
        e = self.entries.get(self._stacked_key(w, bias, rows))
        if e is None or e.epoch != self.epoch:
            return None, 0
        p, q = e.ref(), e.ref2()
        if p is None or q is None or (p._version, q._version) != e.version:
            return None, 0
        e.used = True
        return e.tables[0], e.tables[0].numel() * 4

    def invalidate(self):
        self.epoch += 1

    def refresh(self):
        import ctypes
        _param_uses.clear()                            # a training step begins here (kgcn_amd.train calls refresh() first)
        live, stacked = [], []
        for key, e in list(self.entries.items()):
            p = e.ref()
            if key[0] == "stacked":
                q = e.ref2()
                if p is None or q is None or p.data_ptr() != key[1] or q.data_ptr() != key[2]:
                    del self.entries[key]
                elif e.used:
                    e.used = False
                    stacked.append((p, q, e))
                continue
            if p is None or p.data_ptr() != key[0]:
                del self.entries[key]
                continue
            if not e.used:
                continue                          # no dense() call touched this weight since the last refresh (another model's)
            e.used = False
            live.append((p, e))
        if not (live or stacked) or not enabled_weight_tables:
            return
        jobs = (_lib.WtableJob * (2 * len(live) + len(stacked)))()
        n = 0
        for p, q, e in stacked:
            din, dout = p.shape
            jobs[n] = _lib.WtableJob(p.data_ptr(), dout, 0, e.rows, dout, din, e.tables[0].data_ptr(), q.data_ptr())
            n += 1
        for p, e in live:
            din, dout = p.shape
            for trans, (k, nn) in enumerate(((din, dout), (dout, din))):
                if e.tables[trans] is not None:
                    jobs[n] = _lib.WtableJob(p.data_ptr(), dout, trans, k, nn, 0, e.tables[trans].data_ptr())
                    n += 1
        check(lib.kgcn_wtable_split_multi(ctypes.cast(jobs, ctypes.c_void_p), n, current_stream()), "kgcn_wtable_split_multi")
        for p, e in live:
            e.epoch, e.version = self.epoch, p._version
        for p, q, e in stacked:
            e.epoch, e.version = self.epoch, (p._version, q._version)


enabled_weight_tables = True
weight_tables = WeightTables()


# ---- the host protocol of a dense call, one helper per step: the Functions below decide WHICH route a call takes, these issue it ----
def _w_operand(w, trans, device):
    """-> (tab, nbytes, ready): the weight operand of a wide-layer GEMM -- the fragment table of W (trans = 0) or W^T (trans = 1)
    split by the step's one table launch (ready = 1), else a workspace the call splits into itself (ready = 0); (None, 0, 0)
    where the layer has no table route."""
    tab, nbytes = weight_tables.lookup(w, trans)
    if tab is not None:
        return tab, nbytes, 1
    k, n = (w.shape[1], w.shape[0]) if trans else w.shape
    nbytes = lib.kgcn_dense_fwd_workspace_bytes(k, n)
    if nbytes <= 0:
        return None, 0, 0
    return _lib.workspace(nbytes, device), nbytes, 0


def _dense_fwd(x2d, w, bias, act, stacked=None):
    """-> y = act(x2d @ w + bias).  stacked = (table, bytes) of [w; bias; 0] with x2d.shape[1] rows (WeightTables.lookup_stacked):
    the operand of dense_stacked, which exists only as that table."""
    m, din = x2d.shape
    dout = w.shape[1]
    if stacked is None:
        if w.shape[0] != din:
            raise _lib.KgcnHipError("kernel is %s but inputs have %d features" % (tuple(w.shape), din))
        b = None if bias is None else _f32c(bias, "bias").reshape(-1)
        if b is not None and b.numel() != dout:
            raise _lib.KgcnHipError("bias has %d elements, expected %d" % (b.numel(), dout))
        tab, tb, ready = _w_operand(w, 0, x2d.device)
        if not ready:
            weight_tables.register(w)
    else:
        b, (tab, tb), ready = None, stacked, 1
    y = torch.empty((m, dout), device=x2d.device, dtype=torch.float32)
    if ready:
        check(lib.kgcn_dense_fwd_tab_f32(ptr(x2d), m, din, din, ptr(w), dout, 0, ptr(b), ptr(y), dout,
                                         dout, int(act), ptr(tab), tb, current_stream()), "kgcn_dense_fwd_tab_f32")
    else:
        check(lib.kgcn_dense_fwd_ws_f32(ptr(x2d), m, din, din, ptr(w), dout, 0, ptr(b), ptr(y), dout,
                                        dout, int(act), ptr(tab), tb, current_stream()), "kgcn_dense_fwd_ws_f32")
    return y


def _dense_dx(g, w, x2d):
    """-> dx = g @ w^T (w [din, dout] used transposed), laid out like x2d."""
    m, dout = g.shape
    din = w.shape[0]
    dx = torch.empty_like(x2d)
    tab, tb, ready = _w_operand(w, 1, g.device)
    if ready:
        check(lib.kgcn_dense_fwd_tab_f32(ptr(g), m, dout, dout, ptr(w), dout, 1, None, ptr(dx),
                                         din, din, 0, ptr(tab), tb, current_stream()), "kgcn_dense_fwd_tab_f32(dx)")
    else:
        check(lib.kgcn_dense_fwd_ws_f32(ptr(g), m, dout, dout, ptr(w), dout, 1, None, ptr(dx),
                                        din, din, 0, ptr(tab), tb, current_stream()), "kgcn_dense_fwd_ws_f32(dx)")
    return dx


def _dense_dx_dact(gy, yact, w, act, x2d):
    """-> (dx, dpre): d pre-activation is produced by the dX GEMM itself while it stages the gradient rows (wide layers); the
    weight-gradient GEMM reads it afterwards."""
    m, dout = gy.shape
    din = w.shape[0]
    dx = torch.empty_like(x2d)
    dpre = torch.empty_like(gy)
    tab, tb, ready = _w_operand(w, 1, gy.device)
    if ready:
        check(lib.kgcn_dense_dx_dact_tab_f32(ptr(gy), ptr(yact), m, dout, dout, ptr(w), dout, din, ptr(dx), din, act,
                                             ptr(dpre), ptr(tab), tb, current_stream()), "kgcn_dense_dx_dact_tab_f32")
    else:
        check(lib.kgcn_dense_dx_dact_f32(ptr(gy), ptr(yact), m, dout, dout, ptr(w), dout, din, ptr(dx), din, act,
                                         ptr(dpre), ptr(tab), tb, current_stream()), "kgcn_dense_dx_dact_f32")
    return dx, dpre


_same_stream = contextlib.nullcontext()


def _dense_wgrad(ctx, x2d, w, g, yact, need_w, need_b, dact_pending=False, side=False):
    """-> (dw [x2d.shape[1], dout], db in the bias' shape) = (x2d^T dpre, column sums of dpre).  dact_pending: g is still the gradient
    of the ACTIVATED output and no dX GEMM has formed d pre-activation (a layer whose input needs no gradient): a wide layer
    forms it while the weight-gradient GEMM stages the gradient rows -- no elementwise pass over the [m, dout] tensor -- any
    other takes that pass first.  side: the GEMM may run on the side stream (side_stream_wgrad)."""
    m, din = x2d.shape
    dout = g.shape[1]
    fuse_dact = dact_pending and wgrad_dact_fusion and bool(lib.kgcn_dense_wgrad_dact_supported(din, dout))
    if dact_pending and not fuse_dact:
        g = activation_backward(yact, g, ctx.act)
    stream = None
    if side and side_stream_wgrad and m >= side_wgrad_min_rows:
        stream = _fork_side(g.device)
        for t in (g, x2d, yact):
            t.record_stream(stream)          # the caching allocator must not hand their memory out while the side stream reads it
    with torch.cuda.stream(stream) if stream is not None else _same_stream:
        wsb = lib.kgcn_dense_wgrad_workspace_bytes(m, din, dout)
        # (the operand of dense_stacked, [w; bias; 0], has x2d's width in rows, not w's)
        dw = None if not need_w else torch.empty_like(w) if w.shape[0] == din else \
            torch.empty((din, dout), device=g.device, dtype=torch.float32)
        db = torch.empty((dout,), device=g.device, dtype=torch.float32) if need_b else None
        with _param_grad_stage(ctx, wsb, g.device) as wsp:
            if fuse_dact:
                check(lib.kgcn_dense_wgrad_dact_f32(ptr(x2d), din, ptr(g), ptr(yact), dout, ctx.act, m, din, dout, ptr(dw),
                                                    ptr(db), ptr(wsp), wsb, current_stream()), "kgcn_dense_wgrad_dact_f32")
            else:
                check(lib.kgcn_dense_wgrad_f32(ptr(x2d), din, ptr(g), dout, m, din, dout, ptr(dw),
                                               ptr(db), ptr(wsp), wsb, current_stream()), "kgcn_dense_wgrad_f32")
    return dw, _bias_grad(ctx, db)


def _bias_grad(ctx, db):
    return None if db is None else db.reshape(ctx.bias_shape)


# One-pass backward of the wide layers (kgcn_dense_bwd_f32, csrc/gemmb.hip): dX, dW and dbias from ONE sweep over (grad, act_out,
# x) -- the d pre-activation tensor is never written and read back (six passes over [m, 256] tensors -> four).
dense_bwd_fusion = True


def _dense_bwd_fused_ok(x2d, w, gy, yact, gp=None, gp_ld=0, n_nodes=0, act_is_smooth=False):
    m, din = x2d.shape
    dout = w.shape[1]
    if not (dense_bwd_fusion and lib.kgcn_dense_bwd_supported(m, din, dout)):
        return False
    ts = [t for t in (x2d, gy, yact) if t is not None]
    if not all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts):
        return False
    if gp is None:
        return True
    # (a sigmoid / tanh layer that is read out AND handed on: that kernel form spills registers inside its loop -- two-call route)
    if gy is not None and yact is not None and act_is_smooth:
        return False
    return gp.data_ptr() % 16 == 0 and gp_ld % 4 == 0 and n_nodes >= 8


def _dense_bwd_fused(ctx, x2d, w, gy, yact, act, need_b, gp=None, gp_ld=0, n_nodes=0):
    """-> (dx, dw, db) of y = act(x2d @ w + bias) from one launch (+ the deferrable second stage of dw / db)."""
    m, din = x2d.shape
    dout = w.shape[1]
    dx = torch.empty_like(x2d)
    dw = torch.empty_like(w)
    db = torch.empty((dout,), device=x2d.device, dtype=torch.float32) if need_b else None
    tab, tb, ready = _w_operand(w, 1, x2d.device)
    wsb = lib.kgcn_dense_wgrad_workspace_bytes(m, din, dout)
    with _param_grad_stage(ctx, wsb, x2d.device) as wsp:
        check(lib.kgcn_dense_bwd_f32(ptr(gy), None if gp is None else gp.data_ptr(), gp_ld, n_nodes, ptr(yact) if act else None,
                                     int(act), dout, ptr(x2d), din, m, din, dout, ptr(w), dout, ptr(dx), din, ptr(dw), ptr(db),
                                     ptr(tab), tb, ready, ptr(wsp), wsb, current_stream()), "kgcn_dense_bwd_f32")
    return dx, dw, _bias_grad(ctx, db)


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, w, bias, act=0):
        # (a computed weight -- the concatenated kernels of a multi-channel GraphConv -- is not a leaf: autograd slices its gradient
        # right away, so it does not defer; stack_rows' [w; bias; pad] stands for w and bias, whose gradients are views of it)
        _record_params(ctx, w, bias)
        x2d, w = _f32c(x2d, "x"), _f32c(w, "w")
        y = _dense_fwd(x2d, w, bias, act)
        ctx.act = int(act)
        ctx.save_for_backward(x2d, w, y if act else x2d)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2d, w, yact = ctx.saved_tensors
        gy = _f32c(gy, "grad")
        m = x2d.shape[0]
        dx = dw = db = None
        need_x, need_w = ctx.needs_input_grad[:2]
        need_b = ctx.bias_shape is not None and ctx.needs_input_grad[2]
        if need_x and need_w and not (side_stream_wgrad and m >= side_wgrad_min_rows) and \
                _dense_bwd_fused_ok(x2d, w, gy, yact if ctx.act else None):
            # wide layer that hands a gradient on: dX, dW and dbias in ONE pass over (gy, y, x)
            dx, dw, db = _dense_bwd_fused(ctx, x2d, w, gy, yact, ctx.act, need_b)
            return dx, dw, db, None
        if ctx.act and need_x:
            dx, gy = _dense_dx_dact(gy, yact, w, ctx.act, x2d)
        elif need_x:
            dx = _dense_dx(gy, w, x2d)
        if need_w or need_b:
            # (first layer of a model -- no d inputs: the derivative of the activation is still to be applied)
            dw, db = _dense_wgrad(ctx, x2d, w, gy, yact, need_w, need_b, dact_pending=bool(ctx.act) and not need_x, side=True)
        return dx, dw, db, None


class _StackRows(torch.autograd.Function):
    """[w; bias; pad] along dim 0 (the operand of an aggregate-first GraphConv, layers.py) with a backward that hands out ROW BLOCKS
    of the incoming gradient as views -- nothing reads the gradient's data inside the backward pass, so the second stage of the
    weight-gradient GEMM that produces it may wait for the step's one reduction launch like a leaf parameter's (the output names
    the parameters behind it in `_kgcn_defer_params`; torch.cat's backward does the same slicing, but that is torch's business and
    not a contract)."""

    @staticmethod
    def forward(ctx, w, bias, pad):
        ctx.rows = (w.shape[0], bias.shape[0])
        return torch.cat([w, bias, pad], dim=0)

    @staticmethod
    def backward(ctx, g):
        n0, n1 = ctx.rows
        return g[:n0], g[n0:n0 + n1], None


def stack_rows(w, bias, pad):
    out = _StackRows.apply(w, bias, pad)
    out._kgcn_defer_params = (w, bias)         # _record_params counts / checks THESE: `out` is a new tensor on every call
    return out


class _DenseStacked(torch.autograd.Function):
    """y = act(x2d @ [w; bias; 0]) for an input that needs NO gradient (the first layer's aggregate-first form, layers.py): the operand
    is never assembled -- the forward reads its fragment table (split from w and bias by the step's one table launch), the backward is ONE
    weight-gradient GEMM over x2d whose row blocks ARE d w and d bias (views: nothing reads them inside the pass, so the second stage
    waits for the step's one reduction launch like a leaf parameter's)."""

    @staticmethod
    def forward(ctx, x2d, w, bias, act, tab, tb):
        y = _dense_fwd(x2d, w, None, act, stacked=(tab, tb))
        ctx.act = int(act)
        ctx.save_for_backward(x2d, w, bias, y)
        _record_params(ctx, w, bias)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2d, w, bias, y = ctx.saved_tensors
        din = w.shape[0]
        dwa, _ = _dense_wgrad(ctx, x2d, w, _f32c(gy, "grad"), y, True, False, dact_pending=bool(ctx.act))
        return None, dwa[:din], dwa[din:din + 1].reshape(bias.shape), None, None, None


def dense_stacked(x2d, w, bias, activation=None):
    """act(x2d @ [w; bias; 0]) with x2d [m, rows >= din + 1] -- the GEMM of an aggregate-first GraphConv (A [X | 1 | 0]) [W; b; 0].
    Without a concatenation when the operand's table is ready (inside a training step) and x2d needs no gradient; else stack_rows + dense."""
    rows = x2d.shape[1]
    weight_tables.register_stacked(w, bias, rows)
    # (>= 1,024 rows: below that the dense entry point does not take the table route and would read `rows` rows of w itself)
    if not x2d.requires_grad and x2d.dtype == torch.float32 and x2d.is_contiguous() and bias.dim() == 2 and bias.shape[0] == 1 and \
            x2d.shape[0] >= 1024:
        tab, tb = weight_tables.lookup_stacked(w, bias, rows)
        if tab is not None:
            return _DenseStacked.apply(x2d, w, bias, act_code(activation), tab, tb)
    pad = w.new_zeros((rows - w.shape[0] - 1, w.shape[1]))
    return dense(x2d, stack_rows(w, bias, pad), None, activation=activation)


def dense(x2d, w, bias=None, activation=None):
    """y = act(x2d @ w + bias); the activation rides in the GEMM epilogue."""
    return _Dense.apply(x2d, w, bias, act_code(activation))


def _readout(y, T, N, d, join=None, join_col=0):
    """-> pooled [T, d], the sum over the N node rows of every graph of y [T * N, d] (GraphGather).  join: a [T, wide] buffer whose
    columns join_col .. join_col + d receive it (the concatenation of several read-outs, model_gin.py:61, without a concatenation
    pass: see join_columns); pooled is then that column block."""
    if join is None:
        pooled = torch.empty((T, d), device=y.device, dtype=torch.float32)
        check(lib.kgcn_graph_gather_fwd_f32(ptr(y), T, N, d, ptr(pooled), current_stream()), "kgcn_graph_gather_fwd_f32")
        return pooled
    if join.dtype != torch.float32 or join.dim() != 2 or join.shape[0] != T or not join.is_contiguous() or \
            join_col < 0 or join_col + d > join.shape[1]:
        raise _lib.KgcnHipError("join buffer %s does not take a [%d, %d] read-out at column %d" % (tuple(join.shape), T, d, join_col))
    pooled = join[:, join_col:join_col + d]
    check(lib.kgcn_graph_gather_fwd_ld_f32(ptr(y), T, N, d, pooled.data_ptr(), join.shape[1], current_stream()),
          "kgcn_graph_gather_fwd_ld_f32")
    return pooled


def _readout_grad(gp, gy, T, N, d, shape):
    """-> broadcast of gp [T, d] over the N nodes of every graph (+ gy, the gradient of the rows themselves, when there is one) as a
    new tensor of `shape` -- ONE pass where the row length allows 16-byte accesses.  gp: contiguous float32."""
    g = torch.empty(shape, device=gp.device, dtype=torch.float32)
    if gy is None or d % 4 != 0:
        check(lib.kgcn_graph_gather_bwd_f32(ptr(gp), T, N, d, ptr(g), current_stream()), "kgcn_graph_gather_bwd_f32")
        return g if gy is None else g + gy
    check(lib.kgcn_graph_gather_bwd_add_f32(ptr(gp), ptr(_f32c(gy, "grad")), T, N, d, ptr(g), current_stream()),
          "kgcn_graph_gather_bwd_add_f32")
    return g


class _DenseGather(torch.autograd.Function):
    """y = act(x W + b) of a layer whose output is read out by GraphGather -- and also handed on to the next layer when the
    caller uses y (example_model/model_gin.py:45-60): returns (y [T, N, dout], pooled [T, dout]).  Backward: the incoming
    gradient of node row r is d y[r] + d pooled[r / N]; for wide activated layers the broadcast is formed inside the dX GEMM
    (kgcn_dense_dx_dact_gather_f32) instead of being written out by kgcn_graph_gather_bwd(_add)_f32 and read back."""

    @staticmethod
    def forward(ctx, x2d, w, bias, act, T, N, join=None, join_col=0):
        x2d, w = _f32c(x2d, "x"), _f32c(w, "w")
        m, dout = x2d.shape[0], w.shape[1]
        if m != T * N:
            raise _lib.KgcnHipError("kernel %s / %d graphs of %d nodes do not match inputs %s" % (tuple(w.shape), T, N, tuple(x2d.shape)))
        y = _dense_fwd(x2d, w, bias, act)
        pooled = _readout(y, T, N, dout, join, join_col)
        ctx.act, ctx.T, ctx.N = int(act), int(T), int(N)
        ctx.save_for_backward(x2d, w, y)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        _record_params(ctx, w, bias)
        ctx.set_materialize_grads(False)
        return y.view(T, N, dout), pooled

    @staticmethod
    def backward(ctx, gy, gp):
        x2d, w, y = ctx.saved_tensors
        m, din = x2d.shape
        dout = w.shape[1]
        T, N = ctx.T, ctx.N
        if gy is None and gp is None:
            return None, None, None, None, None, None, None, None
        gy = None if gy is None else _f32c(gy.reshape(m, dout), "grad")
        gp_ld = dout
        need_x, need_w = ctx.needs_input_grad[:2]
        need_b = ctx.bias_shape is not None and ctx.needs_input_grad[2]
        if gp is not None:
            # a column block of a wider gradient (the backward of join_columns / torch.cat) is read where it lies
            strided = gp.dtype == torch.float32 and gp.dim() == 2 and gp.stride(1) == 1 and gp.stride(0) % 4 == 0 and \
                gp.stride(0) >= dout and gp.data_ptr() % 16 == 0
            if strided and ctx.act and need_x and lib.kgcn_dense_dx_dact_gather_supported(m, din, dout):
                gp_ld = gp.stride(0)
            else:
                gp = _f32c(gp, "grad")
        dx = dw = db = None
        if need_x and need_w and (gp is None or (ctx.act and gp.dtype == torch.float32 and gp.dim() == 2 and gp.stride(1) == 1)) and \
                _dense_bwd_fused_ok(x2d, w, gy, y if ctx.act else None, gp, gp_ld if gp is not None else 0, N, ctx.act in (1, 3)):
            # the whole backward in one pass: the read-out's gradient joins (or stands for) the row gradient while the rows are staged
            dx, dw, db = _dense_bwd_fused(ctx, x2d, w, gy, y, ctx.act, need_b, gp, gp_ld if gp is not None else 0, N)
            return dx, dw, db, None, None, None, None, None
        if gp is not None and ctx.act and need_x and lib.kgcn_dense_dx_dact_gather_supported(m, din, dout):
            dx = torch.empty_like(x2d)
            g = torch.empty((m, dout), device=x2d.device, dtype=torch.float32)
            tab, tb, ready = _w_operand(w, 1, x2d.device)
            check(lib.kgcn_dense_dx_dact_gather_f32(ptr(gy), gp.data_ptr(), gp_ld, N, ptr(y), m, dout, dout, ptr(w), dout, din, ptr(dx), din,
                                                    ctx.act, ptr(g), ptr(tab), tb, ready, current_stream()),
                  "kgcn_dense_dx_dact_gather_f32")
        else:
            # incoming gradient as a tensor, then the plain dense backward
            g = gy if gp is None else _readout_grad(gp, gy, T, N, dout, (m, dout))
            if ctx.act:
                g = activation_backward(y, g, ctx.act)
            if need_x:
                dx = _dense_dx(g, w, x2d)
        if need_w or need_b:
            dw, db = _dense_wgrad(ctx, x2d, w, g, y, need_w, need_b)
        return dx, dw, db, None, None, None, None, None


def dense_gather(x3d, w, bias=None, activation=None, join=None, join_col=0):
    """GraphDense followed by GraphGather on [T, N, din] inputs: -> (y [T, N, dout], pooled [T, dout]); use y only if the layer
    output is also handed on.  join / join_col: write the read-out into columns join_col.. of the [T, wide] buffer `join`
    (pooled is then that column block; combine the blocks with join_columns)."""
    T, N, din = x3d.shape
    return _DenseGather.apply(x3d.reshape(T * N, din), w, bias, act_code(activation), T, N, join, int(join_col))


class _JoinColumns(torch.autograd.Function):
    """tf.concat(parts, axis=1) of column blocks that were WRITTEN INTO `buf` by their producers (dense_gather(join=buf)): nothing
    is copied, the gradient of part i is the column block i of the gradient -- a strided view its consumer reads in place."""

    @staticmethod
    def forward(ctx, buf, *parts):
        col = 0
        for p in parts:
            if p.data_ptr() != buf.data_ptr() + 4 * col or p.shape[0] != buf.shape[0] or p.stride(0) != buf.stride(0):
                raise _lib.KgcnHipError("join_columns: part at column %d was not produced into the join buffer" % col)
            col += p.shape[1]
        if col != buf.shape[1]:
            raise _lib.KgcnHipError("join_columns: the parts cover %d of %d columns" % (col, buf.shape[1]))
        ctx.widths = [p.shape[1] for p in parts]
        return buf.view(buf.shape)

    @staticmethod
    def backward(ctx, g):
        out, col = [], 0
        for wd in ctx.widths:
            out.append(g[:, col:col + wd])
            col += wd
        return (None,) + tuple(out)


def join_columns(buf, parts):
    return _JoinColumns.apply(buf, *parts)


# -------------------------------------------------------------------------------------------------
# fused GraphConv (one channel)
# -------------------------------------------------------------------------------------------------
def graphconv_fused_supported(csr, din, dout):
    """Shape test of the fused kernels; they read the row-padded layout (BatchedCSR.padded4()),
    whose per-graph entry count is bounded by max_nnz + 4 * rows."""
    if csr.rows != csr.cols or csr.rows > BatchedCSR.PAD_COL:
        return False
    if csr.row_pad == 0 and csr._p4 is None and csr._make_p4 is None and csr._host is None:
        return False                    # no way to the row-padded copy (ragged-compact / value-substituted containers)
    bound = csr._p4.max_nnz if csr._p4 is not None else csr.max_nnz + 4 * csr.rows
    return bool(lib.kgcn_graphconv_fused_supported(csr.rows, din, dout, bound))


def _fused_adjacency(csr, backward, T, din, dout, with_dx):
    """Descriptor the fused launcher reads: the compact copy (BatchedCSR.compact4()) where the selected kernel reads
    that layout (the FULL forward, the pairs backward), the row-padded one everywhere else.  The compact copy is built
    on first use, never while a hipGraph is being captured (its build reads back to the host)."""
    p4 = csr.padded4()
    if lib.kgcn_graphconv_fused_reads_compact(int(backward), T, p4.rows, din, dout, p4.max_nnz, int(with_dx)):
        c4 = p4.compact4(build=not torch.cuda.is_current_stream_capturing())
        if c4 is not None:
            return c4.desc()
    return p4.desc()


class _GraphConvFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, csr):
        x, w = _f32c(x, "inputs"), _f32c(w, "kernel")
        T, N, din = x.shape
        dout = w.shape[1]
        b = _f32c(bias, "bias").reshape(-1)
        out = torch.empty((T, N, dout), device=x.device, dtype=torch.float32)
        check(lib.kgcn_graphconv_fwd_f32(_fused_adjacency(csr, False, T, din, dout, False), ptr(x), ptr(w), ptr(b),
                                         din, dout, ptr(out), current_stream()), "kgcn_graphconv_fwd_f32")
        ctx.csr = csr
        ctx.bias_shape = tuple(bias.shape)
        _record_params(ctx, w, bias)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = _f32c(g, "grad")
        T, N, din = x.shape
        dout = w.shape[1]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # dW and dbias are the two halves of ONE buffer: the data-parallel exchange all-reduces it where it lies
        # (parallel.GradBucket recognises gradients that already form a contiguous run: no pack / unpack launches)
        dwb = torch.empty((din * dout + dout,), device=x.device, dtype=torch.float32)
        dw, db = dwb[:din * dout].view(din, dout), dwb[din * dout:]
        wsb = lib.kgcn_graphconv_bwd_workspace_bytes(T, din, dout)
        with _param_grad_stage(ctx, wsb, x.device) as wsp:
            check(lib.kgcn_graphconv_bwd_f32(_fused_adjacency(ctx.csr.transpose(), True, T, din, dout, dx is not None),
                                             ptr(x), ptr(w), ptr(g), din, dout, ptr(dx), ptr(dw), ptr(db), ptr(wsp),
                                             wsb, current_stream()), "kgcn_graphconv_bwd_f32")
        return dx, dw, db.reshape(ctx.bias_shape), None


def graphconv_fused(x, w, bias, csr):
    return _GraphConvFused.apply(x, w, bias, csr)


# -------------------------------------------------------------------------------------------------
# GINAggregate
# -------------------------------------------------------------------------------------------------
class _GinAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, adj):
        x = _f32c(x, "inputs")
        T, N, d = x.shape
        if (T, N) != (adj.num_graphs, adj.n_nodes):
            raise _lib.KgcnHipError("inputs %s do not match the adjacency batch (%d graphs x %d nodes)"
                                    % (tuple(x.shape), adj.num_graphs, adj.n_nodes))
        e = None if eps is None else _f32c(eps, "epsilon").reshape(-1)
        out = torch.empty_like(x)
        check(lib.kgcn_gin_aggregate_f32(adj.desc_array(False), adj.num_channels, ptr(x), d, ptr(e),
                                         ptr(out), current_stream()), "kgcn_gin_aggregate_f32")
        ctx.adj = adj
        ctx.save_for_backward(x, e if e is not None else x.new_empty(0))
        ctx.has_eps = e is not None
        ctx.eps_shape = None if eps is None else tuple(eps.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        x, e = ctx.saved_tensors
        adj = ctx.adj
        g = _f32c(g, "grad")
        T, N, d = x.shape
        dx = deps = None
        want_eps = ctx.has_eps and ctx.needs_input_grad[1]
        if ctx.needs_input_grad[0] or want_eps:
            # one call: dx = sum_c (eps_c g + A_c^T g) and d eps_c = <g, x> (the same inner product for every channel,
            # kgcn/layers.py:469), the inner product accumulated while the gradient tiles are staged for the aggregation
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            one = torch.empty((1,), device=x.device, dtype=torch.float32) if want_eps else None
            wsb = lib.kgcn_gin_aggregate_bwd_workspace_bytes(T, N, d)
            wsp = _lib.workspace(wsb, x.device)
            check(lib.kgcn_gin_aggregate_bwd_f32(adj.desc_array(True), adj.num_channels, ptr(g), d,
                                                 ptr(e) if ctx.has_eps else None, ptr(x), ptr(dx), ptr(one), ptr(wsp), wsb,
                                                 current_stream()), "kgcn_gin_aggregate_bwd_f32")
            if want_eps:
                # one channel (the common case): the kernel's output IS the gradient tensor -- no device-to-device copy per layer
                deps = one.reshape(ctx.eps_shape) if adj.num_channels == 1 else \
                    one.expand(adj.num_channels).reshape(ctx.eps_shape).clone()
        return dx, deps, None


def gin_aggregate(x, eps, adj):
    return _GinAggregate.apply(x, eps, adj)


_GIN_DOT = __import__("os").environ.get("KGCN_GIN_DOT") != "0"           # (development A/B: "0" = the two separate ops)


class _GinDense(torch.autograd.Function):
    """GINAggregate followed by an activated wide GraphDense, for an input that needs NO gradient (the first block of
    example_model/model_gin.py:45-50): y = act((eps x + A x) W + b).  The gradient of the aggregation's output is then only needed for
    d eps = <d out, x> (kgcn/layers.py:469): the layer's dX GEMM accumulates that inner product instead of storing its product
    (kgcn_dense_dx_dact_dot_f32) -- the [rows, din] tensor is neither written nor read back by a dot kernel.  Use gin_dense():
    it falls back to the two separate ops whenever a condition of this form does not hold."""

    @staticmethod
    def forward(ctx, x, eps, adj, w, bias, act):
        x, w = _f32c(x, "inputs"), _f32c(w, "w")
        T, N, din = x.shape
        m, dout = T * N, w.shape[1]
        e = _f32c(eps, "epsilon").reshape(-1)
        agg = torch.empty((m, din), device=x.device, dtype=torch.float32)
        check(lib.kgcn_gin_aggregate_f32(adj.desc_array(False), 1, ptr(x), din, ptr(e), ptr(agg), current_stream()),
              "kgcn_gin_aggregate_f32")
        y = _dense_fwd(agg, w, bias, act)
        ctx.act, ctx.eps_shape = int(act), tuple(eps.shape)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        _record_params(ctx, w, bias)
        ctx.save_for_backward(x, agg, w, y)
        return y.view(T, N, dout)

    @staticmethod
    def backward(ctx, gy):
        x, agg, w, y = ctx.saved_tensors
        m, din = agg.shape
        dout = w.shape[1]
        gy = _f32c(gy.reshape(m, dout), "grad")
        deps = torch.empty((1,), device=gy.device, dtype=torch.float32)
        tab, tb, ready = _w_operand(w, 1, gy.device)
        need_w = ctx.needs_input_grad[3]
        need_b = ctx.bias_shape is not None and ctx.needs_input_grad[4]
        if need_w and _dense_bwd_fused_ok(agg, w, gy, y):
            # ONE pass: d eps, dW and dbias from a single sweep over (gy, y, agg, x) -- no d pre-activation tensor either
            dw = torch.empty_like(w)
            db = torch.empty((dout,), device=gy.device, dtype=torch.float32) if need_b else None
            wsb = lib.kgcn_dense_wgrad_workspace_bytes(m, din, dout)
            with _param_grad_stage(ctx, wsb, gy.device) as wsp:
                check(lib.kgcn_dense_bwd_dot_f32(ptr(gy), ptr(y), ctx.act, dout, ptr(agg), din, m, din, dout, ptr(w), dout, ptr(x), din,
                                                 ptr(dw), ptr(db), ptr(deps), ptr(tab), tb, ready, ptr(wsp), wsb, current_stream()),
                      "kgcn_dense_bwd_dot_f32")
            return None, (deps.reshape(ctx.eps_shape) if ctx.needs_input_grad[1] else None), None, dw, _bias_grad(ctx, db), None
        dpre = torch.empty_like(gy)
        wsb = lib.kgcn_dense_dx_dact_dot_workspace_bytes(m, din)
        wsp = _lib.workspace(wsb, gy.device)
        check(lib.kgcn_dense_dx_dact_dot_f32(ptr(gy), ptr(y), m, dout, dout, ptr(w), dout, din, ptr(x), din, ctx.act, ptr(dpre),
                                             ptr(tab), tb, ready, ptr(deps), ptr(wsp), wsb, current_stream()),
              "kgcn_dense_dx_dact_dot_f32")
        dw = db = None
        if need_w or need_b:
            dw, db = _dense_wgrad(ctx, agg, w, dpre, y, need_w, need_b)
        return None, (deps.reshape(ctx.eps_shape) if ctx.needs_input_grad[1] else None), None, dw, db, None


def gin_dense(x, eps, adj, w, bias=None, activation=None):
    """-> act((eps x + A x) @ w + bias), [T, N, dout]; eps: the GINAggregate's epsilon of ONE adjacency channel.  The fused backward
    (no d out tensor: see _GinDense) when x needs no gradient, eps does, the layer is activated and wide enough; else the two ops."""
    T, N, din = x.shape
    act = act_code(activation)
    fused = (not x.requires_grad and eps is not None and eps.requires_grad and eps.numel() == 1 and adj.num_channels == 1 and act and
             torch.is_grad_enabled() and x.dtype == torch.float32 and _GIN_DOT and
             bool(lib.kgcn_dense_dx_dact_dot_supported(T * N, din, w.shape[1])))
    if fused:
        return _GinDense.apply(x, eps, adj, w, bias, act)
    h = gin_aggregate(x, eps, adj)
    return dense(h.reshape(T * N, din), w, bias, activation=activation).reshape(T, N, w.shape[1])


# -------------------------------------------------------------------------------------------------
# GraphMaxPooling
# -------------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj):
        x = _f32c(x, "inputs")
        T, N, d = x.shape
        if (T, N) != (adj.num_graphs, adj.channels[0].cols):
            raise _lib.KgcnHipError("inputs %s do not match the adjacency batch" % (tuple(x.shape),))
        out = torch.empty((T, adj.n_nodes, d), device=x.device, dtype=torch.float32)
        for c, ch in enumerate(adj.channels):            # tf.add_n over the channels
            check(lib.kgcn_graph_maxpool_fwd_f32(ch.desc(), ptr(x), d, ptr(out), 0.0 if c == 0 else 1.0,
                                                 current_stream()), "kgcn_graph_maxpool_fwd_f32")
        ctx.adj = adj
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        adj = ctx.adj
        g = _f32c(g, "grad")
        T, N, d = x.shape
        dx = torch.empty_like(x)
        wsb = lib.kgcn_graph_maxpool_bwd_workspace_bytes(T, adj.n_nodes, d)
        wsp = _lib.workspace(wsb, x.device)
        for c, ch in enumerate(adj.channels):
            check(lib.kgcn_graph_maxpool_bwd_f32(ch.desc(), ch.transpose().desc(), ptr(x), ptr(g), d, ptr(dx),
                                                 0.0 if c == 0 else 1.0, ptr(wsp), wsb, current_stream()),
                  "kgcn_graph_maxpool_bwd_f32")
        return dx, None


def graph_maxpool(x, adj):
    return _MaxPool.apply(x, adj)


# -------------------------------------------------------------------------------------------------
# GAT
# -------------------------------------------------------------------------------------------------
class _Gat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, *weight_a):
        x = _f32c(x, "inputs")
        T, N, d = x.shape
        if (T, N) != (adj.num_graphs, adj.n_nodes) or adj.channels[0].cols != N:
            raise _lib.KgcnHipError("inputs %s do not match the adjacency batch" % (tuple(x.shape),))
        was = [_f32c(w.reshape(-1), "weight_a") for w in weight_a]
        if len(was) != adj.num_channels or any(w.numel() != 2 * d for w in was):
            raise _lib.KgcnHipError("one weight_a [2*%d, 1] per adjacency channel is required" % d)
        out = torch.empty_like(x)
        wsb = lib.kgcn_gat_workspace_bytes(T, N, d)
        ws = _lib.workspace(wsb, x.device)
        for c, ch in enumerate(adj.channels):
            check(lib.kgcn_gat_fwd_f32(ch.desc(), ptr(x), d, ptr(was[c]), ptr(out), 0.0 if c == 0 else 1.0, ptr(ws), wsb,
                                       current_stream()), "kgcn_gat_fwd_f32")
        ctx.adj = adj
        ctx.save_for_backward(x, *was)
        return out

    @staticmethod
    def backward(ctx, g):
        x, *was = ctx.saved_tensors
        adj = ctx.adj
        g = _f32c(g, "grad")
        T, N, d = x.shape
        dx = torch.empty_like(x)
        wsb = lib.kgcn_gat_workspace_bytes(T, N, d)
        ws = _lib.workspace(wsb, x.device)
        dws = []
        for c, ch in enumerate(adj.channels):
            dw = torch.empty(2 * d, device=x.device, dtype=torch.float32)
            check(lib.kgcn_gat_bwd_f32(ch.desc(), ch.transpose().desc(), ptr(x), d, ptr(was[c]), ptr(g), ptr(dx),
                                       0.0 if c == 0 else 1.0, ptr(dw), ptr(ws), wsb, current_stream()),
                  "kgcn_gat_bwd_f32")
            dws.append(dw.reshape(2 * d, 1))
        return (dx, None) + tuple(dws)


def gat(x, adj, weight_a):
    return _Gat.apply(x, adj, *weight_a)


# -------------------------------------------------------------------------------------------------
# decoders: weighted Gram matrix per graph
# -------------------------------------------------------------------------------------------------
class _Gram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = _f32c(x, "inputs")
        T, N, d = x.shape
        wv = None if w is None else _f32c(w.reshape(-1), "kernel")
        out = torch.empty((T, N, N), device=x.device, dtype=torch.float32)
        check(lib.kgcn_gram_fwd_f32(ptr(x), T, N, d, 0 if wv is None else ptr(wv), ptr(out), current_stream()),
              "kgcn_gram_fwd_f32")
        ctx.has_w = wv is not None
        ctx.w_shape = None if w is None else tuple(w.shape)
        ctx.save_for_backward(x, wv if wv is not None else x.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, g):
        x, wv = ctx.saved_tensors
        g = _f32c(g, "grad")
        T, N, d = x.shape
        dx = torch.empty_like(x)
        dw = torch.empty(d, device=x.device, dtype=torch.float32) if ctx.has_w else None
        wsb = lib.kgcn_gram_workspace_bytes(d)
        ws = _lib.workspace(wsb, x.device)
        check(lib.kgcn_gram_bwd_f32(ptr(x), T, N, d, ptr(wv) if ctx.has_w else 0, ptr(g), ptr(dx), 0.0,
                                    ptr(dw) if ctx.has_w else 0, ptr(ws), wsb, current_stream()), "kgcn_gram_bwd_f32")
        return dx, (dw.reshape(ctx.w_shape) if ctx.has_w else None)


def gram(x, w=None):
    """out[t] = (x[t] * w) @ x[t]^T  (w: [d] or None)."""
    return _Gram.apply(x, w)


# -------------------------------------------------------------------------------------------------
# GraphGather
# -------------------------------------------------------------------------------------------------
class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x, "inputs")
        B, N, d = x.shape
        ctx.shape = (B, N, d)
        return _readout(x, B, N, d)

    @staticmethod
    def backward(ctx, g):
        B, N, d = ctx.shape
        g = _f32c(g, "grad")
        dx = torch.empty((B, N, d), device=g.device, dtype=torch.float32)
        check(lib.kgcn_graph_gather_bwd_f32(ptr(g), B, N, d, ptr(dx), current_stream()),
              "kgcn_graph_gather_bwd_f32")
        return dx


def graph_gather(x):
    return _Gather.apply(x)


class _GatherTee(torch.autograd.Function):
    """(x, sum over nodes of x): for a tensor that is read out AND handed to the next layer (model_gin.py:45-60).  Backward:
    d x = d(passed-on x) + broadcast(d pooled) in ONE pass (kgcn_graph_gather_bwd_add_f32) -- separate ops cost a broadcast
    pass plus autograd's accumulation pass over the [B, N, D] tensor."""

    @staticmethod
    def forward(ctx, x):
        x = _f32c(x, "inputs")
        B, N, d = x.shape
        ctx.shape = (B, N, d)
        return x.view_as(x), _readout(x, B, N, d)

    @staticmethod
    def backward(ctx, gx, gp):
        B, N, d = ctx.shape
        return gx if gp is None else _readout_grad(_f32c(gp, "grad"), gx, B, N, d, (B, N, d))


def graph_gather_tee(x):
    """-> (x, pooled [B, D]); use the returned x downstream."""
    return _GatherTee.apply(x)


class _RaggedGather(torch.autograd.Function):
    """GraphGather on a ragged-compact batch (kgcn_amd.ragged): sum of the valid rows + (N - n_b) x the padding
    representative row (quirk Q4: the reference's reduce_sum runs over the padded rows too)."""

    @staticmethod
    def forward(ctx, x, rb):
        x = _f32c(x, "inputs")
        d = x.shape[-1]
        if x.numel() != rb.capacity * d:
            raise _lib.KgcnHipError("inputs %s do not match the ragged batch (capacity %d rows)" % (tuple(x.shape), rb.capacity))
        out = torch.empty((rb.num_graphs, d), device=x.device, dtype=torch.float32)
        check(lib.kgcn_ragged_gather_fwd_f32(ptr(x), ptr(rb.graph_ptr), rb.num_graphs, rb.n_nodes, d, rb.pad_row, ptr(out),
                                             current_stream()), "kgcn_ragged_gather_fwd_f32")
        ctx.rb, ctx.shape = rb, tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        rb = ctx.rb
        g = _f32c(g, "grad")
        d = ctx.shape[-1]
        dx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        wsb = lib.kgcn_ragged_gather_bwd_workspace_bytes(d)
        ws = _lib.workspace(wsb, g.device)
        check(lib.kgcn_ragged_gather_bwd_f32(ptr(g), ptr(rb.graph_ptr), rb.num_graphs, rb.n_nodes, d, rb.pad_row, rb.capacity,
                                             ptr(dx), ptr(ws), wsb, current_stream()), "kgcn_ragged_gather_bwd_f32")
        return dx, None


def ragged_gather(x, rb):
    return _RaggedGather.apply(x, rb)


class _RaggedCompactRows(torch.autograd.Function):
    """Padded [B, N, D] -> the valid rows [1, capacity, D] of a ragged-compact batch; the gradient goes back to the valid
    rows of the padded tensor (zeros on its padded rows)."""

    @staticmethod
    def forward(ctx, padded, rb):
        ctx.rb = rb
        return rb.compact_rows(_f32c(padded, "features"))

    @staticmethod
    def backward(ctx, g):
        return ctx.rb.expand(_f32c(g, "grad"), fill="zero"), None


def ragged_compact_rows(padded, rb):
    return _RaggedCompactRows.apply(padded, rb)


# -------------------------------------------------------------------------------------------------
# cross-layer stack for small graphs (csrc/stack.hip): [GraphConv | GraphDense | BatchNormalization(moving stats)] x k
# (+ GraphGather) in one forward and one backward launch
# -------------------------------------------------------------------------------------------------
# kernels of the cross-layer stack (kgcn_stack_layer.route): 0 automatic, 1 one graph per workgroup trip, 2 64-row tiles (f32 MFMA)
stack_route = 0


def _stack_descriptors(spec, params, buffers):
    """spec: list of (kind, act_code, din, dout, eps); params: flat list, two tensors (or None) per layer (w, b | gamma,
    beta); buffers: per layer (mean, var) or None.  -> (ctypes array of kgcn_stack_layer, keep-alive list)."""
    import ctypes
    arr = (_lib.StackLayer * len(spec))()
    keep = []
    for l, (kind, act, din, dout, eps) in enumerate(spec):
        w, b = params[2 * l], params[2 * l + 1]
        w = _f32c(w.reshape(-1), "stack parameter")
        b = None if b is None else _f32c(b.reshape(-1), "stack parameter")
        mean = var = None
        if kind == 2:
            mean, var = (_f32c(t.reshape(-1), "moving statistics") for t in buffers[l])
        keep += [w, b, mean, var]
        arr[l] = _lib.StackLayer(kind, act, din, dout, w.data_ptr(), 0 if b is None else b.data_ptr(),
                                 0 if mean is None else mean.data_ptr(), 0 if var is None else var.data_ptr(), float(eps),
                                 stack_route if l == 0 else 0)
    return arr, keep


def gcn_stack_supported(csr, spec):
    import ctypes
    if csr.row_pad or csr.rows != csr.cols or csr.rows > 32 or len(spec) > _lib.K["KGCN_STACK_MAX_LAYERS"]:
        return False
    arr = (_lib.StackLayer * len(spec))()
    for l, (kind, act, din, dout, eps) in enumerate(spec):
        arr[l] = _lib.StackLayer(kind, act, din, dout, 1, 1, 1, 1, float(eps), stack_route if l == 0 else 0)   # pointers: NULL checks only
    return bool(lib.kgcn_gcn_stack_supported(csr.rows, csr.max_nnz, arr, len(spec)))


class _GcnStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, csr, enabled, spec, buffers, gather, *params):
        import ctypes
        x = _f32c(x, "inputs")
        T, N, d0 = x.shape
        if (T, N) != (csr.num_graphs, csr.rows) or d0 != spec[0][2]:
            raise _lib.KgcnHipError("inputs %s do not match the adjacency batch / the first layer" % (tuple(x.shape),))
        arr, keep = _stack_descriptors(spec, params, buffers)
        outs = [torch.empty((T, N, s[3]), device=x.device, dtype=torch.float32) for s in spec]
        optr = (ctypes.c_void_p * len(spec))(*[o.data_ptr() for o in outs])
        pooled = torch.empty((T, spec[-1][3]), device=x.device, dtype=torch.float32) if gather else None
        check(lib.kgcn_gcn_stack_fwd_f32(csr.desc(), ptr(x), ptr(enabled), arr, len(spec), optr, ptr(pooled), current_stream()),
              "kgcn_gcn_stack_fwd_f32")
        ctx.csr, ctx.enabled, ctx.spec, ctx.buffers, ctx.gather = csr, enabled, spec, buffers, gather
        ctx.nparams = len(params)
        ctx.save_for_backward(x, *outs, *[p for p in params if p is not None])
        ctx.param_none = [p is None for p in params]
        ctx.param_shapes = [None if p is None else tuple(p.shape) for p in params]
        # (the gradients are views of ONE buffer nothing reads inside the pass: its second stage may wait -- see deferred_reductions)
        _record_params(ctx, *params)
        return pooled if gather else outs[-1]

    @staticmethod
    def backward(ctx, g):
        import ctypes
        spec = ctx.spec
        saved = list(ctx.saved_tensors)
        x, outs, rest = saved[0], saved[1:1 + len(spec)], saved[1 + len(spec):]
        params, it = [], iter(rest)
        for is_none in ctx.param_none:
            params.append(None if is_none else next(it))
        g = _f32c(g, "grad")
        arr, keep = _stack_descriptors(spec, params, ctx.buffers)
        optr = (ctypes.c_void_p * len(spec))(*[o.data_ptr() for o in outs])
        n = int(lib.kgcn_gcn_stack_param_floats(arr, len(spec)))
        dparams = torch.empty((n,), device=g.device, dtype=torch.float32)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        wsb = lib.kgcn_gcn_stack_bwd_workspace_bytes(x.shape[0], arr, len(spec))
        with _param_grad_stage(ctx, wsb, g.device) as ws:
            check(lib.kgcn_gcn_stack_bwd_f32(ctx.csr.transpose().desc(), ptr(x), ptr(ctx.enabled), arr, len(spec), optr, ptr(g),
                                             1 if ctx.gather else 0, ptr(dx), ptr(dparams), ptr(ws), wsb, current_stream()),
                  "kgcn_gcn_stack_bwd_f32")
        grads, off = [], 0
        for l, (kind, act, din, dout, eps) in enumerate(spec):
            nw = dout if kind == 2 else din * dout
            for which, cnt in ((0, nw), (1, dout)):
                i = 2 * l + which
                if ctx.param_none[i]:
                    grads.append(None)
                else:
                    grads.append(dparams[off:off + cnt].reshape(ctx.param_shapes[i]))
                off += cnt
        return (dx, None, None, None, None, None) + tuple(grads)


def gcn_stack(x, csr, enabled, spec, buffers, gather, params):
    """x [T, N, d0]; spec / buffers / params as in _stack_descriptors.  Returns pooled [T, d_last] (gather) or the last
    layer's output [T, N, d_last]."""
    return _GcnStack.apply(x, csr, enabled, tuple(spec), tuple(buffers), bool(gather), *params)


# -------------------------------------------------------------------------------------------------
# aggregate-first GraphConv operand: [X | 1 | 0..]
# -------------------------------------------------------------------------------------------------
class _AugmentOnes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, width):
        x2d = _f32c(x2d, "inputs")
        m, din = x2d.shape
        out = torch.empty((m, width), device=x2d.device, dtype=torch.float32)
        check(lib.kgcn_augment_ones_f32(ptr(x2d), m, din, din, ptr(out), width, current_stream()), "kgcn_augment_ones_f32")
        ctx.shape = (m, din)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g, "grad")
        m, din = ctx.shape
        dx = torch.empty((m, din), device=g.device, dtype=torch.float32)
        check(lib.kgcn_augment_ones_bwd_f32(ptr(g), m, din, g.shape[1], ptr(dx), din, current_stream()),
              "kgcn_augment_ones_bwd_f32")
        return dx, None


def augment_ones(x2d, width):
    """[m, din] -> [m, width] = [x | 1 | 0 ...] (width >= din + 1)."""
    return _AugmentOnes.apply(x2d, width)


# -------------------------------------------------------------------------------------------------
# losses of the model files: one HIP pass (cost per graph, d cost_sum / d logits, partial sums) + one finishing block
# -------------------------------------------------------------------------------------------------
def _grad_scalars(g_opt, g_sum):
    """The upstream gradients of a loss head's (cost_opt, cost_sum) as device scalars (go, gs), either of them None where autograd
    passed none; None when it passed neither."""
    if g_opt is None and g_sum is None:
        return None
    return tuple(None if g is None else _f32c(g.reshape(1), "grad") for g in (g_opt, g_sum))


def _accum_block(accum, n, who, layout):
    """Check the optional epoch accumulator of a task-column loss head: n = `layout` floats."""
    if accum is None:
        return
    require_gpu(accum, "accum")
    if accum.dtype != torch.float32 or not accum.is_contiguous() or accum.numel() != n:
        raise _lib.KgcnHipError("%s: the accumulator is a contiguous float32 block of %s = %d" % (who, layout, n))


def _loss_grad(dlog, g_opt, g_sum, batch):
    """d logits = dlog * (g_sum + g_opt / batch) in one launch (kgcn_loss_grad_f32)."""
    g = _grad_scalars(g_opt, g_sum)
    if g is None:
        return None
    go, gs = g
    out = torch.empty_like(dlog)
    check(lib.kgcn_loss_grad_f32(ptr(dlog), ptr(go), ptr(gs), batch, dlog.numel(), ptr(out), current_stream()), "kgcn_loss_grad_f32")
    return out


_pos_weight_cache = {}         # id(host object) -> (the object itself, content bytes, device, device tensor)


def _pos_weight_operand(pos_weight, W, device):
    """-> (scalar weight, per-task device tensor or None).  A HOST per-task pos_weight (list / numpy array / CPU tensor -- the
    reference's info.pos_weight is a numpy array, kgcn/data_util.py:563-568) is uploaded ONCE and cached on its content: a
    per-step torch.as_tensor(...).to(device) is a synchronous pageable copy every forward and an illegal operation inside a
    hipGraph capture.  Device tensors are used where they lie (a 1-element one is broadcast on the device: no float() sync)."""
    if pos_weight is None:
        return 0.0, None
    if torch.is_tensor(pos_weight) and pos_weight.is_cuda:
        qv = pos_weight.detach().to(torch.float32).reshape(-1)
        if qv.numel() == 1:
            qv = qv.expand(W)
        if qv.numel() != W:
            raise _lib.KgcnHipError("pos_weight has %d entries for %d tasks" % (qv.numel(), W))
        return 0.0, qv.contiguous()
    if not (torch.is_tensor(pos_weight) or hasattr(pos_weight, "__len__")):
        return float(pos_weight), None
    host = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)
    if host.numel() == 1:
        return float(host), None
    if host.numel() != W:
        raise _lib.KgcnHipError("pos_weight has %d entries for %d tasks" % (host.numel(), W))
    content = host.numpy().tobytes()
    hit = _pos_weight_cache.get(id(pos_weight))
    if hit is not None and hit[0] is pos_weight and hit[1] == content and hit[2] == device:
        return 0.0, hit[3]
    if torch.cuda.is_current_stream_capturing():
        raise _lib.KgcnHipError("a host pos_weight was first seen (or changed) while a hipGraph is being captured: pass a device "
                                "tensor, or run one eager step with this pos_weight before the capture")
    if len(_pos_weight_cache) >= 64:
        _pos_weight_cache.clear()
    qv = host.to(device).contiguous()
    _pos_weight_cache[id(pos_weight)] = (pos_weight, content, device, qv)
    return 0.0, qv


class _MaskedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mask, mask_label, kind, pos_weight):
        x = _f32c(logits, "logits")
        if x.dim() != 2:
            raise _lib.KgcnHipError("logits must be [batch, width], got %s" % (tuple(x.shape),))
        B, W = x.shape
        z = _f32c(labels.to(torch.float32), "labels")
        mk = _f32c(mask.to(torch.float32).reshape(-1), "mask")
        ml = None if mask_label is None else _f32c(mask_label.to(torch.float32), "mask_label")
        if tuple(z.shape) != (B, W) or mk.numel() != B or (ml is not None and tuple(ml.shape) != (B, W)):
            raise _lib.KgcnHipError("labels / mask / mask_label do not match logits %s" % (tuple(x.shape),))
        dlog = torch.empty_like(x)
        sums = torch.empty((2,), device=x.device, dtype=torch.float32)
        wsb = lib.kgcn_loss_workspace_bytes(B)
        ws = _lib.workspace(wsb, x.device)
        if kind == "sigmoid":
            # info.pos_weight of the reference is one weight per label column (kgcn/data_util.py:563-568, consumed by
            # example_model/model_multitask.py:72-76); a scalar is accepted too and applies to every task
            qs, qv = _pos_weight_operand(pos_weight, W, x.device)
            check(lib.kgcn_masked_sigmoid_ce_f32(ptr(x), ptr(z), ptr(mk), ptr(ml), B, W, 0 if pos_weight is None else 1,
                                                 qs, ptr(qv), None, ptr(dlog), ptr(sums), ptr(ws), wsb, current_stream()),
                  "kgcn_masked_sigmoid_ce_f32")
        else:
            check(lib.kgcn_masked_softmax_ce_f32(ptr(x), ptr(z), ptr(mk), B, W, None, ptr(dlog), ptr(sums), ptr(ws), wsb,
                                                 current_stream()), "kgcn_masked_softmax_ce_f32")
        ctx.save_for_backward(dlog)
        ctx.batch = B
        ctx.set_materialize_grads(False)           # an output nobody differentiates must not become a zero-filled gradient
        return sums[1], sums[0]                    # cost_opt (mean over the padded batch, Q5), cost_sum

    @staticmethod
    def backward(ctx, g_opt, g_sum):
        (dlog,) = ctx.saved_tensors
        return _loss_grad(dlog, g_opt, g_sum, ctx.batch), None, None, None, None, None


class _SparseCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label_idx):
        x = _f32c(logits, "logits")
        B, W = x.shape
        idx = label_idx.reshape(-1).to(torch.int64).contiguous()
        require_gpu(idx, "labels")
        if idx.numel() != B:
            raise _lib.KgcnHipError("labels have %d entries for %d rows of logits" % (idx.numel(), B))
        dlog = torch.empty_like(x)
        sums = torch.empty((2,), device=x.device, dtype=torch.float32)
        wsb = lib.kgcn_loss_workspace_bytes(B)
        ws = _lib.workspace(wsb, x.device)
        check(lib.kgcn_sparse_softmax_ce_f32(ptr(x), ptr(idx), None, B, W, None, ptr(dlog), ptr(sums), ptr(ws), wsb,
                                             current_stream()), "kgcn_sparse_softmax_ce_f32")
        ctx.save_for_backward(dlog)
        return sums[0]

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors
        return _loss_grad(dlog, None, g, 1), None          # dlog * g in the library's launch (no ATen kernel in the step)


def sparse_softmax_ce_sum(logits, label_idx):
    """example_model/sparse.py:112-113: reduce_sum(sparse_softmax_cross_entropy_with_logits(labels, logits))."""
    return _SparseCE.apply(logits, label_idx)


def masked_sigmoid_ce(logits, labels, mask, mask_label=None, pos_weight=None):
    """example_model/model_multitask.py:66-79 -> (cost_opt, cost_sum)."""
    return _MaskedCE.apply(logits, labels, mask, mask_label, "sigmoid", pos_weight)


def masked_softmax_ce(logits, labels, mask):
    """example_model/model.py:56-61 -> (cost_opt, cost_sum)."""
    return _MaskedCE.apply(logits, labels, mask, None, "softmax", None)


__all__ = ["BatchedCSR", "BatchedAdjacency", "bspmm", "bspmm_raw", "bconv", "dense", "activation", "act_code",
           "graphconv_fused", "graphconv_fused_supported", "gin_aggregate", "graph_gather",
           "graph_maxpool", "gat", "gram", "ragged_gather", "ragged_compact_rows",
           "masked_sigmoid_ce", "masked_softmax_ce", "sparse_softmax_ce_sum", "augment_ones",
           "gcn_stack", "gcn_stack_supported", "graph_gather_tee"]


# -------------------------------------------------------------------------------------------------
# GraphBatchNormalization (kgcn/layers.py:170-220): statistics / apply / backward over the valid node rows
# -------------------------------------------------------------------------------------------------
def graph_bn_stats(x, enabled=None):
    """Batch mean and (population) variance per feature over the valid rows of x [T, N, D] (training mode)."""
    x = _f32c(x, "inputs")
    T, N, D = x.shape
    mean = torch.empty((D,), device=x.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    wsb = lib.kgcn_graph_bn_workspace_bytes(D)
    wsp = _lib.workspace(wsb, x.device)
    check(lib.kgcn_graph_bn_stats_f32(ptr(x), T, N, D, ptr(enabled), ptr(mean), ptr(var), ptr(wsp), wsb,
                                      current_stream()), "kgcn_graph_bn_stats_f32")
    return mean, var


class _GraphBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mean, var, enabled, eps, training, act=0):
        x = _f32c(x, "inputs")
        T, N, D = x.shape
        # learning phase 0: d gamma / d beta are not read inside the backward call (the C side queues their second stage in a deferral scope)
        _record_params(ctx, gamma, beta, when=not training)
        gamma, beta = _f32c(gamma, "gamma"), _f32c(beta, "beta")
        y = torch.empty_like(x)
        check(lib.kgcn_graph_bn_apply_act_f32(ptr(x), T, N, D, ptr(enabled), ptr(mean), ptr(var), ptr(gamma), ptr(beta),
                                              float(eps), int(act), ptr(y), current_stream()), "kgcn_graph_bn_apply_act_f32")
        ctx.save_for_backward(x, gamma, mean, var, y if act else x)
        ctx.enabled, ctx.eps, ctx.training, ctx.act = enabled, float(eps), bool(training), int(act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, var, yact = ctx.saved_tensors
        g = _f32c(g, "grad")
        T, N, D = x.shape
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgamma = torch.empty((D,), device=x.device, dtype=torch.float32)
        dbeta = torch.empty_like(dgamma)
        wsb = lib.kgcn_graph_bn_workspace_bytes(D)
        # d gamma / d beta receive their second stage at the flush: AccumulateGrad must take the two tensors themselves as
        # .grad.  They must NOT be referenced from here as well: a second reference makes AccumulateGrad clone them -- before
        # the flush has written them (and costs two copy launches per step).
        with _param_grad_stage(ctx, wsb, x.device, when=dx is not None) as wsp:
            check(lib.kgcn_graph_bn_bwd_dact_f32(ptr(x), ptr(g), ptr(yact) if ctx.act else None, ctx.act, T, N, D,
                                                 ptr(ctx.enabled), ptr(mean), ptr(var), ptr(gamma), ctx.eps, int(ctx.training),
                                                 ptr(dx), ptr(dgamma), ptr(dbeta), ptr(wsp), wsb, current_stream()),
                  "kgcn_graph_bn_bwd_dact_f32")
        return dx, dgamma, dbeta, None, None, None, None, None, None


def graph_bn(x, gamma, beta, mean, var, enabled=None, eps=1e-3, training=False, activation=None):
    """y = act(gamma (x - mean) / sqrt(var + eps) + beta on the valid rows, 0 on the padding rows).  training=True: mean /
    var are THIS batch's statistics and the backward differentiates through them.  The activation rides in the same pass
    (and its derivative in the backward's reads)."""
    return _GraphBN.apply(x, gamma, beta, mean, var, enabled, eps, training, act_code(activation))


# -------------------------------------------------------------------------------------------------
# graph VAE (example_model/model_vae.py; csrc/vae.hip): counter-based noise, reparameterisation + KL, reconstruction loss
# -------------------------------------------------------------------------------------------------
VAE_MAX_NODES, VAE_MAX_CHANNELS, VAE_MAX_DIM = (_lib.K[n] for n in ("KGCN_VAE_MAX_NODES", "KGCN_VAE_MAX_CHANNELS", "KGCN_VAE_MAX_DIM"))


def _step_ptr(step):
    """A device int64 scalar (read by the kernel at run time, e.g. TFAdam._t_dev) or None (step 0)."""
    if step is None:
        return None
    if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.int64 and step.numel() == 1):
        raise _lib.KgcnHipError("step must be a one-element int64 device tensor (or None)")
    return step


def philox4x64_raw(seed, step, num_blocks, device):
    """Words of Philox4x64-10 blocks 0 .. num_blocks-1, key (seed, 0), counter (j, step, 0, 0): int64 [num_blocks, 4]
    holding the uint64 bit patterns."""
    out = torch.empty((int(num_blocks), 4), device=device, dtype=torch.int64)
    check(lib.kgcn_philox4x64_raw(int(seed) & (2 ** 64 - 1), ptr(_step_ptr(step)), int(num_blocks), ptr(out), current_stream()),
          "kgcn_philox4x64_raw")
    return out


def normal(seed, step, shape, device):
    """The noise the VAE sample kernels draw for (seed, step): N(0, 1) values of Philox4x64-10 + Box-Muller (include/kgcn_hip.h)."""
    out = torch.empty(shape, device=device, dtype=torch.float32)
    check(lib.kgcn_normal_f32(int(seed) & (2 ** 64 - 1), ptr(_step_ptr(step)), out.numel(), ptr(out), current_stream()),
          "kgcn_normal_f32")
    return out


class _VaeSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ms, n_nodes, eps, seed, step, copies):
        ms = _f32c(ms, "mean / std pre-activations")
        if ms.dim() != 2 or ms.shape[1] % 2:
            raise _lib.KgcnHipError("mean / std pre-activations must be [batch, 2 width], got %s" % (tuple(ms.shape),))
        B, D = ms.shape[0], ms.shape[1] // 2
        e = None if eps is None else _f32c(eps, "epsilon")
        if e is not None and tuple(e.shape) != (B, n_nodes, D):
            raise _lib.KgcnHipError("epsilon is %s, expected %s" % (tuple(e.shape), (B, n_nodes, D)))
        z = torch.empty((B, n_nodes, D), device=ms.device, dtype=torch.float32)
        kl = torch.empty((B,), device=ms.device, dtype=torch.float32)
        check(lib.kgcn_vae_sample_fwd_f32(ptr(ms), ms.data_ptr() + 4 * D, B, n_nodes, D, 2 * D, ptr(e), int(seed) & (2 ** 64 - 1),
                                          ptr(step), ptr(z), ptr(kl), current_stream()), "kgcn_vae_sample_fwd_f32")
        ctx.save_for_backward(ms, e if e is not None else ms.new_empty(0))
        ctx.has_eps, ctx.seed, ctx.step, ctx.n_nodes = e is not None, seed, step, n_nodes
        ctx.set_materialize_grads(False)
        # one view of z per consumer: their gradients are added inside the backward kernel, not by an autograd add
        return (kl,) + tuple(z.view(B, n_nodes, D) for _ in range(copies))

    @staticmethod
    def backward(ctx, gkl, *gz):
        ms, e = ctx.saved_tensors
        B, D = ms.shape[0], ms.shape[1] // 2
        gz = [_f32c(g, "grad") for g in gz if g is not None]
        if not gz:
            gz = [ms.new_zeros((B, ctx.n_nodes, D))]
        gk = None if gkl is None else _f32c(gkl, "grad")
        dms = torch.empty_like(ms)
        check(lib.kgcn_vae_sample_bwd_f32(ptr(ms), ms.data_ptr() + 4 * D, B, ctx.n_nodes, D, 2 * D, ptr(e) if ctx.has_eps else None,
                                          int(ctx.seed) & (2 ** 64 - 1), ptr(ctx.step), _ptr_array(gz), len(gz), ptr(gk), ptr(dms),
                                          dms.data_ptr() + 4 * D, current_stream()), "kgcn_vae_sample_bwd_f32")
        return dms, None, None, None, None, None


def vae_sample(ms, n_nodes, eps=None, seed=0, step=None, copies=1):
    """model_vae.py:89-96, 169-181 -> (kl [B], z [B, N, D] x copies).  ms [B, 2 D]: the mean Dense layer's pre-activation in
    columns 0 .. D-1, the std layer's in D .. 2D-1 (both layers as ONE GEMM over [W_mean | W_std]: the read-out they share gets
    one gradient, no autograd add).  mean = clip(., -100, 100), std = clip(sqrt(softplus(.)), -5, 5), z = mean + std * eps
    (the reference's `epsilon` placeholder when `eps` is given, the (seed, step) Philox noise otherwise, step a device int64
    read at run time); kl[b] = N sum_k (1 + 2 log(std + 1e-10) - mean^2 - std).  `copies` views of z, one per consumer, whose
    gradients the backward kernel adds; eps is regenerated there, never stored."""
    if not 1 <= int(copies) <= VAE_MAX_CHANNELS + 1:
        raise _lib.KgcnHipError("vae_sample: 1..%d copies of z" % (VAE_MAX_CHANNELS + 1))
    return _VaeSample.apply(ms, int(n_nodes), eps, seed, _step_ptr(step), int(copies))


def _ptr_array(ts):
    arr = (ctypes.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _vae_adj(adj, C, B, N):
    if not isinstance(adj, BatchedAdjacency):
        raise _lib.KgcnHipError("vae_recon needs a packed kgcn_amd.BatchedAdjacency")
    if adj.num_channels != C or adj.num_graphs != B or adj.n_nodes != N:
        raise _lib.KgcnHipError("adjacency (%d channels, %d graphs x %d nodes) does not match the decoders (%d, %d x %d)"
                                % (adj.num_channels, adj.num_graphs, adj.n_nodes, C, B, N))
    return adj.desc_array(False)


class _VaeRecon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, adj, mask, feat_target, kl, feat_logits, *yw):
        C = len(yw) // 2
        ys = [_f32c(t, "decoder output") for t in yw[:C]]
        ws = [_f32c(t.reshape(-1), "DistMult kernel") for t in yw[C:]]
        xf, tf = _f32c(feat_logits, "decoded features"), _f32c(feat_target, "features")
        B, N, D = ys[0].shape
        F = xf.shape[2]
        if any(tuple(y.shape) != (B, N, D) for y in ys) or any(w.numel() != D for w in ws) or tuple(tf.shape) != tuple(xf.shape) \
                or tuple(xf.shape[:2]) != (B, N):
            raise _lib.KgcnHipError("vae_recon: operand shapes disagree")
        mk = None if mask is None else _f32c(mask.to(torch.float32).reshape(-1), "mask")
        klc = None if kl is None else _f32c(kl, "kl")
        desc = _vae_adj(adj, C, B, N)
        per_graph = torch.empty((3, B), device=xf.device, dtype=torch.float32)
        sums = torch.empty((3,), device=xf.device, dtype=torch.float32)
        check(lib.kgcn_vae_recon_fwd_f32(desc, C, _ptr_array(ys), _ptr_array(ws), D, ptr(xf), ptr(tf), F, ptr(mk), ptr(klc),
                                         ptr(per_graph), ptr(sums), current_stream()), "kgcn_vae_recon_fwd_f32")
        ctx.adj, ctx.C, ctx.has_kl = adj, C, kl is not None
        ctx.w_shapes = [tuple(t.shape) for t in yw[C:]]
        _record_params(ctx, *yw[C:])
        ctx.save_for_backward(xf, tf, mk if mk is not None else xf.new_empty(0), *ys, *ws)
        ctx.has_mask = mk is not None
        ctx.set_materialize_grads(False)
        return sums[0], sums[1], sums[2]

    @staticmethod
    def backward(ctx, g_opt, g_sum, _g_count):
        saved = ctx.saved_tensors
        xf, tf, mk = saved[:3]
        C = ctx.C
        ys, ws = saved[3:3 + C], saved[3 + C:]
        B, N, D = ys[0].shape
        F = xf.shape[2]
        g = _grad_scalars(g_opt, g_sum)
        if g is None:
            return (None,) * (5 + 2 * C)
        go, gs = g
        dys = [torch.empty_like(y) for y in ys]
        dws = [torch.empty((D,), device=xf.device, dtype=torch.float32) for _ in range(C)]
        dxf = torch.empty_like(xf)
        dkl = torch.empty((B,), device=xf.device, dtype=torch.float32) if (ctx.has_kl and go is not None) else None
        wsb = lib.kgcn_vae_recon_workspace_bytes(B, C, D)
        with _param_grad_stage(ctx, wsb, xf.device) as wsp:
            check(lib.kgcn_vae_recon_bwd_f32(_vae_adj(ctx.adj, C, B, N), C, _ptr_array(ys), _ptr_array(ws), D, ptr(xf), ptr(tf), F,
                                             ptr(mk) if ctx.has_mask else None, ptr(go), ptr(gs), _ptr_array(dys),
                                             _ptr_array(dws), ptr(dxf), ptr(dkl), ptr(wsp), wsb, current_stream()),
                  "kgcn_vae_recon_bwd_f32")
        return (None, None, None, dkl, dxf) + tuple(dys) + tuple(dw.view(s) for dw, s in zip(dws, ctx.w_shapes))


def vae_recon(adj, ys, ws, feat_logits, feat_target, mask=None, kl=None):
    """model_vae.py:203-253 -> (cost_opt, cost_sum, correct_count), none of them materialising the [B, C, N, N] logits:
    ys[c] [B, N, D] / ws[c] [D] the link decoder output and DistMult kernel of adjacency channel c, adj the packed target
    adjacency (kgcn_amd.BatchedAdjacency, C channels), feat_logits / feat_target [B, N, F], mask [B] (None = ones), kl [B]
    the per-graph KL sums of vae_sample (None = no KL term).  Limits: N <= 128, C <= 8, D <= 64 (larger shapes raise)."""
    if len(ys) != len(ws) or not ys:
        raise _lib.KgcnHipError("vae_recon: one decoder output and one DistMult kernel per channel")
    return _VaeRecon.apply(adj, mask, feat_target, kl, feat_logits, *ys, *ws)


# -------------------------------------------------------------------------------------------------
# multimodal sequence encoder (example_model/model_multimodal.py:70-93; csrc/seq.hip): fused embedding + Conv1D + relu +
# MaxPooling1D, and the go_backwards LSTM
# -------------------------------------------------------------------------------------------------
SEQ_MAX_EMBED, SEQ_MAX_FILTERS, SEQ_MAX_KERNEL, SEQ_MAX_POOL = (_lib.K[n] for n in (
    "KGCN_SEQ_MAX_EMBED", "KGCN_SEQ_MAX_FILTERS", "KGCN_SEQ_MAX_KERNEL", "KGCN_SEQ_MAX_POOL"))
SEQ_MAX_UNITS, SEQ_MAX_LSTM_INPUT, SEQ_MAX_SYMBOLS, SEQ_MAX_LENGTH = (_lib.K[n] for n in (
    "KGCN_SEQ_MAX_UNITS", "KGCN_SEQ_MAX_LSTM_INPUT", "KGCN_SEQ_MAX_SYMBOLS", "KGCN_SEQ_MAX_LENGTH"))
RECURRENT_ACTIVATIONS = {"hard_sigmoid": _lib.K["KGCN_SEQ_ACT_HARD_SIGMOID"], "sigmoid": _lib.K["KGCN_SEQ_ACT_SIGMOID"]}


def seq_limits_check(length=None, symbols=None, embed_dim=None, kernel_size=None, filters=None, pool=None, units=None,
                     in_dim=None):
    """Raise KgcnHipError for a sequence-encoder shape beyond the kernels' limits (include/kgcn_hip.h); None = not checked."""
    for name, v, hi in (("length", length, SEQ_MAX_LENGTH), ("symbols", symbols, SEQ_MAX_SYMBOLS),
                        ("embedding width", embed_dim, SEQ_MAX_EMBED), ("kernel size", kernel_size, SEQ_MAX_KERNEL),
                        ("filters", filters, SEQ_MAX_FILTERS), ("pool size", pool, SEQ_MAX_POOL), ("units", units, SEQ_MAX_UNITS),
                        ("LSTM input width", in_dim, SEQ_MAX_LSTM_INPUT)):
        if v is not None and not 1 <= int(v) <= hi:
            raise _lib.KgcnHipError("sequence encoder: %s %d outside 1..%d" % (name, int(v), hi))


def _tokens2d(tokens):
    if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.dtype == torch.int32 and tokens.dim() == 2):
        raise _lib.KgcnHipError("tokens must be an int32 [batch, length] device tensor")
    return tokens.contiguous()


def _conv_bias(bias, filters):
    b = _f32c(bias, "conv bias").reshape(-1)
    if b.numel() != filters:
        raise _lib.KgcnHipError("conv bias %s does not match %d filters" % (tuple(bias.shape), filters))
    return b


class _SeqConvPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, table, w, bias, pool):
        tokens = _tokens2d(tokens)
        table, w, b = _f32c(table, "embedding table"), _f32c(w, "conv kernel"), _f32c(bias, "conv bias").reshape(-1)
        B, L = tokens.shape
        S, E = table.shape
        k, F = w.shape[0], w.shape[2]
        if w.dim() != 3 or w.shape[1] != E or b.numel() != F:
            raise _lib.KgcnHipError("conv kernel %s / bias %s do not match an embedding width of %d" % (tuple(w.shape), tuple(b.shape), E))
        seq_limits_check(L, S, E, k, F, pool)
        T = L // pool
        out = torch.empty((B, T, F), device=table.device, dtype=torch.float32)
        train = any(ctx.needs_input_grad[1:4])
        arg = torch.empty((B, T, F), device=table.device, dtype=torch.uint8) if train else None
        check(lib.kgcn_seq_convpool_fwd_f32(ptr(tokens), B, L, ptr(table), S, E, ptr(w), ptr(b), k, F, int(pool), ptr(out), ptr(arg),
                                            current_stream()), "kgcn_seq_convpool_fwd_f32")
        if train:
            ctx.save_for_backward(tokens, table, w, arg)
            ctx.pool, ctx.bias_shape = int(pool), tuple(bias.shape)
            _record_params(ctx, table, w, bias)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None or not any(ctx.needs_input_grad[1:4]):
            return None, None, None, None, None
        tokens, table, w, arg = ctx.saved_tensors
        B, L = tokens.shape
        S, E = table.shape
        k, F = w.shape[0], w.shape[2]
        g = _f32c(g, "grad")
        dtable, dw = torch.empty_like(table), torch.empty_like(w)
        db = torch.empty((F,), device=w.device, dtype=torch.float32)
        wsb = lib.kgcn_seq_convpool_workspace_bytes(B, L, S, E, k, F, ctx.pool)
        with _param_grad_stage(ctx, wsb, w.device) as wsp:
            check(lib.kgcn_seq_convpool_bwd_f32(ptr(tokens), B, L, ptr(table), S, E, ptr(w), k, F, ctx.pool, ptr(g), ptr(arg), ptr(dtable),
                                                ptr(dw), ptr(db), ptr(wsp), wsb, current_stream()), "kgcn_seq_convpool_bwd_f32")
        n = ctx.needs_input_grad
        return None, dtable if n[1] else None, dw if n[2] else None, db.view(ctx.bias_shape) if n[3] else None, None


def seq_conv_pool(tokens, table, w, bias, pool):
    """Embedding(table) -> Conv1D(w [k, E, F], bias, padding='same', relu) -> MaxPooling1D(pool) of model_multimodal.py:75-85 in one
    pass: tokens [B, L] int32 (in [0, S): validated when the dataset is loaded, data_util.sequence_table) -> [B, L // pool, F].
    The backward routes the gradient to the lowest-index maximum of each window (a byte per output, written only when a
    gradient is needed) and forms d table / d w / d bias in deferrable fixed-order partials."""
    return _SeqConvPool.apply(tokens, table, w, bias, int(pool))


class _SeqLSTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wx, wh, bias, act, out, out_col):
        x, wx, wh = _f32c(x, "LSTM input"), _f32c(wx, "LSTM kernel"), _f32c(wh, "LSTM recurrent kernel")
        b = _f32c(bias, "LSTM bias").reshape(-1)
        B, T, D = x.shape
        H = wh.shape[0]
        if tuple(wx.shape) != (D, 4 * H) or tuple(wh.shape) != (H, 4 * H) or b.numel() != 4 * H:
            raise _lib.KgcnHipError("LSTM weights %s / %s / %s do not match input width %d" % (tuple(wx.shape), tuple(wh.shape),
                                                                                            tuple(b.shape), D))
        seq_limits_check(length=max(T, 1), units=H, in_dim=D)
        if out is None:
            out = torch.empty((B, H), device=x.device, dtype=torch.float32)
            out_col = 0
        elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or not out.is_contiguous() or \
                out_col < 0 or out_col + H > out.shape[1]:
            raise _lib.KgcnHipError("output buffer %s does not take [%d, %d] at column %d" % (tuple(out.shape), B, H, out_col))
        h = out[:, out_col:out_col + H]
        train = any(ctx.needs_input_grad[:4])
        stash = torch.empty((max(lib.kgcn_seq_lstm_stash_floats(B, T, H), 1),), device=x.device, dtype=torch.float32) if train else None
        check(lib.kgcn_seq_lstm_fwd_f32(ptr(x), B, T, D, ptr(wx), ptr(wh), ptr(b), H, act, h.data_ptr(), out.shape[1], ptr(stash),
                                        current_stream()), "kgcn_seq_lstm_fwd_f32")
        if train:
            ctx.save_for_backward(x, wx, wh, b, stash)
            ctx.act, ctx.bias_shape, ctx.used = act, tuple(bias.shape), False
            _record_params(ctx, wx, wh, bias)
        ctx.set_materialize_grads(False)
        return h

    @staticmethod
    def backward(ctx, g):
        n = ctx.needs_input_grad
        if g is None or not any(n[:4]):
            return (None,) * 7
        if ctx.used:
            raise _lib.KgcnHipError("seq_lstm: the backward consumes its stash and runs once per forward")
        ctx.used = True
        x, wx, wh, b, stash = ctx.saved_tensors
        B, T, D = x.shape
        H = wh.shape[0]
        if g.dtype != torch.float32 or g.stride(1) != 1 or g.stride(0) < H:
            g = _f32c(g, "grad")
        dx = torch.empty_like(x) if n[0] else None
        need_w = any(n[1:4])
        dwx = torch.empty_like(wx) if need_w else None
        dwh = torch.empty_like(wh) if need_w else None
        db = torch.empty((4 * H,), device=x.device, dtype=torch.float32) if need_w else None
        wsb = lib.kgcn_seq_lstm_workspace_bytes(B, T, D, H) if need_w else 0
        with _param_grad_stage(ctx, wsb, x.device) as wsp:
            check(lib.kgcn_seq_lstm_bwd_f32(ptr(x), B, T, D, ptr(wx), ptr(wh), ptr(b), H, ctx.act, g.data_ptr(), g.stride(0), ptr(stash),
                                            ptr(dx), ptr(dwx), ptr(dwh), ptr(db), ptr(wsp), wsb, current_stream()), "kgcn_seq_lstm_bwd_f32")
        return (dx, dwx if n[1] else None, dwh if n[2] else None, db.view(ctx.bias_shape) if n[3] else None, None, None, None)


def seq_lstm(x, wx, wh, bias, recurrent_activation="hard_sigmoid", out=None, out_col=0):
    """K.layers.LSTM(H, return_sequences=False, go_backwards=True) of model_multimodal.py:88-91 (Keras v1 cell, gates i, f, c, o):
    x [B, T, D], kernel wx [D, 4H], recurrent kernel wh [H, 4H], bias [4H] -> h after input step 0 [B, H].  out / out_col: h is
    written into columns out_col .. out_col + H of the contiguous [B, wide] buffer `out` (a column block of a concatenation,
    join_columns) and returned as that view.  Training keeps a stash of 6H floats per sequence step (gate pre-activations, h, c);
    the backward consumes it (one backward per forward)."""
    try:
        act = RECURRENT_ACTIVATIONS[recurrent_activation]
    except KeyError:
        raise _lib.KgcnHipError("recurrent_activation must be one of %s" % sorted(RECURRENT_ACTIVATIONS)) from None
    return _SeqLSTM.apply(x, wx, wh, bias, act, out, int(out_col))


def _seq_conv_operands(tokens, table, w, pool, rows, rep):
    tokens = _tokens2d(tokens)
    table, w = _f32c(table, "embedding table"), _f32c(w, "conv kernel")
    S, E = table.shape
    if w.dim() != 3 or w.shape[1] != E:
        raise _lib.KgcnHipError("conv kernel %s does not match an embedding width of %d" % (tuple(w.shape), E))
    rep = int(rep)
    if rep < 1 or rows != tokens.shape[0] * rep:
        raise _lib.KgcnHipError("%d rows are not %d copies of %d token rows" % (rows, rep, tokens.shape[0]))
    (C, L), k, F = tokens.shape, w.shape[0], w.shape[2]
    seq_limits_check(L, S, E, k, F, pool)
    return tokens, table, w, rep, (C, L, S, E, k, F, L // int(pool))


def _seq_conv_pool_copies(tokens, table, w, bias, pool, scale, rep, noise, argmax):
    """The one body of seq_conv_pool_scaled (noise None) and seq_conv_pool_perturbed (noise = (sigma, sample, ids, seed))."""
    if noise is None:
        scale = _f32c(scale, "scale").reshape(-1)
        B = scale.numel()
    else:
        C = tokens.shape[0] if torch.is_tensor(tokens) and tokens.dim() == 2 else 0
        scale, sigma, sample, ids, B, seed = _perturb_operands(scale, *noise[:3], lambda b: C, noise[3])
    tokens, table, w, rep, (_, L, S, E, k, F, T) = _seq_conv_operands(tokens, table, w, pool, B, rep)
    b = _conv_bias(bias, F)
    out = torch.empty((B, T, F), device=table.device, dtype=torch.float32)
    arg = torch.empty((B, T, F), device=table.device, dtype=torch.uint8) if argmax else None
    conv = (L, ptr(table), S, E, ptr(w), ptr(b), k, F, int(pool), ptr(out), ptr(arg), current_stream())
    if noise is None:
        check(lib.kgcn_seq_convpool_scaled_fwd_f32(ptr(tokens), B, rep, ptr(scale), *conv), "kgcn_seq_convpool_scaled_fwd_f32")
    else:
        check(lib.kgcn_seq_convpool_perturbed_fwd_f32(ptr(tokens), B, rep, ptr(scale), ptr(sigma), ptr(sample), ptr(ids), seed, *conv),
              "kgcn_seq_convpool_perturbed_fwd_f32")
    return out, arg


def seq_conv_pool_scaled(tokens, table, w, bias, pool, scale, rep, argmax=False):
    """The conv-pool of seq_conv_pool on rep scaled copies of every token row, without autograd (integrated gradients,
    kgcn/feed.py:88-89 add_perturbation on the embedded layer): tokens [C, L] int32, scale [C rep] fp32 -> (pooled [C rep, L // pool, F],
    arg-max bytes of the same shape when argmax=True, else None).  Row b reads token row b // rep and its embedding rows times
    scale[b]; the scaled [C rep, L, E] input is never written."""
    return _seq_conv_pool_copies(tokens, table, w, bias, pool, scale, rep, None, argmax)


# noise streams of the smooth attribution methods
IG_STREAM_FEATURES, IG_STREAM_ADJACENCY, IG_STREAM_SEQUENCE, IG_STREAM_VECTOR = (_lib.K[n] for n in (
    "KGCN_IG_STREAM_FEATURES", "KGCN_IG_STREAM_ADJACENCY", "KGCN_IG_STREAM_SEQUENCE", "KGCN_IG_STREAM_VECTOR"))


def _i32_row(v, name, n, device):
    """ids / sample numbers -> int32 device tensor [n].  The kernels read them as unsigned 32-bit counter words
    (include/kgcn_hip.h): a host sequence is checked to lie in 0 .. 2^31 - 1; a device tensor is passed as it is, without the
    device -> host read a check would need, and a negative entry there is the counter word 2^32 + v."""
    if torch.is_tensor(v) and v.is_cuda:
        if v.dtype != torch.int32:
            raise _lib.KgcnHipError("%s must be int32 on the device" % name)
        t = v.reshape(-1).contiguous()
    else:
        import numpy as np
        a = np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
            raise _lib.KgcnHipError("%s outside 0..2^31-1" % name)
        t = torch.as_tensor(a.astype(np.int32), device=device)
    if t.numel() != n:
        raise _lib.KgcnHipError("%d %s for %d rows" % (t.numel(), name, n))
    return t


def _perturb_operands(scale, sigma, sample, ids, n_ids, seed):
    """scale / sigma [B] fp32, sample [B], ids [n_ids(B)] -> validated device operands; sigma may be a number (every row)."""
    scale = _f32c(scale, "scale").reshape(-1)
    B = scale.numel()
    if not torch.is_tensor(sigma):
        if float(sigma) < 0.0:
            raise _lib.KgcnHipError("noise scale %r is negative" % (sigma,))
        sigma = torch.full((B,), float(sigma), device=scale.device, dtype=torch.float32)
    sigma = _f32c(sigma, "sigma").reshape(-1)
    if sigma.numel() != B:
        raise _lib.KgcnHipError("%d sigmas for %d rows" % (sigma.numel(), B))
    sample = _i32_row(sample, "sample numbers", B, scale.device)
    ids = _i32_row(ids, "ids", n_ids(B), scale.device)
    return scale, sigma, sample, ids, B, int(seed) & (2 ** 64 - 1)


def ig_perturb(x, scale, sigma, sample, ids, rep, stream, seed):
    """rep perturbed copies of every [R, W] array of x [C, R, W] (smooth_grad / smooth_ig, kgcn/feed.py:88-89 add_perturbation
    with the noise drawn on the device): out[b] = x[b // rep] * scale[b] + sigma[b] * z with z the N(0, 1) noise of
    (seed, stream, compound ids[b // rep], sample sample[b]) defined in include/kgcn_hip.h -> [C rep, R, W].  A row with
    sigma[b] == 0 is x * scale[b] exactly.  sigma: a [C rep] tensor or one non-negative number."""
    x = _f32c(x, "x")
    if x.dim() != 3:
        raise _lib.KgcnHipError("x must be [compounds, rows, width], got %s" % (tuple(x.shape),))
    C, R, W = x.shape
    rep = int(rep)
    if rep < 1:
        raise _lib.KgcnHipError("%d copies per compound" % rep)
    scale, sigma, sample, ids, B, seed = _perturb_operands(scale, sigma, sample, ids, lambda b: C, seed)
    if B != C * rep:
        raise _lib.KgcnHipError("%d rows are not %d copies of %d compounds" % (B, rep, C))
    out = torch.empty((B, R, W), device=x.device, dtype=torch.float32)
    check(lib.kgcn_ig_perturb_rows_f32(ptr(x), B, rep, R, W, ptr(scale), ptr(sigma), ptr(sample), ptr(ids), int(stream), seed,
                                       ptr(out), current_stream()), "kgcn_ig_perturb_rows_f32")
    return out


def ig_perturb_values(csr, values, scale, sigma, sample, ids, stream, seed):
    """The same for the stored values [nnz] of one channel of a plain BatchedCSR: entry e of graph b (CSR order) becomes
    values[e] * scale[b] + sigma[b] * z(ids[b], sample[b], column = position of e among graph b's entries); scale, sigma, sample
    and ids are per graph.  -> [nnz]."""
    if csr.row_pad != 0:
        raise _lib.KgcnHipError("ig_perturb_values takes a plain batched CSR (row_pad 0)")
    values = _f32c(values, "values").reshape(-1)
    if values.numel() != csr.nnz:
        raise _lib.KgcnHipError("%d values for %d stored entries" % (values.numel(), csr.nnz))
    scale, sigma, sample, ids, B, seed = _perturb_operands(scale, sigma, sample, ids, lambda b: b, seed)
    if B != csr.num_graphs:
        raise _lib.KgcnHipError("%d scales for %d graphs" % (B, csr.num_graphs))
    out = torch.empty_like(values)
    check(lib.kgcn_ig_perturb_values_f32(ptr(csr.rowptr), csr.num_graphs, csr.rows, csr.nnz, csr.max_nnz, ptr(values), ptr(scale),
                                         ptr(sigma), ptr(sample), ptr(ids), int(stream), seed, ptr(out), current_stream()),
          "kgcn_ig_perturb_values_f32")
    return out


def seq_conv_pool_perturbed(tokens, table, w, bias, pool, scale, rep, sigma, sample, ids, seed, argmax=False):
    """seq_conv_pool_scaled with noise on the embedded input: the window element at position l, column e of row b is
    table[tokens[b // rep, l], e] * scale[b] + sigma[b] * z, z the N(0, 1) noise of (seed, stream IG_STREAM_SEQUENCE, compound
    ids[b // rep], sample sample[b], row l, column e) (include/kgcn_hip.h), drawn inside the window staging: the noisy
    [C rep, L, E] input is never written.  Rows with sigma[b] == 0 are exactly seq_conv_pool_scaled's.  ops.seq_conv_pool_input_grad
    takes the result as it takes the scaled forward's."""
    return _seq_conv_pool_copies(tokens, table, w, bias, pool, scale, rep, (sigma, sample, ids, seed), argmax)


def seq_conv_pool_input_grad(dout, argmax, tokens, table, w, pool, rep, row_weight=None, times_table=False):
    """Gradient with respect to the scaled embedded input of seq_conv_pool_scaled, summed over the rep copies of every token
    row: d pooled [C rep, L // pool, F] and its arg-max bytes -> [C, L, E], the sum in copy order of row_weight[b] (None = 1)
    times the gradient of copy b, times table[tokens] when times_table (the attribution of kgcn/visualization.py:207-215).
    No weight gradient is formed."""
    B = dout.shape[0]
    tokens, table, w, rep, (C, L, S, E, k, F, T) = _seq_conv_operands(tokens, table, w, pool, B, rep)
    dout = _f32c(dout, "grad")
    if tuple(dout.shape) != (B, T, F) or argmax is None or tuple(argmax.shape) != (B, T, F) or argmax.dtype != torch.uint8:
        raise _lib.KgcnHipError("d pooled %s / arg-max bytes do not match [%d, %d, %d]" % (tuple(dout.shape), B, T, F))
    require_gpu(argmax, "arg-max bytes")
    argmax = argmax.contiguous()
    wt = None
    if row_weight is not None:
        wt = _f32c(row_weight, "row weights").reshape(-1)
        if wt.numel() != B:
            raise _lib.KgcnHipError("%d row weights for %d rows" % (wt.numel(), B))
    dx = torch.empty((C, L, E), device=table.device, dtype=torch.float32)
    check(lib.kgcn_seq_convpool_input_grad_f32(ptr(tokens), B, rep, L, ptr(table), S, E, ptr(w), k, F, int(pool), ptr(dout), ptr(argmax),
                                               ptr(wt), 1 if times_table else 0, ptr(dx), current_stream()),
          "kgcn_seq_convpool_input_grad_f32")
    return dx


# -------------------------------------------------------------------------------------------------
# general Conv1D -> MaxPooling1D on the matrix pipe (sample_protein/sequence/cnn.py:36-61; csrc/conv1d.hip)
# -------------------------------------------------------------------------------------------------
CONV1D_MAX_CHANNELS, CONV1D_MAX_KERNEL, CONV1D_MAX_POOL, CONV1D_MAX_LENGTH, CONV1D_MAX_SYMBOLS = (_lib.K[n] for n in (
    "KGCN_CONV1D_MAX_CHANNELS", "KGCN_CONV1D_MAX_KERNEL", "KGCN_CONV1D_MAX_POOL", "KGCN_CONV1D_MAX_LENGTH", "KGCN_CONV1D_MAX_SYMBOLS"))
CONV1D_ACTIVATIONS = (None, "none", "linear", "relu", "tanh")


def conv1d_limits_check(length=None, in_dim=None, filters=None, kernel_size=None, pool=None, symbols=None):
    """Raise KgcnHipError for a Conv1D shape beyond the kernels' limits (include/kgcn_hip.h); None = not checked."""
    for name, v, hi in (("length", length, CONV1D_MAX_LENGTH), ("input width", in_dim, CONV1D_MAX_CHANNELS),
                        ("filters", filters, CONV1D_MAX_CHANNELS), ("kernel size", kernel_size, CONV1D_MAX_KERNEL),
                        ("pool size", pool, CONV1D_MAX_POOL), ("symbols", symbols, CONV1D_MAX_SYMBOLS)):
        if v is not None and not 1 <= int(v) <= hi:
            raise _lib.KgcnHipError("conv1d_pool: %s %d outside 1..%d" % (name, int(v), hi))


class _Conv1DPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, pool, act, tokens, table):
        w = _f32c(w, "conv kernel")
        if w.dim() != 3:
            raise _lib.KgcnHipError("conv kernel must be [kernel_size, in_dim, filters], got %s" % (tuple(w.shape),))
        k, Cin, F = w.shape
        S = 0
        if tokens is not None:
            if x is not None or table is None:
                raise _lib.KgcnHipError("conv1d_pool takes a dense input or a (tokens, table) pair")
            tokens, table = _tokens2d(tokens), _f32c(table, "embedding table")
            if table.dim() != 2 or table.shape[1] != Cin:
                raise _lib.KgcnHipError("embedding table %s does not match a conv kernel %s" % (tuple(table.shape), tuple(w.shape)))
            (B, L), S = tokens.shape, table.shape[0]
        else:
            if x is None or table is not None:
                raise _lib.KgcnHipError("conv1d_pool takes a dense input or a (tokens, table) pair")
            x = _f32c(x, "conv input")
            if x.dim() != 3 or x.shape[2] != Cin:
                raise _lib.KgcnHipError("conv input %s does not match a conv kernel %s" % (tuple(x.shape), tuple(w.shape)))
            B, L = x.shape[:2]
        b = _conv_bias(bias, F)
        conv1d_limits_check(L, Cin, F, k, pool, S if tokens is not None else None)
        T = L // pool
        out = torch.empty((B, T, F), device=w.device, dtype=torch.float32)
        n = ctx.needs_input_grad
        train = n[0] or n[1] or n[2] or n[6]
        arg = torch.empty((B, T, F), device=w.device, dtype=torch.uint8) if train else None
        check(lib.kgcn_conv1d_pool_fwd_f32(ptr(x), ptr(tokens), ptr(table), S, B, L, Cin, ptr(w), ptr(b), k, F, pool, act, ptr(out),
                                           ptr(arg), current_stream()), "kgcn_conv1d_pool_fwd_f32")
        if train:
            ctx.save_for_backward(x, tokens, table, w, arg, out)
            ctx.pool, ctx.act, ctx.bias_shape = pool, act, tuple(bias.shape)
            _record_params(ctx, w, bias, when=n[1] or n[2])
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        n = ctx.needs_input_grad
        if g is None or not (n[0] or n[1] or n[2] or n[6]):
            return (None,) * 7
        x, tokens, table, w, arg, out = ctx.saved_tensors
        k, Cin, F = w.shape
        B, L = (x if tokens is None else tokens).shape[:2]
        S = 0 if tokens is None else table.shape[0]
        g = _f32c(g, "grad")
        dx = torch.empty((B, L, Cin), device=w.device, dtype=torch.float32) if (n[0] or n[6]) else None
        params = n[1] or n[2]
        dw = torch.empty_like(w) if params else None
        db = torch.empty((F,), device=w.device, dtype=torch.float32) if params else None
        wsb = lib.kgcn_conv1d_pool_workspace_bytes(B, L, Cin, k, F, ctx.pool)
        with _param_grad_stage(ctx, wsb, w.device, when=params) as wsp:
            check(lib.kgcn_conv1d_pool_bwd_f32(ptr(x), ptr(tokens), ptr(table), S, B, L, Cin, ptr(w), k, F, ctx.pool, ctx.act, ptr(g),
                                               ptr(arg), ptr(out), ptr(dx), ptr(dw), ptr(db), ptr(wsp), wsb, current_stream()),
                  "kgcn_conv1d_pool_bwd_f32")
        dtable = None
        if n[6]:
            dtable = torch.empty_like(table)
            check(lib.kgcn_embedding_grad_f32(ptr(tokens), B, L, ptr(dx), S, Cin, ptr(dtable), current_stream()),
                  "kgcn_embedding_grad_f32")
        return (dx if n[0] else None, dw if n[1] else None, db.view(ctx.bias_shape) if n[2] else None, None, None, None, dtable)


def conv1d_pool(x, w, bias, pool=1, activation=None, tokens=None, table=None):
    """Keras Conv1D(F, k, padding='same', activation) -> MaxPooling1D(pool) in one pass (pool = 1: no pooling): x [B, L, Cin] (or
    x None and tokens [B, L] int32 with table [S, Cin]: the rows are table[tokens], the embedded tensor is never written),
    w [k, Cin, F], bias [F] -> [B, L // pool, F].  activation: None, 'relu' or 'tanh'.  The backward routes the gradient to the
    lowest-index maximum of each window and forms d x (dense mode) or d table (token mode; kgcn_embedding_grad_f32), d w and d bias
    (deferrable fixed-order partials)."""
    if activation not in CONV1D_ACTIVATIONS:
        raise _lib.KgcnHipError("conv1d_pool: unsupported activation %r (None, 'relu', 'tanh')" % (activation,))
    return _Conv1DPool.apply(x, w, bias, int(pool), act_code(activation), tokens, table)


def embedding_grad(tokens, dembedded, symbols):
    """d table [S, E] = the rows of dembedded [B, L, E] summed by the symbol tokens [B, L] holds there (fixed order, no atomics)."""
    g = _f32c(dembedded, "embedded gradient")
    tokens = _tokens2d(tokens)
    if tuple(tokens.shape) != tuple(g.shape[:2]):
        raise _lib.KgcnHipError("tokens must be an int32 device tensor matching the gradient's [batch, length]")
    conv1d_limits_check(length=g.shape[1], in_dim=g.shape[2], symbols=symbols)
    dtable = torch.empty((int(symbols), g.shape[2]), device=g.device, dtype=torch.float32)
    check(lib.kgcn_embedding_grad_f32(ptr(tokens), g.shape[0], g.shape[1], ptr(g), int(symbols), g.shape[2], ptr(dtable),
                                      current_stream()), "kgcn_embedding_grad_f32")
    return dtable


# -------------------------------------------------------------------------------------------------
# integrated gradients of the protein-sequence CNN, fused over the copies (csrc/convig.hip; include/kgcn_hip.h): the first
# Conv1D -> MaxPooling1D layer of K scaled copies from ONE bias-free pass per protein, and the copies' gradients summed before ONE
# input-gradient pass.  Read-outs: no autograd.
# -------------------------------------------------------------------------------------------------
CONV1D_IG_MAX_COPIES = _lib.K["KGCN_CONV1D_IG_MAX_COPIES"]


def conv1d_ig_scales(alpha):
    """The scales of the copies as a host fp32 array [K], checked before any launch: 1 <= K <= CONV1D_IG_MAX_COPIES, every scale
    finite and >= 0 (the window maximum commutes with a non-negative scale only)."""
    import numpy as np
    a = np.asarray(alpha.detach().cpu().numpy() if torch.is_tensor(alpha) else alpha, np.float32).reshape(-1)
    if not 1 <= a.size <= CONV1D_IG_MAX_COPIES:
        raise ValueError("conv1d_ig: K = %d copies outside 1..%d" % (a.size, CONV1D_IG_MAX_COPIES))
    if not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError("conv1d_ig: every scale must be finite and >= 0, got %s" % (a[~(np.isfinite(a) & (a >= 0))][:4],))
    return a


def _conv1d_ig_rows(t, name, K):
    t = _f32c(t.detach(), name)
    if t.dim() != 3 or t.shape[0] % K:
        raise ValueError("conv1d_ig: %s must be [C K, T, F] with K = %d, got %s" % (name, K, tuple(t.shape)))
    conv1d_limits_check(length=t.shape[1], filters=t.shape[2])
    return t


@torch.no_grad()
def conv1d_pool_window_max(tokens, table, w, pool):
    """Pm [C, L // pool, F], the window maxima of conv(table[tokens], w) WITHOUT bias or activation, and their arg-max bytes
    (the lowest index among equal maxima): kgcn_conv1d_pool_fwd_f32 in token mode with a zero bias and KGCN_ACT_NONE."""
    tokens, table, w = _tokens2d(tokens), _f32c(table.detach(), "embedding table"), _f32c(w.detach(), "conv kernel")
    if w.dim() != 3 or table.dim() != 2 or table.shape[1] != w.shape[1]:
        raise _lib.KgcnHipError("embedding table %s does not match a conv kernel %s" % (tuple(table.shape), tuple(w.shape)))
    (C, L), S, (k, Cin, F) = tokens.shape, table.shape[0], w.shape
    conv1d_limits_check(L, Cin, F, k, pool, S)
    T = L // int(pool)
    Pm = torch.empty((C, T, F), device=w.device, dtype=torch.float32)
    arg = torch.empty((C, T, F), device=w.device, dtype=torch.uint8)
    zero = torch.zeros((F,), device=w.device, dtype=torch.float32)
    check(lib.kgcn_conv1d_pool_fwd_f32(None, ptr(tokens), ptr(table), S, C, L, Cin, ptr(w), ptr(zero), k, F, int(pool), ACT_CODES[None],
                                       ptr(Pm), ptr(arg), current_stream()), "kgcn_conv1d_pool_fwd_f32")
    return Pm, arg


@torch.no_grad()
def conv1d_ig_expand(Pm, alpha, bias):
    """The first Conv1D(relu) -> MaxPooling1D layer of K scaled copies of C proteins from conv1d_pool_window_max's Pm [C, T, F]:
    out[c K + k] = max(0, fl(fl(alpha[k] Pm[c]) + bias)) -> [C K, T, F] (two roundings; at alpha 1 the composed layer bit for
    bit).  alpha [K]: conv1d_ig_scales refuses a negative or non-finite scale before any launch."""
    a = conv1d_ig_scales(alpha)
    require_gpu(Pm, "Pm")
    Pm = _conv1d_ig_rows(Pm, "Pm", 1)
    C, T, F = Pm.shape
    K = int(a.size)
    b = _conv_bias(bias.detach(), F)
    out = torch.empty((C * K, T, F), device=Pm.device, dtype=torch.float32)
    if T:
        al = torch.as_tensor(a, device=Pm.device)
        check(lib.kgcn_ig_conv1d_expand_f32(ptr(Pm), C, K, T, F, ptr(al), ptr(b), ptr(out), current_stream()), "kgcn_ig_conv1d_expand_f32")
    return out


@torch.no_grad()
def conv1d_ig_reduce(dout, out, weights):
    """r [C, T, F] = sum_k weights[k] dout[c K + k] [out[c K + k] > 0] over the K copies of every protein, k ascending from +0 in
    fp32 (product and sum unfused), no atomics; a copy of weight 0 is neither read nor added.  dout, out [C K, T, F]."""
    import numpy as np
    wh = np.asarray(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, np.float32).reshape(-1)
    K = int(wh.size)
    if not 1 <= K <= CONV1D_IG_MAX_COPIES:
        raise ValueError("conv1d_ig: K = %d copies outside 1..%d" % (K, CONV1D_IG_MAX_COPIES))
    require_gpu(out, "out")
    out, dout = _conv1d_ig_rows(out, "out", K), _conv1d_ig_rows(dout, "dout", K)
    if tuple(dout.shape) != tuple(out.shape):
        raise ValueError("conv1d_ig_reduce: dout %s and out %s differ" % (tuple(dout.shape), tuple(out.shape)))
    B, T, F = out.shape
    r = torch.empty((B // K, T, F), device=out.device, dtype=torch.float32)
    if T:
        w = torch.as_tensor(wh, device=out.device)
        check(lib.kgcn_ig_conv1d_reduce_f32(ptr(dout), ptr(out), B // K, K, T, F, ptr(w), ptr(r), current_stream()),
              "kgcn_ig_conv1d_reduce_f32")
    return r


@torch.no_grad()
def conv1d_pool_window_grad(r, arg, Pm, tokens, table, w, pool):
    """d rows [C, L, Cin] of conv1d_pool_window_max for the gradient r [C, T, F] arriving at Pm: r routed through `arg`, then the
    transposed convolution -- ONE kgcn_conv1d_pool_bwd_f32 with KGCN_ACT_NONE, dx only."""
    tokens, table, w = _tokens2d(tokens), _f32c(table.detach(), "embedding table"), _f32c(w.detach(), "conv kernel")
    r, Pm = _f32c(r, "r"), _f32c(Pm, "Pm")
    (C, L), S, (k, Cin, F) = tokens.shape, table.shape[0], w.shape
    conv1d_limits_check(L, Cin, F, k, pool, S)
    shape = (C, L // int(pool), F)
    if tuple(r.shape) != shape or tuple(Pm.shape) != shape or tuple(arg.shape) != shape or arg.dtype != torch.uint8 or not arg.is_contiguous():
        raise _lib.KgcnHipError("conv1d_pool_window_grad: r, Pm and the arg-max bytes must be %s" % (shape,))
    dx = torch.empty((C, L, Cin), device=w.device, dtype=torch.float32)
    wsb = lib.kgcn_conv1d_pool_workspace_bytes(C, L, Cin, k, F, int(pool))
    wsp = _lib.workspace(wsb, w.device)
    check(lib.kgcn_conv1d_pool_bwd_f32(None, ptr(tokens), ptr(table), S, C, L, Cin, ptr(w), k, F, int(pool), ACT_CODES[None], ptr(r),
                                       ptr(arg), ptr(Pm), ptr(dx), None, None, ptr(wsp), wsb, current_stream()),
          "kgcn_conv1d_pool_bwd_f32")
    return dx


class _GatherInto(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, join, join_col):
        y = _f32c(y, "inputs")
        T, N, d = y.shape
        ctx.shape = (T, N, d)
        ctx.set_materialize_grads(False)
        return _readout(y, T, N, d, join, join_col)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        T, N, d = ctx.shape
        if g.dtype != torch.float32 or g.stride(1) != 1 or g.stride(0) < d:
            g = _f32c(g, "grad")
        dx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib.kgcn_graph_gather_bwd_ld_f32(g.data_ptr(), g.stride(0), T, N, d, ptr(dx), current_stream()),
              "kgcn_graph_gather_bwd_ld_f32")
        return dx, None, None


def graph_gather_into(y, join, join_col):
    """GraphGather (sum over nodes) of y [T, N, d] written into columns join_col .. join_col + d of the [T, wide] buffer `join`
    (combine the blocks with join_columns); the backward reads the gradient's column block where it lies, whatever its row
    stride (dense_gather(join=) needs a multiple of 4)."""
    return _GatherInto.apply(y, join, int(join_col))


# -------------------------------------------------------------------------------------------------
# knowledge-graph link prediction (sample_kg/network_prediction/model_py/{gcn,distmult,ip}.py; csrc/linkpred.hip): label-batch
# assembly with the negative draw, the pairwise ranking loss, and its atomic-free gradient
# -------------------------------------------------------------------------------------------------
LINKPRED_MODES = {"gcn": _lib.K["KGCN_LP_GCN"], "distmult": _lib.K["KGCN_LP_DISTMULT"], "ip": _lib.K["KGCN_LP_IP"]}
LINKPRED_MAX_DIM, LINKPRED_MAX_BATCH, LINKPRED_MAX_REL_FLOATS = (_lib.K[n] for n in (
    "KGCN_LP_MAX_DIM", "KGCN_LP_MAX_BATCH", "KGCN_LP_MAX_REL_FLOATS"))


class _LinkPredLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, labels, perm, negatives, batch, mode, seed, step, h, w):
        h = _f32c(h, "node rows")
        N, D = h.shape
        wc = _f32c(w, "relation vectors") if w is not None else None
        R = wc.shape[0] if wc is not None else 0
        L = int(batch)
        rows = torch.empty((L, 6), device=h.device, dtype=torch.int32)
        s1 = torch.empty((L,), device=h.device, dtype=torch.float32)
        s2 = torch.empty((L,), device=h.device, dtype=torch.float32)
        sums = torch.empty((5,), device=h.device, dtype=torch.float32)
        check(lib.kgcn_linkpred_fwd_f32(ptr(h), N, D, ptr(wc), R, mode, ptr(labels), ptr(perm), labels.shape[0], L, ptr(negatives),
                                        negatives.shape[0], int(seed) & (2 ** 64 - 1), ptr(step), ptr(rows), ptr(s1), ptr(s2),
                                        ptr(sums), current_stream()), "kgcn_linkpred_fwd_f32")
        ctx.mode, ctx.L, ctx.has_w = mode, L, wc is not None
        _record_params(ctx, w)
        ctx.save_for_backward(h, wc if wc is not None else h.new_empty(0), rows, s1, s2, sums)
        correct = sums[2]
        ctx.mark_non_differentiable(correct, s1, s2, rows)
        ctx.set_materialize_grads(False)
        return sums[0], sums[1], correct, s1, s2, rows

    @staticmethod
    def backward(ctx, g_opt, g_sum, _g_count, _g_s1, _g_s2, _g_rows):
        h, wc, rows, s1, s2, sums = ctx.saved_tensors
        N, D = h.shape
        g = _grad_scalars(g_opt, g_sum)
        if g is None:
            return (None,) * 9
        go, gs = g
        R = wc.shape[0] if ctx.has_w else 0
        dh = torch.empty_like(h)
        dw = torch.empty_like(wc) if ctx.has_w else None
        wsb = lib.kgcn_linkpred_workspace_bytes(N, D, R, ctx.mode, ctx.L)
        with _param_grad_stage(ctx, wsb, h.device) as wsp:
            check(lib.kgcn_linkpred_bwd_f32(ptr(h), N, D, ptr(wc) if ctx.has_w else None, R, ctx.mode, ptr(rows), ptr(s1), ptr(s2),
                                            ptr(sums), ctx.L, ptr(go), ptr(gs), ptr(dh), ptr(dw), ptr(wsp), wsb, current_stream()),
                  "kgcn_linkpred_bwd_f32")
        return None, None, None, None, None, None, None, dh, dw


def linkpred_loss(h, feed, mode, w=None, seed=0, step=None, batch=None, labels=None, perm=None, negatives=None):
    """model_py/{gcn,distmult,ip}.py from the gathers to the metrics -> (cost_opt, cost_sum, correct_count, s1 [L], s2 [L],
    rows [L, 6] int32).  h [N, D] the node rows (the embedding table, or the GraphConv output), w [R, D] the DistMult relation
    vectors (mode 'distmult' only).  The batch comes from `feed` (data_util.LinkPredFeed: the device-resident label list, the row
    permutation of the epoch and the negative table; keyword overrides for tests): window (*step mod floor(M / L)) of the
    permuted list, col 3 := col 0, col 5 := a negative drawn on the device from (seed, *step, row).  rows are the assembled batch;
    for 'ip' s1 / s2 are the per-row terms of the batch-wide sums the cost is taken on (ip.py:46-47).  Differentiable in h and w
    through cost_opt and cost_sum; correct_count, s1, s2 and rows are metrics."""
    if mode not in LINKPRED_MODES:
        raise _lib.KgcnHipError("linkpred_loss: mode must be one of %s" % sorted(LINKPRED_MODES))
    code = LINKPRED_MODES[mode]
    if h.dim() != 2 or not 1 <= h.shape[1] <= LINKPRED_MAX_DIM:
        raise _lib.KgcnHipError("linkpred_loss: node rows must be [N, D <= %d], got %s" % (LINKPRED_MAX_DIM, tuple(h.shape)))
    if (mode == "distmult") != (w is not None):
        raise _lib.KgcnHipError("linkpred_loss: relation vectors are required by 'distmult' and only by it")
    if w is not None and (w.dim() != 2 or w.shape[1] != h.shape[1] or w.numel() > LINKPRED_MAX_REL_FLOATS):
        raise _lib.KgcnHipError("linkpred_loss: relation vectors must be [R, %d] with R D <= %d" % (h.shape[1], LINKPRED_MAX_REL_FLOATS))
    if labels is None:
        # the kernels read the ids unchecked: the feed's host-side bounds against these node rows / relation vectors
        if feed.max_node >= h.shape[0] or (w is not None and feed.max_relation >= w.shape[0]):
            raise _lib.KgcnHipError("linkpred_loss: the label list names node %d / relation %d, beyond %d node rows / %s relations"
                                    % (feed.max_node, feed.max_relation, h.shape[0], "-" if w is None else w.shape[0]))
    labels = feed.labels if labels is None else labels
    perm = (feed.perm if feed is not None else None) if perm is None else perm
    negatives = feed.negatives if negatives is None else negatives
    batch = feed.batch if batch is None else int(batch)
    for t, name in ((labels, "label list"), (negatives, "negative table")) + (((perm, "permutation"),) if perm is not None else ()):
        require_gpu(t, name)
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.KgcnHipError("linkpred_loss: the %s must be a contiguous int32 device tensor" % name)
    if labels.dim() != 2 or labels.shape[1] != 6 or not 1 <= batch <= min(labels.shape[0], LINKPRED_MAX_BATCH):
        raise _lib.KgcnHipError("linkpred_loss: label list %s cannot feed batches of %d rows" % (tuple(labels.shape), batch))
    if perm is not None and perm.shape != (labels.shape[0],):
        raise _lib.KgcnHipError("linkpred_loss: the permutation must have one entry per label row")
    return _LinkPredLoss.apply(labels, perm, negatives, batch, code, seed, _step_ptr(step), h, w)


# -------------------------------------------------------------------------------------------------
# integrated gradients of the link-prediction model (kgcn visualize on model_py/gcn.py; csrc/kgig.hip): many targets over
# one graph, from the stash of the K scaled layer-2 outputs
# -------------------------------------------------------------------------------------------------
KG_IG_MODES = {"score": _lib.K["KGCN_KGIG_SCORE"], "loss": _lib.K["KGCN_KGIG_LOSS"]}
KG_IG_WIDTH, KG_IG_MAX_NODES, KG_IG_MAX_STEPS, KG_IG_GROUPS = (_lib.K[n] for n in (
    "KGCN_KGIG_WIDTH", "KGCN_KGIG_MAX_NODES", "KGCN_KGIG_MAX_STEPS", "KGCN_KGIG_GROUPS"))


def kg_ig_check_host(indptr, indices, num_nodes, targets=None, mode="score", steps=1, width=KG_IG_WIDTH):
    """Everything the kernel reads unchecked, on host (numpy) copies: raises ValueError, returns the targets as int32 [T, 4]
    (None when none were given).  The CSR must have monotone row offsets and, in every row, strictly increasing columns inside
    [0, N) -- sorted and duplicate-free: the scatter spreads a row's entries over lanes and relies on their being distinct."""
    import numpy as np
    N = int(num_nodes)
    if mode not in KG_IG_MODES:
        raise ValueError("kg_ig: mode must be one of %s, got %r" % (sorted(KG_IG_MODES), mode))
    if int(width) != KG_IG_WIDTH:
        raise ValueError("kg_ig: the layers must be %d wide (model_py/gcn.py), got %d" % (KG_IG_WIDTH, int(width)))
    if not 1 <= N <= KG_IG_MAX_NODES:
        raise ValueError("kg_ig: %d nodes outside 1..%d (the target's row lives in LDS)" % (N, KG_IG_MAX_NODES))
    if not 1 <= int(steps) <= KG_IG_MAX_STEPS:
        raise ValueError("kg_ig: %d steps outside 1..%d" % (int(steps), KG_IG_MAX_STEPS))
    indptr = np.asarray(indptr).astype(np.int64).reshape(-1)
    indices = np.asarray(indices).astype(np.int64).reshape(-1)
    if indptr.shape[0] != N + 1 or indptr[0] != 0 or indptr[-1] != indices.shape[0] or np.any(np.diff(indptr) < 0):
        raise ValueError("kg_ig: the row offsets must rise from 0 to nnz = %d over %d rows" % (indices.shape[0], N))
    if indices.size:
        if indices.min() < 0 or indices.max() >= N:
            raise ValueError("kg_ig: adjacency column outside [0, %d)" % N)
        inside = np.ones(indices.shape[0], bool)
        inside[indptr[:-1][indptr[:-1] < indices.shape[0]]] = False            # the first entry of every non-empty row
        if np.any((np.diff(indices, prepend=-1) <= 0) & inside):
            raise ValueError("kg_ig: every adjacency row must hold sorted, duplicate-free columns")
    if targets is None:
        return None
    tg = np.asarray(targets)
    if tg.ndim != 2 or tg.shape[1] != 4 or not np.issubdtype(tg.dtype, np.integer):
        raise ValueError("kg_ig: targets must be an integer [T, 4] array of (a, b, a', b'), got %s %s" % (tg.shape, tg.dtype))
    used = tg if mode == "loss" else tg[:, :2]
    if used.size and (used.min() < 0 or used.max() >= N):
        raise ValueError("kg_ig: target node outside [0, %d)" % N)
    return np.ascontiguousarray(tg, np.int32)


def kg_ig(csr, g1, rowsum, b1, w2, h2, p, scales, weights, targets, mode="score", want_u=False, groups=None):
    """csrc/kgig.hip: integrated gradients of T targets of the link-prediction gcn from the stash -> (node_ig [T, N], score [T, K],
    u [T, N, C] or None).  csr: the one graph (a BatchedCSR of one graph); g1 = A (E W1), rowsum = A 1, p = E W1, h2 [K, N, C] the
    layer-2 outputs at scales [K] (formed from fp32 scales[k] * g1 + rowsum[:, None] * b1), weights [K] the step weights;
    targets: host integer [T, 4] rows (a, b, a', b'), mode 'score' (a, b only) or 'loss'.  groups: workgroups of the launch
    (default KG_IG_GROUPS; each walks whole targets in a grid-stride loop).  A read-out: no autograd, runs under no_grad.
    The CSR and the targets are validated on the host (kg_ig_check_host), once per container."""
    import numpy as np
    if csr.num_graphs != 1 or csr.rows != csr.cols or csr.row_pad:
        raise ValueError("kg_ig: the adjacency must be one square graph in the plain CSR layout")
    N = csr.rows
    h2 = _f32c(h2, "h2")
    if h2.dim() != 3 or h2.shape[1] != N:
        raise ValueError("kg_ig: h2 must be [K, %d, C], got %s" % (N, tuple(h2.shape)))
    K, _, C = h2.shape
    host = getattr(csr, "_kg_ig_host", None)
    if host is None:
        host = (csr.rowptr.cpu().numpy(), csr.cv[:, 0].cpu().numpy())
        kg_ig_check_host(host[0], host[1], N, None, mode, K, C)
        csr._kg_ig_host = host
        csr._kg_ig_dev = (csr.cv[:, 0].contiguous(), csr.values)
    tg = kg_ig_check_host(host[0], host[1], N, targets.cpu().numpy() if torch.is_tensor(targets) else targets, mode, K, C)
    indices, values = csr._kg_ig_dev
    dev = h2.device
    with torch.no_grad():
        g1, p, w2 = _f32c(g1.detach(), "g1"), _f32c(p.detach(), "p"), _f32c(w2.detach(), "w2")
        rowsum, b1 = _f32c(rowsum.detach(), "rowsum").reshape(-1), _f32c(b1.detach(), "b1").reshape(-1)
        sc = torch.as_tensor(np.asarray(scales, np.float32), device=dev) if not torch.is_tensor(scales) else _f32c(scales, "scales")
        wt = torch.as_tensor(np.asarray(weights, np.float32), device=dev) if not torch.is_tensor(weights) else _f32c(weights, "weights")
        if tuple(g1.shape) != (N, C) or tuple(p.shape) != (N, C) or tuple(w2.shape) != (C, C) or rowsum.numel() != N or \
                b1.numel() != C or sc.numel() != K or wt.numel() != K:
            raise ValueError("kg_ig: operand shapes disagree with N = %d, C = %d, K = %d" % (N, C, K))
        T = tg.shape[0]
        tgd = torch.from_numpy(tg).to(dev)
        node_ig = torch.empty((T, N), device=dev, dtype=torch.float32)
        score = torch.empty((T, K), device=dev, dtype=torch.float32)
        u = torch.zeros((T, N, C), device=dev, dtype=torch.float32) if want_u else None
        g = KG_IG_GROUPS if groups is None else int(groups)
        if not 1 <= g <= 65535:
            raise ValueError("kg_ig: %d workgroups" % g)
        check(lib.kgcn_kg_ig_f32(ptr(csr.rowptr), ptr(indices), ptr(values), csr.nnz, N, C, ptr(g1), ptr(rowsum), ptr(b1), ptr(w2),
                                 ptr(h2), ptr(p), ptr(sc), ptr(wt), K, ptr(tgd), T, KG_IG_MODES[mode], g, ptr(node_ig), ptr(score),
                                 ptr(u), current_stream()), "kgcn_kg_ig_f32")
    return node_ig, score, u


# -------------------------------------------------------------------------------------------------
# ranking of all node pairs of the link-prediction model (run_enrichment.sh: script/predscore.py; csrc/pairrank.hip): the
# score-ordered pair list straight from the node rows, and its train / test / new marks with the enrichment counts
# -------------------------------------------------------------------------------------------------
PAIRRANK_MAX_NODES, PAIRRANK_MAX_CANDIDATES, PAIRRANK_MAX_TOP = (_lib.K[n] for n in (
    "KGCN_PAIRRANK_MAX_NODES", "KGCN_PAIRRANK_MAX_CANDIDATES", "KGCN_PAIRRANK_MAX_TOP"))


def _pair_rank_ws(n, d, capacity, entries, device):
    nbytes = lib.kgcn_pair_rank_workspace_bytes(n, d, capacity, entries)
    if nbytes < 0:
        check(1, "kgcn_pair_rank_workspace_bytes")
    return _lib.workspace(nbytes, device, torch.uint8), nbytes


@torch.no_grad()
def pair_rank(h, w=None, cutoff=10000):
    """The first `cutoff` entries (0, or more than there are: all N (N - 1) / 2) of the list of node pairs i < j ordered as
    predscore.py:153 orders its (score, row, col) tuples -- score, then row, then col, all descending -> (score [K] float32,
    row [K] int32, col [K] int32) device tensors.  The score is s_ij = sum_k (h[i,k] w[k]) h[j,k] in fp32 on the f32 MFMA, k
    ascending (w: one relation's DistMult vector [D], None for gcn / ip); -0.0 ranks as +0.0 and NaN below every number.
    The [N, N] matrix is never formed: a radix select finds the key of the cutoff-th score, its three counts are read (the
    one synchronisation besides the end of the call: not for hipGraph capture), and the pairs at or above it are gathered,
    sorted and cut.  A read-out: no autograd.  Bitwise reproducible."""
    h = _f32c(h.detach(), "node rows")
    if h.dim() != 2 or not 2 <= h.shape[0] <= PAIRRANK_MAX_NODES or not 1 <= h.shape[1] <= LINKPRED_MAX_DIM:
        raise _lib.KgcnHipError("pair_rank: node rows must be [2 <= N <= %d, 1 <= D <= %d], got %s"
                                % (PAIRRANK_MAX_NODES, LINKPRED_MAX_DIM, tuple(h.shape)))
    N, D = h.shape
    cutoff = int(cutoff)
    if cutoff < 0:
        raise _lib.KgcnHipError("pair_rank: negative cutoff %d" % cutoff)
    wc = None
    if w is not None:
        wc = _f32c(w.detach(), "relation vector").reshape(-1)
        if wc.numel() != D:
            raise _lib.KgcnHipError("pair_rank: the relation vector must have %d entries, got %s" % (D, tuple(w.shape)))
    total = N * (N - 1) // 2
    k = total if cutoff == 0 or cutoff > total else cutoff
    counts = torch.empty((3,), device=h.device, dtype=torch.int64)
    ws, wsb = _pair_rank_ws(N, D, 0, 0, h.device)
    check(lib.kgcn_pair_rank_select_f32(ptr(h), N, D, ptr(wc), cutoff, ptr(counts), ptr(ws), wsb, current_stream()),
          "kgcn_pair_rank_select_f32")
    _, above, equal = counts.tolist()
    capacity = above + equal
    if not k <= capacity <= total:
        raise _lib.KgcnHipError("pair_rank: the select counted %d + %d candidates for %d of %d entries" % (above, equal, k, total))
    if capacity > PAIRRANK_MAX_CANDIDATES:
        raise _lib.KgcnHipError("pair_rank: %d pairs score at or above the cutoff's (%d of them tie at it), more than the %d "
                                "candidates one call sorts: lower the cutoff" % (capacity, equal, PAIRRANK_MAX_CANDIDATES))
    ws, wsb = _pair_rank_ws(N, D, capacity, 0, h.device)
    score = torch.empty((k,), device=h.device, dtype=torch.float32)
    row = torch.empty((k,), device=h.device, dtype=torch.int32)
    col = torch.empty((k,), device=h.device, dtype=torch.int32)
    check(lib.kgcn_pair_rank_emit_f32(ptr(h), N, D, ptr(wc), cutoff, ptr(counts), capacity, ptr(score), ptr(row), ptr(col), ptr(ws),
                                      wsb, current_stream()), "kgcn_pair_rank_emit_f32")
    return score, row, col


def pair_codes(pairs, device):
    """Host pairs (row < col) -> the sorted, duplicate-free uint32 codes row << 16 | col the table kernel searches, as an
    int32-typed device tensor of those bits."""
    import numpy as np
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if p.size and (p.min() < 0 or p.max() >= PAIRRANK_MAX_NODES or np.any(p[:, 0] >= p[:, 1])):
        raise ValueError("pair_codes: pairs must be (row, col) with 0 <= row < col < %d" % PAIRRANK_MAX_NODES)
    codes = np.unique((p[:, 0] << 16) | p[:, 1]).astype(np.uint32)
    return torch.from_numpy(codes.view(np.int32)).to(device)


@torch.no_grad()
def pair_rank_table(score, row, col, target_codes, test_codes, top_ratio):
    """convert / process_table / enrichment of predscore.py:194-280 on a sorted list (pair_rank's output) -> (train_edge,
    test_edge, new_edge [K] uint8, score_ranking [K] int64, hits [P] int64, covered [P] int64).  target_codes (train + test)
    and test_codes: pair_codes tensors.  train = in target and not in test, test = in test, new = neither; score_ranking =
    1 + the entries with a larger score (len - rankdata(max) + 1); hits[p] = test entries among the first top_ratio[p]
    entries that are no train edge; covered[p] = the list holds that many such entries.  P <= 16 host integers."""
    score = _f32c(score, "score")
    K = score.numel()
    top = [int(t) for t in top_ratio]
    if K < 1 or K > PAIRRANK_MAX_CANDIDATES or len(top) > PAIRRANK_MAX_TOP or any(t < 0 for t in top):
        raise _lib.KgcnHipError("pair_rank_table: %d entries, %d thresholds (up to %d entries, %d thresholds >= 0)"
                                % (K, len(top), PAIRRANK_MAX_CANDIDATES, PAIRRANK_MAX_TOP))
    for t, name in ((row, "row"), (col, "col"), (target_codes, "target codes"), (test_codes, "test codes")):
        require_gpu(t, name)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1:
            raise _lib.KgcnHipError("pair_rank_table: %s must be a contiguous 1-D int32 device tensor" % name)
    if row.numel() != K or col.numel() != K:
        raise _lib.KgcnHipError("pair_rank_table: score, row and col must have one length")
    dev = score.device
    flags = torch.empty((3, K), device=dev, dtype=torch.uint8)
    ranking = torch.empty((K,), device=dev, dtype=torch.int64)
    hits = torch.zeros((len(top),), device=dev, dtype=torch.int64)
    covered = torch.zeros((len(top),), device=dev, dtype=torch.int64)
    ws, wsb = _pair_rank_ws(2, 1, 0, K, dev)
    tops = (ctypes.c_int64 * max(len(top), 1))(*top)
    check(lib.kgcn_pair_rank_table_i32(ptr(score), ptr(row), ptr(col), K, ptr(target_codes) if target_codes.numel() else None,
                                       target_codes.numel(), ptr(test_codes) if test_codes.numel() else None, test_codes.numel(),
                                       tops, len(top), ptr(flags[0]), ptr(flags[1]), ptr(flags[2]), ptr(ranking),
                                       ptr(hits) if top else None, ptr(covered) if top else None, ptr(ws), wsb, current_stream()),
          "kgcn_pair_rank_table_i32")
    return flags[0], flags[1], flags[2], ranking, hits, covered


# -------------------------------------------------------------------------------------------------
# k-fold cross-validation of the compound-protein interaction networks (gcn.py train_cv): the loss head of
# sample_chem/compound-protein_interaction/multitask.py (csrc/cvloss.hip) and the ranking metrics of compute_metrics
# (gcn.py:170-256; csrc/cvmetrics.hip)
# -------------------------------------------------------------------------------------------------
class _MultitaskSoftmax2CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mask_label, accum):
        x = _f32c(logits, "logits")
        z = _f32c(labels, "labels")
        ml = _f32c(mask_label, "mask_label")
        if z.dim() != 2 or z.shape != ml.shape or x.shape[0] != z.shape[0] or x.numel() != 2 * z.numel():
            raise _lib.KgcnHipError("multitask_softmax2_ce: logits %s must be [B, 2, T] (or [B, 2 T]) for labels %s and mask_label %s"
                                    % (tuple(x.shape), tuple(z.shape), tuple(ml.shape)))
        B, T = z.shape
        _accum_block(accum, 3 * T + 1, "multitask_softmax2_ce", "3 T + 1")
        dlog = torch.empty_like(x)
        pred = torch.empty((B, T), device=x.device, dtype=torch.float32)
        stats = torch.empty((3 * T + 1,), device=x.device, dtype=torch.float32)
        check(lib.kgcn_multitask_softmax2_ce_f32(ptr(x), ptr(z), ptr(ml), B, T, ptr(dlog), ptr(pred), ptr(stats), ptr(accum),
                                                 current_stream()), "kgcn_multitask_softmax2_ce_f32")
        ctx.save_for_backward(dlog)
        ctx.set_materialize_grads(False)
        each = stats[:3 * T]
        ctx.mark_non_differentiable(each, pred)
        return stats[3 * T], each, pred

    @staticmethod
    def backward(ctx, g, g_each, g_pred):
        (dlog,) = ctx.saved_tensors
        return _loss_grad(dlog, None, g, 1), None, None, None


def multitask_softmax2_ce(logits, labels, mask_label, accum=None):
    """compute_metrics of sample_chem/compound-protein_interaction/multitask.py:53-86 in one HIP pass -> (cost, each_cost [T],
    each_correct_count [T], each_count [T], prediction [B, T]).  logits [B, 2, T] (or the Dense output [B, 2 T] it is a view
    of), labels and mask_label [B, T] float32; each_cost[t] sums the two-class sparse softmax cross entropy over the rows with
    mask_label != 0, cost = sum_t each_cost[t] (cost_opt and cost_sum of the model alike), a tie of the two logits predicts
    class 0, prediction = softmax(logits, axis=1)[:, 1, :] for every row.  accum: a float32 device block [3 T + 1] =
    each_cost | each_correct_count | each_count | cost that the call adds its values to in place (an epoch's sums with one
    read-back).  Only cost is differentiable."""
    cost, each, pred = _MultitaskSoftmax2CE.apply(logits, labels, mask_label, accum)
    T = labels.shape[1]
    return cost, each[:T], each[T:2 * T], each[2 * T:], pred


BINARY_METRICS_COLUMNS = ("n_used", "P", "TP", "FP", "n_nonfinite", "auc_num2", "n_groups", "spare")
BINARY_METRICS_MAX_ELEMENTS, BINARY_METRICS_MAX_TASKS = _lib.K["KGCN_BINARY_METRICS_MAX_ELEMENTS"], _lib.K["KGCN_BINARY_METRICS_MAX_TASKS"]


@torch.no_grad()
def binary_metrics(score, label, mask=None, threshold=0.5):
    """The sums behind compute_metrics (gcn.py:170-256) for every task at once -> (counts [T, 8] int64 numpy array with the
    columns BINARY_METRICS_COLUMNS, ap [T] float64 numpy array).  score [n, T] float32 (rows may be strided), label [n, T],
    mask None (every row counts, as the reference) or [n, T] (a row counts where mask != 0).  TP / FP count score > threshold;
    auc_num2 / (2 P N) is roc_curve + auc, ap is average_precision_score (kgcn_amd.cv.metrics_from_counts derives every
    metric).  One radix sort of all tasks' keys and one scan per task on the device; all integers exact, two runs agree bit
    for bit.  Raises ValueError when a counted score is NaN or infinite (as scikit-learn's input check)."""
    require_gpu(score, "score")
    if score.dtype != torch.float32 or score.dim() != 2 or score.shape[0] < 1 or score.shape[1] < 1:
        raise _lib.KgcnHipError("binary_metrics: score must be a float32 [n >= 1, T >= 1] tensor, got %s %s" % (score.dtype, tuple(score.shape)))
    if score.stride(1) != 1 or score.stride(0) < score.shape[1]:
        score = score.contiguous()
    n, T = score.shape
    if n * T > BINARY_METRICS_MAX_ELEMENTS or T > BINARY_METRICS_MAX_TASKS:
        raise _lib.KgcnHipError("binary_metrics: %d x %d elements (at most 2^31, %d tasks)" % (n, T, BINARY_METRICS_MAX_TASKS))
    lab = _f32c(label.to(torch.float32), "label")
    mk = None if mask is None else _f32c(mask.to(torch.float32), "mask")
    if tuple(lab.shape) != (n, T) or (mk is not None and tuple(mk.shape) != (n, T)):
        raise _lib.KgcnHipError("binary_metrics: label / mask do not match score %s" % ((n, T),))
    counts = torch.empty((T, 8), device=score.device, dtype=torch.int64)
    ap = torch.empty((T,), device=score.device, dtype=torch.float64)
    wsb = lib.kgcn_binary_metrics_workspace_bytes(n, T)
    if wsb < 0:
        check(1, "kgcn_binary_metrics_workspace_bytes")
    ws = _lib.workspace(wsb, score.device, torch.uint8)
    check(lib.kgcn_binary_metrics_f32(ptr(score), score.stride(0), ptr(lab), ptr(mk), n, T, float(threshold), ptr(counts), ptr(ap),
                                      ptr(ws), wsb, current_stream()), "kgcn_binary_metrics_f32")
    counts, ap = counts.cpu().numpy(), ap.cpu().numpy()
    if counts[:, 4].any():
        raise ValueError("binary_metrics: %d scores are NaN or infinite (tasks %s)"
                         % (int(counts[:, 4].sum()), [int(t) for t in counts[:, 4].nonzero()[0]]))
    return counts, ap


# -------------------------------------------------------------------------------------------------
# vector-modality models and regression (example_model/model_multimodal_vec.py, model_multimodal_regression.py): the
# Dense + BatchNormalization + activation layer of the vector towers at short batches (csrc/shortm.hip) and the regression
# head (csrc/regress.hip)
# -------------------------------------------------------------------------------------------------
# The short-batch kernels take a Dense(+BN)(+activation) layer of at most short_dense_max_rows rows when short_dense_fusion is
# on; everything else -- and every shape kgcn_dense_bn_short_supported refuses -- runs dense -> graph_bn.  Both values follow
# tools/vecmodal_bench.py (profiles/vecmodal_bench.json; DESIGN.md, "Vector-modality models and regression"): OFF by default.
# On the MI355X the short route was ahead at one of the fifteen measured (rows, K, N) -- 50 x 114 -> 52, by 10 % -- and behind
# at the other fourteen (by 7 % to 6x, growing with rows and K), and the whole captured step of both models was 10 % slower
# with it at 50 rows and up to 3x at 256.  The row limit is the kernels' own: no measured row count favours the route.
short_dense_fusion = False
short_dense_max_rows = _lib.K["KGCN_DENSE_BN_SHORT_MAX_ROWS"]


def dense_bn_short_supported(rows, k, n):
    """Whether csrc/shortm.hip takes a [rows, k] x [k, n] layer (host query, no launch)."""
    return bool(lib.kgcn_dense_bn_short_supported(int(rows), int(k), int(n)))


def dense_bn_route(rows, k, n):
    """-> 'short' (the fused short-batch kernels) or 'composed' (dense -> graph_bn): the one place that decides."""
    if short_dense_fusion and rows <= short_dense_max_rows and dense_bn_short_supported(rows, k, n):
        return "short"
    return "composed"


def _row_strided(t, width, name):
    """A float32 device matrix whose rows may be strided (a column block of a wider buffer) as it lies, anything else contiguous."""
    require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise _lib.KgcnHipError("%s must be a float32 matrix, got %s %s" % (name, t.dtype, tuple(t.shape)))
    if t.stride(1) != 1 or t.stride(0) < width:
        t = t.contiguous()
    return t


def _column_block(out, out_col, rows, n, device):
    """-> (buffer, the [rows, n] view at column out_col): a fresh [rows, n] tensor when out is None."""
    if out is None:
        out = torch.empty((rows, n), device=device, dtype=torch.float32)
        return out, out
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or not out.is_contiguous() or not out.is_cuda or \
            out_col < 0 or out_col + n > out.shape[1]:
        raise _lib.KgcnHipError("output buffer %s does not take [%d, %d] at column %d" % (tuple(out.shape), rows, n, out_col))
    return out, out[:, out_col:out_col + n]


class _DenseBNShort(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, mean, var, eps, act, out, out_col):
        w = _f32c(w, "w")
        K, N = w.shape
        x = _row_strided(x, K, "x")
        B = x.shape[0]
        if x.shape[1] != K:
            raise _lib.KgcnHipError("dense_bn: x %s does not match the kernel %s" % (tuple(x.shape), tuple(w.shape)))
        vecs = [None if v is None else _f32c(v, "vector").reshape(-1) for v in (bias, gamma, beta, mean, var)]
        if any(v is not None and v.numel() != N for v in vecs):
            raise _lib.KgcnHipError("dense_bn: bias / gamma / beta / moving statistics must hold %d values" % N)
        b, ga, be, mu, va = vecs
        out, y = _column_block(out, out_col, B, N, x.device)
        train = any(ctx.needs_input_grad[:5])
        pre = torch.empty((B, N), device=x.device, dtype=torch.float32) if train and ga is not None else None
        check(lib.kgcn_dense_bn_short_fwd_f32(x.data_ptr(), x.stride(0), B, K, ptr(w), ptr(b), N, ptr(ga), ptr(be), ptr(mu), ptr(va),
                                              float(eps), int(act), y.data_ptr(), y.stride(0), ptr(pre), current_stream()),
              "kgcn_dense_bn_short_fwd_f32")
        if train:
            ctx.save_for_backward(x, w, ga, mu, va, y, pre)
            ctx.eps, ctx.act = float(eps), int(act)
            ctx.vec_shapes = [None if v is None else tuple(v.shape) for v in (bias, gamma, beta)]
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        n = ctx.needs_input_grad
        if g is None or not any(n[:5]):
            return (None,) * 11
        x, w, ga, mu, va, y, pre = ctx.saved_tensors
        B, K = x.shape
        N = w.shape[1]
        g = _row_strided(g, N, "grad")
        new = lambda *shape: torch.empty(shape, device=x.device, dtype=torch.float32)
        dw = new(K, N) if n[1] else None
        db = new(N) if n[2] else None
        dga = new(N) if n[3] else None
        dbe = new(N) if n[4] else None
        dpre = new(B, N) if n[0] else None
        check(lib.kgcn_dense_bn_short_bwd_f32(x.data_ptr(), x.stride(0), B, K, N, y.data_ptr(), y.stride(0), g.data_ptr(), g.stride(0),
                                              ptr(pre), ptr(ga), ptr(mu), ptr(va), ctx.eps, ctx.act, ptr(dw), ptr(db), ptr(dga),
                                              ptr(dbe), ptr(dpre), current_stream()), "kgcn_dense_bn_short_bwd_f32")
        dx = None
        if n[0]:
            dx = new(B, K)
            check(lib.kgcn_dense_bn_short_dx_f32(ptr(dpre), B, N, ptr(w), K, ptr(dx), K, current_stream()), "kgcn_dense_bn_short_dx_f32")
        sb, sg, se = ctx.vec_shapes
        return (dx, dw, None if db is None else db.view(sb), None if dga is None else dga.view(sg),
                None if dbe is None else dbe.view(se), None, None, None, None, None, None)


class _ActInto(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, out, out_col):
        x = _row_strided(x, x.shape[1] if x.dim() == 2 else 0, "inputs")
        B, N = x.shape
        out, y = _column_block(out, out_col, B, N, x.device)
        check(lib.kgcn_act_cols_fwd_f32(x.data_ptr(), x.stride(0), B, N, int(act), y.data_ptr(), y.stride(0), current_stream()),
              "kgcn_act_cols_fwd_f32")
        ctx.save_for_backward(y)
        ctx.act = int(act)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        (y,) = ctx.saved_tensors
        B, N = y.shape
        g = _row_strided(g, N, "grad")
        dx = torch.empty((B, N), device=y.device, dtype=torch.float32)
        check(lib.kgcn_act_cols_bwd_f32(y.data_ptr(), y.stride(0), g.data_ptr(), g.stride(0), B, N, ctx.act, ptr(dx), N,
                                        current_stream()), "kgcn_act_cols_bwd_f32")
        return dx, None, None, None


def activation_into(x, activation, out=None, out_col=0):
    """act(x) of a [B, N] matrix (rows may be strided) written into columns out_col .. out_col + N of the contiguous [B, wide]
    buffer `out` and returned as that view (a block of a concatenation, join_columns): one launch each way, and the backward
    reads the gradient's column block where it lies."""
    return _ActInto.apply(x, act_code(activation), out, int(out_col))


def dense_bn(x, w, b, gamma=None, beta=None, moving_mean=None, moving_variance=None, eps=1e-3, activation=None, out=None, out_col=0):
    """K.layers.Dense -> K.layers.BatchNormalization (learning phase 0: the moving statistics are constants, quirk Q6) ->
    activation on x [B, K] (rows may be strided):  y = act(gamma (x w + b - moving_mean) / sqrt(moving_variance + eps) + beta);
    gamma None (then beta and the statistics None too): y = act(x w + b).  out / out_col: y is written into columns out_col ..
    out_col + N of the contiguous [B, wide] buffer `out` and returned as that view; the other columns are not touched.
    Route (dense_bn_route): the short-batch kernels of csrc/shortm.hip -- one launch forward, one for dW / db / dgamma / dbeta,
    one more for dX when x requires grad -- or dense -> graph_bn on a [B, 1, N] view.  Same function either way."""
    act = act_code(activation)
    if (gamma is None) != (beta is None) or (gamma is None) != (moving_mean is None) or (gamma is None) != (moving_variance is None):
        raise _lib.KgcnHipError("dense_bn: gamma, beta, moving_mean and moving_variance come together or not at all")
    if x.dim() != 2 or w.dim() != 2:
        raise _lib.KgcnHipError("dense_bn: x [B, K] and w [K, N] are matrices, got %s and %s" % (tuple(x.shape), tuple(w.shape)))
    B, (K, N) = x.shape[0], w.shape
    if dense_bn_route(B, K, N) == "short":
        return _DenseBNShort.apply(x, w, b, gamma, beta, moving_mean, moving_variance, float(eps), act, out, int(out_col))
    if gamma is None:
        y = dense(x, w, b, activation=activation)
    else:
        y = graph_bn(dense(x, w, b).reshape(B, 1, N), gamma, beta, moving_mean, moving_variance, None, eps, False, activation).reshape(B, N)
    return y if out is None else activation_into(y, None, out, out_col)


class _MaskedSqErr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, labels, mask_label, accum):
        p = _f32c(pred, "pred")
        z = _f32c(labels.to(torch.float32), "labels")
        ml = _f32c(mask_label.to(torch.float32), "mask_label")
        if p.dim() != 2 or z.shape != p.shape or ml.shape != p.shape:
            raise _lib.KgcnHipError("masked_squared_error: pred %s, labels %s and mask_label %s must be one [B, T] shape"
                                    % (tuple(p.shape), tuple(z.shape), tuple(ml.shape)))
        B, T = p.shape
        _accum_block(accum, 2 * T + 1, "masked_squared_error", "2 T + 1")
        dpred = torch.empty_like(p)
        stats = torch.empty((2 * T + 2,), device=p.device, dtype=torch.float32)
        check(lib.kgcn_masked_sqerr_f32(ptr(p), ptr(z), ptr(ml), B, T, ptr(dpred), ptr(stats), ptr(accum), current_stream()),
              "kgcn_masked_sqerr_f32")
        ctx.save_for_backward(dpred)
        ctx.batch = B * T
        ctx.set_materialize_grads(False)
        each = stats[:2 * T]
        ctx.mark_non_differentiable(each)
        return stats[2 * T + 1], stats[2 * T], each

    @staticmethod
    def backward(ctx, g_opt, g_sum, g_each):
        (dpred,) = ctx.saved_tensors
        return _loss_grad(dpred, g_opt, g_sum, ctx.batch), None, None, None


def masked_squared_error(pred, labels, mask_label, accum=None):
    """model_multimodal_regression.py:94-101 in one HIP pass -> (cost_opt, cost_sum, error_sum [T], count [T]): loss =
    mask_label (labels - pred)^2 on [B, T]; cost_opt = reduce_mean(loss) over the padded batch, cost_sum = reduce_sum(loss),
    error_sum / count per task (their totals are the file's metrics; mse = error_sum / count, kgcn/core.py:184-186).  accum: a
    float32 device block [2 T + 1] = error_sum | count | cost_sum the call adds its values to in place.  cost_opt and cost_sum
    are differentiable; a row with mask_label 0 has gradient exactly 0."""
    cost_opt, cost_sum, each = _MaskedSqErr.apply(pred, labels, mask_label, accum)
    T = pred.shape[1]
    return cost_opt, cost_sum, each[:T], each[T:]


REGRESSION_SUMS_COLUMNS = ("n", "sum_y", "ss_tot", "ss_res", "sum_log_ratio", "n_bad_ratio")


@torch.no_grad()
def regression_metrics(pred, label, mask=None):
    """The sums behind r2 / mse / gmfe (gcn.py:204-208) for every task at once -> [T, 6] float64 numpy array with the columns
    REGRESSION_SUMS_COLUMNS: n, sum y, sum (y - mean y)^2, sum (y - p)^2, sum log(y / p) over the rows with a positive finite
    ratio, the count of the other rows.  pred / label [n, T] float32 (rows may be strided), mask None (every row counts, as the
    reference) or [n, T].  Two passes in fp64 on the device in a fixed order; kgcn_amd.cv.regression_metrics_from_sums derives
    the metrics."""
    if pred.dim() != 2 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise _lib.KgcnHipError("regression_metrics: pred must be a [n >= 1, T >= 1] tensor, got %s" % (tuple(pred.shape),))
    n, T = pred.shape
    pred = _row_strided(pred, T, "pred")
    label = _row_strided(label.to(torch.float32), T, "label")
    mk = None if mask is None else _f32c(mask.to(torch.float32), "mask")
    if tuple(label.shape) != (n, T) or (mk is not None and tuple(mk.shape) != (n, T)):
        raise _lib.KgcnHipError("regression_metrics: label / mask do not match pred %s" % ((n, T),))
    sums = torch.empty((T, 6), device=pred.device, dtype=torch.float64)
    check(lib.kgcn_regression_sums_f64(pred.data_ptr(), pred.stride(0), label.data_ptr(), label.stride(0), ptr(mk), n, T,
                                       sums.data_ptr(), current_stream()), "kgcn_regression_sums_f64")
    return sums.cpu().numpy()


# -------------------------------------------------------------------------------------------------
# integrated gradients of the compound-protein interaction multitask network (kgcn visualize on multitask.py; csrc/cpiig.hip): the
# sweep over the scaled copies of many compounds, all tasks at once
# -------------------------------------------------------------------------------------------------
CPI_IG_TASKS_PER_PASS = _lib.K["KGCN_CPIIG_TASKS_PER_PASS"]           # tasks a lane of the accumulate pass carries


def cpi_ig_limits_check(nodes, width, tasks, steps):
    """The ranges csrc/cpiig.hip serves, on the host: N, Wd, T >= 1 and K >= 2 copies (the start and the end copy)."""
    N, Wd, T, K = int(nodes), int(width), int(tasks), int(steps)
    if N < 1 or Wd < 1 or T < 1:
        raise ValueError("cpi_ig: N = %d nodes, Wd = %d columns, T = %d tasks: each must be >= 1" % (N, Wd, T))
    if K < 2:
        raise ValueError("cpi_ig: %d scaled copies, at least 2 (the start and the end copy)" % K)
    return N, Wd, T, K


def _f32_vector(v, n, name, device, who="cpi_ig"):
    import numpy as np
    t = _f32c(v.detach(), name).reshape(-1) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, np.float32).reshape(-1), device=device)
    if t.numel() != n:
        raise ValueError("%s: %s has %d entries, expected %d" % (who, name, t.numel(), n))
    return t


@torch.no_grad()
def cpi_ig(P, Q, u, e, alpha, gamma, wA, wB=None):
    """csrc/cpiig.hip -> (p [C, K, T], GA [C, T, N, Wd], GB [C, T, N, Wd] or None).  P = sum_ch A_ch X W_ch and
    Q = sum_ch rowsum(A_ch) (x) b_ch, both [C, N, Wd]; u [T, Wd] and e [T] the per-task difference of the Dense layer's two
    columns and biases; alpha, gamma [K]: copy k has the pre-activation alpha[k] P + gamma[k] Q; wA, wB [K] copy weights.
    p[c, k, t] is task t's prediction of copy k, GA[c, t] = sum_k wA[k] d p[c, k, t] / d Z_k (GB with wB; not formed when wB is
    None).  A read-out: no autograd.  Bitwise reproducible, and a compound's rows do not depend on the others in the call."""
    P, Q = _f32c(P.detach(), "P"), _f32c(Q.detach(), "Q")
    u = _f32c(u.detach(), "u")
    if P.dim() != 3 or tuple(Q.shape) != tuple(P.shape):
        raise ValueError("cpi_ig: P and Q must both be [C, N, Wd], got %s and %s" % (tuple(P.shape), tuple(Q.shape)))
    if u.dim() != 2 or u.shape[1] != P.shape[2]:
        raise ValueError("cpi_ig: u must be [T, %d], got %s" % (P.shape[2], tuple(u.shape)))
    C = P.shape[0]
    dev = P.device
    K = alpha.numel() if torch.is_tensor(alpha) else len(alpha)
    N, Wd, T, K = cpi_ig_limits_check(P.shape[1], P.shape[2], u.shape[0], K)
    e = _f32_vector(e, T, "e", dev)
    alpha, gamma, wA = (_f32_vector(v, K, n, dev) for v, n in ((alpha, "alpha"), (gamma, "gamma"), (wA, "wA")))
    wB = None if wB is None else _f32_vector(wB, K, "wB", dev)
    p = torch.empty((C, K, T), device=dev, dtype=torch.float32)
    GA = torch.empty((C, T, N, Wd), device=dev, dtype=torch.float32)
    GB = None if wB is None else torch.empty_like(GA)
    nbytes = lib.kgcn_cpi_ig_workspace_bytes(C, Wd, T, K)
    ws = _lib.workspace(nbytes, dev)
    check(lib.kgcn_cpi_ig_f32(ptr(P), ptr(Q), C, N, Wd, ptr(u), ptr(e), T, ptr(alpha), ptr(gamma), ptr(wA), ptr(wB), K, ptr(p),
                              ptr(GA), ptr(GB), ptr(ws), nbytes, current_stream()), "kgcn_cpi_ig_f32")
    return p, GA, GB


@torch.no_grad()
def spmm_values_grad(csr, grad, rhs, rhs_ld=None, rhs_gs=None):
    """d values[e] = <grad[row_e, :], rhs[col_e, :]> for every stored entry of the batched CSR (the values gradient of bspmm as
    a read-out) -> [nnz] in CSR order.  grad [T*M, d]; rhs [T*K, d], or any fp32 tensor addressed by the row stride rhs_ld and
    the graph stride rhs_gs in floats (0, 0: one d-vector met by every entry)."""
    grad = _f32c(grad.detach(), "grad")
    rhs = _f32c(rhs.detach(), "rhs")
    if grad.dim() != 2 or grad.shape[0] != csr.num_graphs * csr.rows:
        raise ValueError("spmm_values_grad: grad must be [T*M, d] = [%d, d], got %s" % (csr.num_graphs * csr.rows, tuple(grad.shape)))
    d = grad.shape[1]
    if rhs_ld is None:
        if tuple(rhs.shape) != (csr.num_graphs * csr.cols, d):
            raise ValueError("spmm_values_grad: rhs must be [T*K, d] = [%d, %d], got %s" % (csr.num_graphs * csr.cols, d, tuple(rhs.shape)))
        rhs_ld, rhs_gs = d, csr.cols * d
    else:
        rhs_ld, rhs_gs = int(rhs_ld), int(rhs_gs)
        last = (csr.num_graphs - 1) * rhs_gs + (csr.cols - 1) * rhs_ld + d
        if rhs_ld < 0 or rhs_gs < 0 or last > rhs.numel():
            raise ValueError("spmm_values_grad: strides (%d, %d) reach past the %d floats of rhs" % (rhs_ld, rhs_gs, rhs.numel()))
    dv = torch.empty((csr.nnz,), device=grad.device, dtype=torch.float32)
    check(lib.kgcn_spmm_values_grad_f32(csr.desc(), ptr(grad), d, csr.rows * d, ptr(rhs), rhs_ld, rhs_gs, d, ptr(dv),
                                        current_stream()), "kgcn_spmm_values_grad_f32")
    return dv


# -------------------------------------------------------------------------------------------------
# integrated gradients over the per-graph vector of the vector-modality models (csrc/vecig.hip): the scaled copies of the vector
# branch's first layer, expanded from one product per compound and reduced to one gradient per compound
# -------------------------------------------------------------------------------------------------
IG_COPIES_MAX_WIDTH, IG_COPIES_MAX_COPIES, IG_COPIES_MAX_ROWS = (_lib.K[n] for n in (
    "KGCN_IG_COPIES_MAX_WIDTH", "KGCN_IG_COPIES_MAX_COPIES", "KGCN_IG_COPIES_MAX_ROWS"))


def ig_copies_limits_check(compounds, copies, width):
    """The ranges csrc/vecig.hip serves, on the host: 1 <= H <= IG_COPIES_MAX_WIDTH, 1 <= K <= IG_COPIES_MAX_COPIES, C >= 0 with
    C K <= IG_COPIES_MAX_ROWS -> (C, K, H)."""
    C, K, H = int(compounds), int(copies), int(width)
    if not 1 <= H <= IG_COPIES_MAX_WIDTH:
        raise ValueError("ig_copies: H = %d columns outside 1..%d" % (H, IG_COPIES_MAX_WIDTH))
    if not 1 <= K <= IG_COPIES_MAX_COPIES:
        raise ValueError("ig_copies: K = %d copies outside 1..%d" % (K, IG_COPIES_MAX_COPIES))
    if C < 0 or C * K > IG_COPIES_MAX_ROWS:
        raise ValueError("ig_copies: %d compounds x %d copies outside 0..%d rows" % (C, K, IG_COPIES_MAX_ROWS))
    return C, K, H


@torch.no_grad()
def ig_copies_expand(P, alpha, bias=None, gamma=None, beta=None, moving_mean=None, moving_variance=None, eps=1e-3, activation=None,
                     out=None, out_col=0):
    """The first Dense + BatchNormalization + activation layer of K scaled copies of C inputs from ONE product per input:
    P [C, H] = v W, alpha [K] -> Y [C K, H], Y[c K + k] = act(bn(alpha[k] P[c] + bias)) with bn(x) = gamma (x - moving_mean) /
    sqrt(moving_variance + eps) + beta (learning phase 0; gamma None, then beta and the statistics None too: no normalisation).
    The fp32 operations are those of dense -> graph_bn after the GEMM: a copy with alpha 1 is that layer applied to the same P,
    bit for bit.  out / out_col: Y goes into columns out_col .. out_col + H of the contiguous [C K, wide] buffer `out` and is
    returned as that view (as dense_bn writes).  A read-out: no autograd."""
    act = act_code(activation)
    if (gamma is None) != (beta is None) or (gamma is None) != (moving_mean is None) or (gamma is None) != (moving_variance is None):
        raise ValueError("ig_copies_expand: gamma, beta, moving_mean and moving_variance come together or not at all")
    require_gpu(P, "P")
    if P.dim() != 2:
        raise ValueError("ig_copies_expand: P must be [C, H], got %s" % (tuple(P.shape),))
    P = _f32c(P.detach(), "P")
    dev = P.device
    K = alpha.numel() if torch.is_tensor(alpha) else len(alpha)
    C, K, H = ig_copies_limits_check(P.shape[0], K, P.shape[1])
    alpha = _f32_vector(alpha, K, "alpha", dev, "ig_copies_expand")
    b, ga, be, mu, va = (None if v is None else _f32_vector(v, H, n, dev, "ig_copies_expand") for v, n in (
        (bias, "bias"), (gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_variance, "moving_variance")))
    out, y = _column_block(out, int(out_col), C * K, H, dev)
    check(lib.kgcn_ig_copies_expand_f32(ptr(P), C, K, H, ptr(alpha), ptr(b), ptr(ga), ptr(be), ptr(mu), ptr(va), float(eps), int(act),
                                        y.data_ptr(), y.stride(0) if C * K else H, current_stream()), "kgcn_ig_copies_expand_f32")
    return y


@torch.no_grad()
def ig_copies_reduce(dY, Y, weights, scale=None, activation=None):
    """The weighted sum over the K copies of every input of the gradient with respect to the first layer's pre-activation:
    dY, Y [C K, H] (the gradient arriving at the layer's output and that output; rows may be strided), weights [K], scale [H]
    (the normalisation's gamma / sqrt(moving_variance + eps); None: ones) -> S [C, H] = scale sum_k weights[k] dY[c K + k]
    act'(Y[c K + k]), summed over k in order in fp32.  A copy of weight 0 is skipped: whatever its dY rows hold (NaN included) never reaches the sum.  S W^T is then
    the summed gradient with respect to the layer's input.  A read-out: no autograd; bitwise reproducible, and an input's row
    does not depend on the others in the call."""
    act = act_code(activation)
    if Y.dim() != 2 or tuple(dY.shape) != tuple(Y.shape):
        raise ValueError("ig_copies_reduce: dY and Y must both be [C K, H], got %s and %s" % (tuple(dY.shape), tuple(Y.shape)))
    rows, H = Y.shape
    K = weights.numel() if torch.is_tensor(weights) else len(weights)
    if K < 1 or rows % K:
        raise ValueError("ig_copies_reduce: %d rows are not copies of %d weights" % (rows, K))
    C, K, H = ig_copies_limits_check(rows // K, K, H)
    dY, Y = _row_strided(dY.detach(), H, "dY"), _row_strided(Y.detach(), H, "Y")
    dev = Y.device
    w = _f32_vector(weights, K, "weights", dev, "ig_copies_reduce")
    sc = None if scale is None else _f32_vector(scale, H, "scale", dev, "ig_copies_reduce")
    S = torch.empty((C, H), device=dev, dtype=torch.float32)
    check(lib.kgcn_ig_copies_reduce_f32(dY.data_ptr(), dY.stride(0) if rows else H, Y.data_ptr(), Y.stride(0) if rows else H, C, K, H,
                                        ptr(w), ptr(sc), int(act), ptr(S), current_stream()), "kgcn_ig_copies_reduce_f32")
    return S


# -------------------------------------------------------------------------------------------------
# classical graph kernels of graph_kernel/gk.py (csrc/graphkern.hip; the drivers are kgcn_amd/graph_kernel.py): colour
# refinement, feature runs and the exact f64 Gram over them.  Read-outs: no autograd.  Integer-exact, bitwise reproducible.
# -------------------------------------------------------------------------------------------------
GRAM_CHUNK_COLS = 1024              # dense columns laid out per MFMA pass of gram_from_runs (a multiple of 16)
HASH_MASK_FULL = (1 << 64) - 1


def _ws_bytes(nbytes, what, device):
    if nbytes < 0:
        check(1, what)
    return _lib.workspace(nbytes, device, torch.uint8), nbytes


_SAME = "same"                      # a shape entry of _operand: the size of the dimension before it


def _operand(who, name, t, dtype, shape):
    """THE operand check of this section and the three below it: t is a contiguous device tensor of `dtype` and `shape` -> t, or
    a KgcnHipError that names the op, the operand, what was expected and what came.  shape: an int is an element count (any
    contiguous layout of it); a tuple has one entry a dimension -- an int, None (open: the op reads the size from the operand),
    (lo, hi) (open within lo..hi; hi None: no upper limit) or _SAME; None leaves the whole shape open."""
    got = t.shape
    if shape is None or isinstance(shape, int):
        fits = shape is None or t.numel() == shape
    else:
        fits = len(got) == len(shape)
        for i, want in enumerate(shape if fits else ()):
            if want == _SAME:
                fits = got[i] == got[i - 1]
            elif isinstance(want, tuple):
                fits = got[i] >= want[0] and (want[1] is None or got[i] <= want[1])
            elif want is not None:
                fits = got[i] == want
            if not fits:
                break
    if fits and t.is_cuda and t.dtype == dtype and t.is_contiguous():
        return t
    if isinstance(shape, tuple):                                      # the refusal: only now is the expectation spelled out
        expected = "shape [%s]" % ", ".join("*" if w is None else "%d..%s" % (w[0], "" if w[1] is None else w[1]) if isinstance(w, tuple)
                                            else str(w) for w in shape)
    else:
        expected = "any shape" if shape is None else "%d elements" % shape
    raise _lib.KgcnHipError("%s: %s must be a contiguous %s device tensor of %s, got a %s%s %s tensor of shape %s" % (
        who, name, dtype, expected, "" if t.is_contiguous() else "non-contiguous ", t.dtype, "device" if t.is_cuda else "host", list(got)))


def _ptr_if(t, n):
    """The pointer of an operand of n elements, NULL when there are none (an empty tensor's pointer is not defined)."""
    return ptr(t) if n else None


def _plain_square(csr, who):
    if not isinstance(csr, BatchedCSR) or csr.row_pad != 0 or csr.rows != csr.cols:
        raise _lib.KgcnHipError("%s takes a plain square BatchedCSR" % who)
    return csr.num_graphs, csr.rows


# The four ops below have a plain form and a copies form (R colourings of the same graphs: the next section).  As in
# csrc/graphkern.h, where both C entry points wrap one launcher and plain is copies == 1, each has ONE host body: `who` is the
# public name, `entry` its C entry point kgcn_<who>_i32, `copies` None the plain form, whose entry point takes no copies argument.
def _copies(copies, T, M, who):
    """-> (R, the arguments only the copies entry points take)."""
    if copies is None:
        return 1, ()
    copies = int(copies)
    if copies < 1 or copies * T * M >= 2 ** 31 - 1:
        raise _lib.KgcnHipError("%s: %d copies of %d graphs x %d rows; at least one copy and fewer than 2^31 - 1 rows in all "
                                "(positions and colours are int32)" % (who, copies, T, M))
    return copies, (copies,)


def _wl_refine(who, entry, csr, num_nodes, colors, copies, hash_mask):
    T, M = _plain_square(csr, who)
    R, extra = _copies(copies, T, M, who)
    _operand(who, "num_nodes", num_nodes, torch.int32, T), _operand(who, "colors", colors, torch.int32, R * T * M)
    sorted_nbr = torch.empty((R, max(csr.nnz, 1)), device=csr.device, dtype=torch.int32)
    keys = torch.empty((2, max(R * T * M, 1)), device=csr.device, dtype=torch.int64)
    check(entry(ctypes.byref(csr.desc()), ptr(num_nodes), ptr(colors), *extra, int(hash_mask) & HASH_MASK_FULL, ptr(sorted_nbr),
                ptr(keys[0]), ptr(keys[1]), current_stream()), "kgcn_%s_i32" % who)
    return sorted_nbr[0] if copies is None else sorted_nbr, keys[0], keys[1]


def _wl_rank(who, entry, csr, num_nodes, colors, copies, sorted_nbr, key_hi, key_lo):
    T, M = _plain_square(csr, who)
    R, extra = _copies(copies, T, M, who)
    n = R * T * M
    _operand(who, "num_nodes", num_nodes, torch.int32, T), _operand(who, "colors", colors, torch.int32, n)
    _operand(who, "sorted_nbr", sorted_nbr, torch.int32, (R,) * len(extra) + (max(csr.nnz, 1),))     # what _wl_refine returns
    _operand(who, "key_hi", key_hi, torch.int64, max(n, 1)), _operand(who, "key_lo", key_lo, torch.int64, max(n, 1))
    new = torch.empty((max(n, 1),), device=csr.device, dtype=torch.int32)
    info = torch.empty((2,), device=csr.device, dtype=torch.int64)
    query = lib.kgcn_wl_rank_copies_workspace_bytes if extra else lib.kgcn_wl_rank_workspace_bytes
    ws, wsb = _ws_bytes(query(T * M, *extra), "kgcn_%s_workspace_bytes" % who, csr.device)
    check(entry(ctypes.byref(csr.desc()), ptr(num_nodes), ptr(colors), *extra, ptr(sorted_nbr), ptr(key_hi), ptr(key_lo), ptr(new),
                ptr(info), ptr(ws), wsb, current_stream()), "kgcn_%s_i32" % who)
    return new[:n], info


def _two_pass_runs(call, T, extra, dev, what):
    """The count call over the copies * T run slots, the read of the total, the emit call -> (run_col int64 (u64 bits),
    run_graph, run_count int32)."""
    slots = T * (extra[0] if extra else 1)
    run_ptr = torch.empty((slots + 1,), device=dev, dtype=torch.int64)
    query = lib.kgcn_graph_runs_copies_workspace_bytes if extra else lib.kgcn_graph_runs_workspace_bytes
    ws, wsb = _ws_bytes(query(T, *extra), "kgcn_graph_runs_copies_workspace_bytes" if extra else "kgcn_graph_runs_workspace_bytes", dev)
    check(call(run_ptr, None, None, None, 0, ws, wsb), what)
    total = int(run_ptr[slots].item())
    col, graph, count = (torch.empty((max(total, 1),), device=dev, dtype=dt) for dt in (torch.int64, torch.int32, torch.int32))
    check(call(run_ptr, col, graph, count, total, ws, wsb), what)
    return col[:total], graph[:total], count[:total]


def _wl_runs(who, entry, colors, num_nodes, T, M, copies, column_offset, column_stride):
    R, extra = _copies(copies, T, M, who)
    _operand(who, "num_nodes", num_nodes, torch.int32, T), _operand(who, "colors", colors, torch.int32, R * T * M)
    stride = (int(column_stride),) if extra else ()
    return _two_pass_runs(lambda rp, c, g, n, cap, ws, wsb: entry(
        ptr(colors), ptr(num_nodes), T, M, *extra, int(column_offset), *stride, ptr(rp), ptr(c), ptr(g), ptr(n), cap, ptr(ws), wsb,
        current_stream()), T, extra, colors.device, "kgcn_%s_i32" % who)


def _sp_features(who, entry, csr, num_nodes, labels, copies, num_labels):
    T, M = _plain_square(csr, who)
    R, extra = _copies(copies, T, M, who)
    _operand(who, "num_nodes", num_nodes, torch.int32, T), _operand(who, "labels", labels, torch.int32, R * T * M)
    return _two_pass_runs(lambda rp, c, g, n, cap, ws, wsb: entry(
        ctypes.byref(csr.desc()), ptr(num_nodes), ptr(labels), *extra, int(num_labels), ptr(rp), ptr(c), ptr(g), ptr(n), cap, ptr(ws),
        wsb, current_stream()), T, extra, csr.device, "kgcn_%s_i32" % who)


@torch.no_grad()
def wl_refine(csr, num_nodes, colors, hash_mask=HASH_MASK_FULL):
    """First half of one Weisfeiler-Lehman refinement -> (sorted_nbr [max(nnz, 1)] int32: every row's neighbour colours ascending,
    key_hi, key_lo [T*M] int64 holding the two words of the 128-bit signature mix, and-ed with hash_mask)."""
    return _wl_refine("wl_refine", lib.kgcn_wl_refine_i32, csr, num_nodes, colors, None, hash_mask)


@torch.no_grad()
def wl_rank(csr, num_nodes, colors, sorted_nbr, key_hi, key_lo):
    """Second half: dense colours of the key classes -> (new_colors [T*M] int32, -1 for rows that do not exist; info [2] int64
    device tensor = number of colours, pairs of equal keys with different true signatures -- 0 iff the partition is exact)."""
    return _wl_rank("wl_rank", lib.kgcn_wl_rank_i32, csr, num_nodes, colors, None, sorted_nbr, key_hi, key_lo)


@torch.no_grad()
def wl_runs(colors, num_nodes, T, M, column_offset):
    """The colour histogram of every graph as feature runs, column = column_offset + colour."""
    return _wl_runs("wl_runs", lib.kgcn_wl_runs_i32, colors, num_nodes, T, M, None, column_offset, None)


@torch.no_grad()
def sp_features(csr, num_nodes, labels, num_labels):
    """Shortest-path feature runs: per graph the counts of (label_k, label_j, distance) over all ordered node pairs, k = j
    and unreachable pairs (distance 255) included; column = label_k << 20 | label_j << 8 | distance."""
    return _sp_features("sp_features", lib.kgcn_sp_features_i32, csr, num_nodes, labels, None, num_labels)


@torch.no_grad()
def gram_from_runs(run_col, run_graph, run_count, G, chunk_cols=None, normalize=False, return_stats=False):
    """K [G, G] float64 = F F^T of the count matrix the runs describe, exact (csrc/graphkern.hip: one-graph columns on an
    int64 diagonal, the others through v_mfma_f64_16x16x4_f64, chunk_cols dense columns a pass).  normalize: K_ij /
    sqrt(K_ii K_jj).  return_stats: also {"columns", "diag_columns", "dense_columns"}.  One read-back (the dense column count)."""
    chunk_cols = GRAM_CHUNK_COLS if chunk_cols is None else int(chunk_cols)
    who = "gram_from_runs"
    n = int(_operand(who, "run_col", run_col, torch.int64, None).numel())
    dev = run_col.device
    _operand(who, "run_graph", run_graph, torch.int32, n), _operand(who, "run_count", run_count, torch.int32, n)
    ws, wsb = _ws_bytes(lib.kgcn_graph_gram_workspace_bytes(n, G, chunk_cols), "kgcn_graph_gram_workspace_bytes", dev)
    stats = torch.empty((3,), device=dev, dtype=torch.int64)
    col, graph, count = _ptr_if(run_col, n), _ptr_if(run_graph, n), _ptr_if(run_count, n)
    check(lib.kgcn_gram_plan_i64(col, graph, count, n, G, chunk_cols, ptr(stats), ptr(ws), wsb, current_stream()), "kgcn_gram_plan_i64")
    cols, diag_cols, dense_cols = stats.tolist()
    K = torch.empty((G, G), device=dev, dtype=torch.float64)
    check(lib.kgcn_gram_dense_f64(graph, count, n, G, dense_cols, chunk_cols, ptr(K), ptr(ws), wsb, current_stream()),
          "kgcn_gram_dense_f64")
    if normalize:
        K = gram_normalize(K)
    if return_stats:
        return K, {"columns": cols, "diag_columns": diag_cols, "dense_columns": dense_cols}
    return K


@torch.no_grad()
def gram_normalize(K):
    """auxiliary_methods.normalize_gram_matrix in fp64 on the device: K_ij / sqrt(K_ii K_jj), 0 where a diagonal entry is 0."""
    out = torch.empty_like(_operand("gram_normalize", "K", K, torch.float64, (None, _SAME)))
    check(lib.kgcn_gram_normalize_f64(ptr(K), K.shape[0], ptr(out), current_stream()), "kgcn_gram_normalize_f64")
    return out


# -------------------------------------------------------------------------------------------------
# hash graph kernels for continuous node attributes (csrc/hashkern.hip; the driver is graph_kernel.hash_graph_kernel): the fp64
# scaling and bucketing of attribute rows, the ranking of int64 pairs, and R colourings ("copies") of the same graphs through
# one launch sequence of the refinement, run and shortest-path kernels.  fp64 and integers: bitwise reproducible.
# -------------------------------------------------------------------------------------------------
LSH_MAX_DIM = _lib.K["KGCN_LSH_MAX_DIM"]


_ATTR_ROWS = ((1, None), (1, LSH_MAX_DIM))   # the shape of attribute rows [rows, d]: at least one row, 1..LSH_MAX_DIM attributes


@torch.no_grad()
def attr_scale(x):
    """Attribute rows x [rows, d] float64 (the existing nodes in graph order) -> (scaled [rows, d], mean [d], std [d]):
    sklearn.preprocessing.scale of hash_graph_kernel.py:40 in the summation order csrc/hashkern.hip states (chunks of 256 rows,
    then the chunk sums, nothing fused); a column of equal values becomes 0."""
    rows, d = _operand("attr_scale", "x", x, torch.float64, _ATTR_ROWS).shape
    dev = x.device
    scaled = torch.empty_like(x)
    stats = torch.empty((2, d), device=dev, dtype=torch.float64)
    ws, wsb = _ws_bytes(lib.kgcn_attr_scale_workspace_bytes(rows, d), "kgcn_attr_scale_workspace_bytes", dev)
    check(lib.kgcn_attr_scale_f64(ptr(x), rows, d, ptr(scaled), ptr(stats[0]), ptr(stats[1]), ptr(ws), wsb, current_stream()),
          "kgcn_attr_scale_f64")
    return scaled, stats[0], stats[1]


@torch.no_grad()
def lsh_buckets(x, v, b, bin_width):
    """bucket [R, rows] int64 = floor((x . v_r + b_r) / bin_width) of auxiliary_methods.py:31, the dot product added for k
    ascending and unfused.  x [rows, d], v [R, d], b [R] float64 on the device.  A value that is not finite or reaches 2^62 in
    magnitude raises (one read-back of the device's error count): nothing wraps silently."""
    rows, d = _operand("lsh_buckets", "x", x, torch.float64, _ATTR_ROWS).shape
    R = _operand("lsh_buckets", "v", v, torch.float64, ((1, None), d)).shape[0]
    _operand("lsh_buckets", "b", b, torch.float64, (R,))
    w = float(bin_width)
    if not 0.0 < w < float("inf"):
        raise _lib.KgcnHipError("lsh_buckets: the bin width %r must be positive and finite" % (bin_width,))
    if R * rows >= 2 ** 31 - 1:
        raise _lib.KgcnHipError("lsh_buckets: %d draws x %d rows; fewer than 2^31 - 1 buckets a call" % (R, rows))
    bucket = torch.empty((R, rows), device=x.device, dtype=torch.int64)
    errors = torch.empty((1,), device=x.device, dtype=torch.int64)
    check(lib.kgcn_lsh_buckets_f64(ptr(x), rows, d, ptr(v), ptr(b), R, ctypes.byref(ctypes.c_double(w)), ptr(bucket), ptr(errors),
                                   current_stream()), "kgcn_lsh_buckets_f64")
    bad = int(errors.item())
    if bad:
        raise _lib.KgcnHipError("lsh_buckets: %d of %d projected values (x . v + b) / %g are not finite or reach 2^62: no int64 "
                                "bucket holds them, refused" % (bad, R * rows, w))
    return bucket


@torch.no_grad()
def rank_pairs(hi, lo, mark=None):
    """Dense ranks int32 [n] of the int64 pairs (hi, lo) in ascending signed order -- np.unique(..., return_inverse=True) of the
    pairs -- and info [2] int64 on the device = (number of classes, existing rows with hi == 2^63 - 1: refuse when not 0).
    mark: None or int32 [n]; a row with mark < 0 does not exist, takes no part and gets -1."""
    n = int(_operand("rank_pairs", "hi", hi, torch.int64, (None,)).numel())
    _operand("rank_pairs", "lo", lo, torch.int64, (n,))
    if mark is not None:
        _operand("rank_pairs", "mark", mark, torch.int32, (n,))
    dev = hi.device
    ranks = torch.empty((max(n, 1),), device=dev, dtype=torch.int32)
    info = torch.empty((2,), device=dev, dtype=torch.int64)
    ws, wsb = _ws_bytes(lib.kgcn_rank_pairs_workspace_bytes(n), "kgcn_rank_pairs_workspace_bytes", dev)
    check(lib.kgcn_rank_pairs_i64(_ptr_if(hi, n), _ptr_if(lo, n), None if mark is None else _ptr_if(mark, n), n,
                                  ptr(ranks), ptr(info), ptr(ws), wsb, current_stream()), "kgcn_rank_pairs_i64")
    return ranks[:n], info


@torch.no_grad()
def wl_refine_copies(csr, num_nodes, colors, copies, hash_mask=HASH_MASK_FULL):
    """wl_refine for colors [copies, T*M] over the one stored batch -> (sorted_nbr [copies, max(nnz, 1)], key_hi, key_lo [copies * T*M])."""
    return _wl_refine("wl_refine_copies", lib.kgcn_wl_refine_copies_i32, csr, num_nodes, colors, copies, hash_mask)


@torch.no_grad()
def wl_rank_copies(csr, num_nodes, colors, copies, sorted_nbr, key_hi, key_lo):
    """wl_rank over all copies in one ranking -> (new_colors [copies * T*M] int32, info [2]): copies whose colours are disjoint
    stay disjoint, and one info -- one read-back -- serves them all."""
    return _wl_rank("wl_rank_copies", lib.kgcn_wl_rank_copies_i32, csr, num_nodes, colors, copies, sorted_nbr, key_hi, key_lo)


@torch.no_grad()
def wl_runs_copies(colors, num_nodes, T, M, copies, column_offset, column_stride):
    """The colour histograms of every (copy, graph) as feature runs in slot order (all graphs of copy 0, then copy 1, ...),
    column = column_offset + copy * column_stride + colour, graph = t."""
    return _wl_runs("wl_runs_copies", lib.kgcn_wl_runs_copies_i32, colors, num_nodes, T, M, copies, column_offset, column_stride)


@torch.no_grad()
def sp_features_copies(csr, num_nodes, labels, copies, num_labels):
    """sp_features for labels [copies, T*M]: the breadth-first searches run once a graph, the keys of every copy are sorted and
    counted from the same distances; runs in slot order, column = copy << 32 | label_k << 20 | label_j << 8 | distance.
    num_labels: every copy's labels are below it, up to 4,096."""
    return _sp_features("sp_features_copies", lib.kgcn_sp_features_copies_i32, csr, num_nodes, labels, copies, num_labels)


# -------------------------------------------------------------------------------------------------
# batched C-SVC over a precomputed kernel (csrc/svm.hip; the drivers are graph_kernel.svm_fit / svm_decision / svm_predict /
# svm_cv): libsvm's SMO in fp64, one workgroup a problem, bounded launches.  fp64 and integers: bitwise reproducible.
# -------------------------------------------------------------------------------------------------
SVM_MAX_ROWS, SVM_MAX_CLASSES, SVM_DEFAULT_SLICE = (_lib.K[n] for n in ("KGCN_SVM_MAX_ROWS", "KGCN_SVM_MAX_CLASSES",
                                                                        "KGCN_SVM_DEFAULT_SLICE"))
SVM_RUNNING, SVM_CONVERGED, SVM_MAX_ITER, SVM_REFUSED = (_lib.K[n] for n in ("KGCN_SVM_RUNNING", "KGCN_SVM_CONVERGED",
                                                                             "KGCN_SVM_MAX_ITER", "KGCN_SVM_REFUSED"))
_SVM_MAX_GRAPHS = 46340              # what gram_from_runs builds


class SvmNotConverged(_lib.KgcnHipError):
    """svm_smo_batch stopped problems at max_iter.  problems: their indices; result: what svm_smo_batch would have returned
    (the state after max_iter iterations, as libsvm returns it with a warning)."""

    def __init__(self, problems, n_iter, result):
        self.problems, self.result = problems, result
        shown = ", ".join("%d (%d iterations)" % (p, n_iter[p]) for p in problems[:8])
        super().__init__("svm_smo_batch: %d of %d problems reached max_iter before m(alpha) - M(alpha) < tol: problem %s%s"
                         % (len(problems), len(n_iter), shown, ", ..." if len(problems) > 8 else ""))


class SvmSets:
    """Index sets into the rows of a Gram matrix, on the host (checked there) and on the device (read there): sets[s] an
    integer array of rows of K; signs[s] (training sets) the label +1 / -1 of each entry, None for evaluation sets."""

    def __init__(self, sets, signs=None, graphs=None, device="cuda"):
        import numpy as np
        sets = [np.asarray(s, np.int64).reshape(-1) for s in sets]
        self.lengths = np.array([s.shape[0] for s in sets], np.int64)
        self.count, self.total = len(sets), int(self.lengths.sum())
        self.max_rows = int(self.lengths.max()) if sets else 0
        self.ptr_host = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.idx_host = (np.concatenate(sets) if self.total else np.zeros(0, np.int64)).astype(np.int64)
        if self.total and (self.idx_host.min() < 0 or (graphs is not None and self.idx_host.max() >= graphs)):
            raise ValueError("an index set names a row outside 0..%s" % ("?" if graphs is None else graphs - 1))
        if self.total and self.idx_host.max() >= 2 ** 31 - 1:
            raise ValueError("row indices are int32")
        self.sign_host = None
        if signs is not None:
            signs = [np.asarray(s).reshape(-1) for s in signs]
            if len(signs) != len(sets) or any(a.shape != b.shape for a, b in zip(signs, sets)):
                raise ValueError("signs must match the sets entry for entry")
            self.sign_host = (np.concatenate(signs) if self.total else np.zeros(0)).astype(np.int8)
            if self.total and not np.all(np.abs(np.concatenate(signs)) == 1):
                raise ValueError("signs must be +1 or -1")
        self.ptr = torch.from_numpy(self.ptr_host).to(device)
        self.idx = torch.from_numpy(np.concatenate([self.idx_host.astype(np.int32), np.zeros(1, np.int32)])).to(device)
        self.sign = None if self.sign_host is None else torch.from_numpy(np.concatenate([self.sign_host, np.ones(1, np.int8)])).to(device)
        self.device = self.ptr.device

    def rows(self, s):
        return self.idx_host[self.ptr_host[s]:self.ptr_host[s + 1]]

    def args(self):
        """What the C entry points take for a list of sets: (ptr, idx, [sign,] count, total, max_rows)."""
        signs = () if self.sign is None else (ptr(self.sign),)
        return (ptr(self.ptr), ptr(self.idx)) + signs + (self.count, self.total, self.max_rows)


_SVM_GRAM = ((1, _SVM_MAX_GRAPHS), _SAME)


def _ws_word(ws):
    """The int32 control word of a workspace (what is still running), at its head as the entry point aligns it to 256 bytes."""
    return ws[(-ws.data_ptr()) % 256:][:4].view(torch.int32)


def _svm_host_i32(a, name, n, lo, hi, who):
    import numpy as np
    a = np.asarray(a, np.int64).reshape(-1)
    if a.shape[0] != n or (n and (a.min() < lo or a.max() >= hi)):
        raise ValueError("%s: %s must hold %d values in %d..%d" % (who, name, n, lo, hi - 1))
    return a.astype(np.int32)


def _svm_train_sets(sets, G, who):
    if not isinstance(sets, SvmSets) or sets.sign is None:
        raise _lib.KgcnHipError("%s: the training sets must be an SvmSets with signs" % who)
    if sets.total and sets.idx_host.max() >= G:
        raise ValueError("%s: a training set names row %d of a %d-row K" % (who, int(sets.idx_host.max()), G))
    if sets.max_rows > SVM_MAX_ROWS:
        raise _lib.KgcnHipError("%s: %d training rows in one set, up to %d (G, alpha and QD of a problem live in LDS); refused before "
                                "any launch" % (who, sets.max_rows, SVM_MAX_ROWS))
    if sets.count and sets.lengths.min() < 1:
        raise ValueError("%s: an empty training set" % who)


@torch.no_grad()
def svm_smo_batch(K, sets, prob_set, prob_C, tol=1e-3, max_iter=None, iters_per_launch=None):
    """Solve P C-SVC duals over the one Gram matrix K [G, G] float64 on the device: problem p trains on set prob_set[p] of `sets` (an
    SvmSets with signs) with C = prob_C[p].  -> (alpha [P, sets.max_rows] float64, rho [P] float64, n_iter [P] int64 device tensors;
    status [P] host int32 of SVM_* codes; the number of launches).  Each launch runs at most iters_per_launch (default
    SVM_DEFAULT_SLICE) iterations a problem and one word is read back after it; slicing changes no bit.  max_iter None: libsvm's
    max(10^7, 100 n) per problem.  A problem that reaches max_iter raises SvmNotConverged (which carries the state): unconverged
    coefficients are never returned silently.  Sets of more than SVM_MAX_ROWS rows are refused before any launch."""
    import numpy as np
    who = "svm_smo_batch"
    G = _operand(who, "K", K, torch.float64, _SVM_GRAM).shape[0]
    _svm_train_sets(sets, G, who)
    P = len(np.asarray(prob_set).reshape(-1))
    ps = _svm_host_i32(prob_set, "prob_set", P, 0, max(sets.count, 1), who)
    pc = np.asarray(prob_C, np.float64).reshape(-1)
    if pc.shape[0] != P or not np.all((pc > 0) & np.isfinite(pc)):
        raise ValueError("%s: prob_C must hold %d positive finite values" % (who, P))
    tol = float(tol)
    if not 0.0 < tol < float("inf"):
        raise ValueError("%s: tol must be positive and finite, got %r" % (who, tol))
    ipl = SVM_DEFAULT_SLICE if iters_per_launch is None else int(iters_per_launch)
    cap = 0 if max_iter is None else int(max_iter)
    if ipl < 1 or ipl >= 2 ** 31 or (max_iter is not None and cap < 1):
        raise ValueError("%s: iters_per_launch and max_iter must be at least 1" % who)
    dev = K.device
    stride = max(sets.max_rows, 1)
    alpha = torch.zeros((P, stride), device=dev, dtype=torch.float64)
    rho = torch.zeros((P,), device=dev, dtype=torch.float64)
    n_iter = torch.zeros((P,), device=dev, dtype=torch.int64)
    status = torch.zeros((P,), device=dev, dtype=torch.int32)
    if P == 0:
        return alpha, rho, n_iter, np.zeros(0, np.int32), 0
    d_ps, d_pc = torch.from_numpy(ps).to(dev), torch.from_numpy(pc).to(dev)
    ws, wsb = _ws_bytes(lib.kgcn_svm_workspace_bytes(P, stride), "kgcn_svm_workspace_bytes", dev)
    word = _ws_word(ws)
    longest = max(int(10_000_000), 100 * stride) if max_iter is None else cap
    slices = 0
    while True:
        check(lib.kgcn_svm_smo_f64(ptr(K), G, *sets.args(), ptr(d_ps), ptr(d_pc), P, ctypes.byref(ctypes.c_double(tol)), cap, ipl,
                                   1 if slices == 0 else 0, ptr(alpha), ptr(rho), ptr(n_iter), ptr(status), ptr(ws), wsb,
                                   current_stream()), "kgcn_svm_smo_f64")
        slices += 1
        if int(word.item()) == 0:
            break
        if slices > longest // ipl + 2:
            raise _lib.KgcnHipError("%s: problems still running after %d launches of %d iterations" % (who, slices, ipl))
    st = status.cpu().numpy()
    refused = np.flatnonzero(st == SVM_REFUSED)
    if refused.size:
        raise _lib.KgcnHipError("%s: the device refused the descriptors of %d problems (first: %d)" % (who, refused.size, refused[0]))
    result = (alpha, rho, n_iter, st, slices)
    late = np.flatnonzero(st != SVM_CONVERGED)
    if late.size:
        raise SvmNotConverged([int(p) for p in late], n_iter.cpu().numpy(), result)
    return result


def _svm_refuse_errors(errors, who):
    bad = int(errors.item())
    if bad:
        raise _lib.KgcnHipError("%s: the device found %d descriptors out of range; nothing was written for them" % (who, bad))


@torch.no_grad()
def svm_decision_batch(K, sets, prob_set, alpha, rho, eval_sets, job_prob, job_eval, check_errors=True):
    """Decision values of jobs (problem job_prob[q], evaluation set job_eval[q] of the SvmSets eval_sets) -> (dec flat float64 device
    tensor, job_out host int64 [jobs + 1]: job q owns dec[job_out[q]:job_out[q + 1]], one value a row of its set; errors [1] device).
    dec = sum_t (alpha_t y_t) K[row, idx_t] - rho, t ascending over all training rows (libsvm's sign: positive is the +1 class)."""
    import numpy as np
    who = "svm_decision_batch"
    G = _operand(who, "K", K, torch.float64, _SVM_GRAM).shape[0]
    _svm_train_sets(sets, G, who)
    if not isinstance(eval_sets, SvmSets):
        raise _lib.KgcnHipError("%s: the evaluation sets must be an SvmSets" % who)
    if eval_sets.total and eval_sets.idx_host.max() >= G:
        raise ValueError("%s: an evaluation set names row %d of a %d-row K" % (who, int(eval_sets.idx_host.max()), G))
    P = len(np.asarray(prob_set).reshape(-1))
    ps = _svm_host_i32(prob_set, "prob_set", P, 0, max(sets.count, 1), who)
    J = len(np.asarray(job_prob).reshape(-1))
    jp = _svm_host_i32(job_prob, "job_prob", J, 0, max(P, 1), who)
    je = _svm_host_i32(job_eval, "job_eval", J, 0, max(eval_sets.count, 1), who)
    if J > 65535:
        raise ValueError("%s: %d jobs, up to 65,535 a call" % (who, J))
    stride = max(sets.max_rows, 1)
    _operand(who, "alpha", alpha, torch.float64, (P, stride)), _operand(who, "rho", rho, torch.float64, (P,))
    job_out = np.concatenate([[0], np.cumsum(eval_sets.lengths[je])]).astype(np.int64)
    total, dev = int(job_out[-1]), K.device
    dec = torch.zeros((max(total, 1),), device=dev, dtype=torch.float64)
    errors = torch.zeros((1,), device=dev, dtype=torch.int64)
    d_ps, d_jp, d_je, d_jo = (torch.from_numpy(a).to(dev) for a in (ps, jp, je, job_out))
    check(lib.kgcn_svm_decision_f64(ptr(K), G, *sets.args(), ptr(d_ps), P, ptr(alpha), ptr(rho), *eval_sets.args(), ptr(d_jp), ptr(d_je),
                                    ptr(d_jo), J, ptr(dec), total, ptr(errors), current_stream()), "kgcn_svm_decision_f64")
    if check_errors:
        _svm_refuse_errors(errors, who)
    return dec[:total], job_out, errors


@torch.no_grad()
def svm_vote(dec, job_out, eval_sets, vote_first_job, vote_eval, classes, labels, check_errors=True):
    """libsvm's one-vs-one vote: vote v reads the classes (classes - 1) / 2 consecutive jobs from vote_first_job[v] (pair order (0, 1),
    (0, 2), ..., (1, 2), ...; all on evaluation set vote_eval[v]) -> (pred flat int32 class indices, vote_out host int64 [votes + 1],
    counts int64 [votes + 1] on the device: counts[v] = rows of vote v whose prediction equals labels[row], counts[votes] = descriptors
    the device refused -- one read-back serves a whole nested cross-validation).  labels [G] int32 device: class index of every row of K.
    Two classes: class 1 unless dec > 0 (scikit-learn: classes_[1] where its decision_function >= 0)."""
    import numpy as np
    who = "svm_vote"
    classes = int(classes)
    if not 2 <= classes <= SVM_MAX_CLASSES:
        raise ValueError("%s: %d classes, 2..%d" % (who, classes, SVM_MAX_CLASSES))
    if not isinstance(eval_sets, SvmSets):
        raise _lib.KgcnHipError("%s: the evaluation sets must be an SvmSets" % who)
    job_out = np.ascontiguousarray(job_out, np.int64).reshape(-1)
    J, npairs = job_out.shape[0] - 1, classes * (classes - 1) // 2
    if J < 0:
        raise _lib.KgcnHipError("%s: job_out must hold jobs + 1 offsets, got none" % who)
    total = int(job_out[-1])
    _operand(who, "dec", dec, torch.float64, total)                   # job_out[-1] values
    G = int(_operand(who, "labels", labels, torch.int32, (None,)).numel())
    if eval_sets.total and eval_sets.idx_host.max() >= G:
        raise ValueError("%s: an evaluation set names row %d, labels holds %d" % (who, int(eval_sets.idx_host.max()), G))
    V = len(np.asarray(vote_first_job).reshape(-1))
    vf = _svm_host_i32(vote_first_job, "vote_first_job", V, 0, max(J - npairs + 1, 1), who)
    ve = _svm_host_i32(vote_eval, "vote_eval", V, 0, max(eval_sets.count, 1), who)
    if V > 65535:
        raise ValueError("%s: %d votes, up to 65,535 a call" % (who, V))
    m = eval_sets.lengths[ve]
    for s in range(npairs):
        if V and not np.array_equal(job_out[vf + s + 1] - job_out[vf + s], m):
            raise ValueError("%s: the jobs of a vote do not all cover its evaluation set" % who)
    vote_out = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    ptotal, dev = int(vote_out[-1]), dec.device
    pred = torch.zeros((max(ptotal, 1),), device=dev, dtype=torch.int32)
    counts = torch.zeros((V + 1,), device=dev, dtype=torch.int64)
    d_jo, d_vf, d_ve, d_vo = (torch.from_numpy(a).to(dev) for a in (job_out, vf, ve, vote_out))
    dec1 = dec if total else torch.zeros((1,), device=dev, dtype=torch.float64)
    check(lib.kgcn_svm_vote_i32(ptr(dec1), total, ptr(d_jo), J, *eval_sets.args(), ptr(d_vf), ptr(d_ve), ptr(d_vo), V, classes, ptr(labels),
                                G, ptr(pred), ptotal, ptr(counts), ptr(counts[V:]), current_stream()), "kgcn_svm_vote_i32")
    if check_errors:
        _svm_refuse_errors(counts[V], who)
    return pred[:ptotal], vote_out, counts


# -------------------------------------------------------------------------------------------------
# active learning (csrc/labelprop.hip; the driver is kgcn_amd/active_learning.py): one RBF affinity matrix for every task and
# every query over the same points, label propagation / spreading for all tasks in one sweep over it, uncertainty scores and
# the pick on the device.  fp64 and integers, stated summation orders (include/kgcn_hip.h): bitwise reproducible.  The matrix
# need not be stored: rbf_apply / rbf_degrees / lp_propagate_free rebuild its tiles where they are consumed, with the same bits.
# -------------------------------------------------------------------------------------------------
LP_MAX_ROWS, LP_MAX_TASKS, LP_MAX_COLS, LP_BLOCK_ROWS, LP_MAX_PICKS, LP_DEFAULT_CHECK = (_lib.K["KGCN_LP_" + n] for n in (
    "MAX_ROWS", "MAX_TASKS", "MAX_COLS", "BLOCK_ROWS", "MAX_PICKS", "DEFAULT_CHECK"))
LP_PROPAGATION, LP_SPREADING = _lib.K["KGCN_LP_PROPAGATION"], _lib.K["KGCN_LP_SPREADING"]
LP_RUNNING, LP_CONVERGED, LP_MAX_ITER = _lib.K["KGCN_LP_RUNNING"], _lib.K["KGCN_LP_CONVERGED"], _lib.K["KGCN_LP_MAX_ITER"]
LP_SCORES = {"E": _lib.K["KGCN_LP_SCORE_E"], "LC_MEAN": _lib.K["KGCN_LP_SCORE_LC_MEAN"], "MS_MEAN": _lib.K["KGCN_LP_SCORE_MS_MEAN"],
             "LC_TASKS": _lib.K["KGCN_LP_SCORE_LC_TASKS"], "MS_TASKS": _lib.K["KGCN_LP_SCORE_MS_TASKS"]}
LP_DEFAULT_MAX_BYTES = 16 << 30      # the affinity matrix of 46,340 points


_LP_MATRIX = ((1, LP_MAX_ROWS), _SAME)


def _lp_task_col(task_col, who):
    import numpy as np
    tc = np.asarray(task_col, np.int64).reshape(-1)
    T = tc.shape[0] - 1
    if T < 1 or T > LP_MAX_TASKS or tc[0] != 0 or np.any(np.diff(tc) < 1) or tc[-1] > LP_MAX_COLS:
        raise _lib.KgcnHipError("%s: task_col must ascend from 0 over 1..%d tasks of at least one class each, up to %d columns in "
                                "all, got %s" % (who, LP_MAX_TASKS, LP_MAX_COLS, tc.tolist()))
    return tc.astype(np.int32), T, int(tc[-1])


@torch.no_grad()
def rbf_affinity(X, gamma, max_bytes=LP_DEFAULT_MAX_BYTES):
    """X [n, d] float64 on the device -> W [n, n] = exp(-gamma max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)) (sklearn's rbf_kernel), the dot
    products on the fp64 matrix pipe; symmetric bit for bit, unit diagonal.  Refused before any launch: a matrix of more than
    max_bytes bytes, more than LP_MAX_ROWS points, a gamma that is not positive and finite, an X that is not finite."""
    who = "rbf_affinity"
    n, d = _operand(who, "X", X, torch.float64, ((1, None), (1, None))).shape
    gamma, max_bytes = float(gamma), int(max_bytes)
    if n > LP_MAX_ROWS or n * n * 8 > max_bytes:
        raise _lib.KgcnHipError("%s: the %d x %d affinity matrix takes %d bytes, over max_bytes = %d (or over %d points); refused "
                                "before any launch" % (who, n, n, n * n * 8, max_bytes, LP_MAX_ROWS))
    if not 0.0 < gamma < float("inf"):
        raise _lib.KgcnHipError("%s: gamma must be positive and finite, got %r" % (who, gamma))
    if not bool(torch.isfinite(X).all()):
        raise _lib.KgcnHipError("%s: X holds values that are not finite; refused before any launch" % who)
    W = torch.empty((n, n), device=X.device, dtype=torch.float64)
    norms = torch.empty((n,), device=X.device, dtype=torch.float64)
    check(lib.kgcn_rbf_affinity_f64(ptr(X), n, d, ctypes.byref(ctypes.c_double(gamma)), max_bytes, ptr(W), ptr(norms),
                                    current_stream()), "kgcn_rbf_affinity_f64")
    return W


@torch.no_grad()
def lp_degrees(W):
    """-> (s, d) [n] float64: s_i = sum_j W_ij (LabelPropagation's normaliser) and d_i = the same without the diagonal term (the degree
    of LabelSpreading's normed Laplacian); per row the columns j = l (mod 64) in ascending order, then the lane tree."""
    n = _operand("lp_degrees", "W", W, torch.float64, _LP_MATRIX).shape[0]
    out = torch.empty((2, n), device=W.device, dtype=torch.float64)
    check(lib.kgcn_lp_degrees_f64(ptr(W), n, ptr(out[0]), ptr(out[1]), current_stream()), "kgcn_lp_degrees_f64")
    return out[0], out[1]


def _lp_run(who, entry, front, n, labels, task_col, variant, alpha, tol, max_iter, iters_per_check, dev):
    """THE launch / read-back loop of lp_propagate and lp_propagate_free: `entry` is the C entry point, `front` its arguments
    before n (the matrix, or the points): both share everything from n on.  -> (dist, n_iter, status, words read back)."""
    tc, T, K = _lp_task_col(task_col, who)
    _operand(who, "labels", labels, torch.int32, (n, T))
    if variant not in (LP_PROPAGATION, LP_SPREADING):
        raise ValueError("%s: variant must be LP_PROPAGATION or LP_SPREADING" % who)
    alpha, tol, max_iter = float(alpha), float(tol), int(max_iter)
    ipc = LP_DEFAULT_CHECK if iters_per_check is None else int(iters_per_check)
    if variant == LP_SPREADING and not 0.0 < alpha < 1.0:
        raise ValueError("%s: alpha must lie in (0, 1), got %r" % (who, alpha))
    if not 0.0 <= tol < float("inf") or not 1 <= max_iter < 2 ** 30 or ipc < 1:
        raise ValueError("%s: tol %r, max_iter %r, iters_per_check %r" % (who, tol, max_iter, ipc))
    d_tc = torch.from_numpy(tc).to(dev)
    meta = torch.zeros((2, T), device=dev, dtype=torch.int32)           # n_iter | status
    dist = torch.empty((n, K), device=dev, dtype=torch.float64)
    ws, wsb = _ws_bytes(lib.kgcn_lp_workspace_bytes(n, T, K), "kgcn_lp_workspace_bytes", dev)
    word = _ws_word(ws)
    c_alpha, c_tol = ctypes.c_double(alpha), ctypes.c_double(tol)
    done = reads = 0
    while True:
        steps = min(ipc, max_iter - done)
        check(entry(*front, n, ptr(labels), ptr(d_tc), T, K, variant, ctypes.byref(c_alpha), ctypes.byref(c_tol), max_iter, done,
                    steps, ptr(meta[0]), ptr(meta[1]), ptr(ws), wsb, current_stream()), entry.__name__)
        done += steps
        reads += 1
        if int(word.item()) == 0:
            break
        if done >= max_iter:
            raise _lib.KgcnHipError("%s: tasks still running after max_iter = %d steps" % (who, max_iter))
    check(lib.kgcn_lp_finish_f64(n, ptr(d_tc), T, K, done, ptr(dist), ptr(ws), wsb, current_stream()), "kgcn_lp_finish_f64")
    return dist, meta[0], meta[1], reads


@torch.no_grad()
def lp_propagate(W, scale, labels, task_col, variant, alpha=0.2, tol=1e-3, max_iter=1000, iters_per_check=None):
    """Label propagation (variant LP_PROPAGATION, scale = s of lp_degrees) or spreading (LP_SPREADING, scale = d) of all tasks at
    once over W: labels [n, T] int32 on the device (class index inside the task, -1 = unlabelled), task_col [T + 1] on the host.
    -> (dist [n, K] float64: the normalised label distributions, task t in columns task_col[t]:task_col[t + 1]; n_iter [T] and
    status [T] int32, all on the device; the number of words read back).  Each task runs until its sum |F' - F| < tol
    (LP_CONVERGED) or for max_iter steps (LP_MAX_ITER, n_iter = max_iter, as scikit-learn warns and goes on); a finished task
    is frozen.  One word is read back per iters_per_check steps (default LP_DEFAULT_CHECK); the grouping changes no bit."""
    who = "lp_propagate"
    n = _operand(who, "W", W, torch.float64, _LP_MATRIX).shape[0]
    _operand(who, "scale", scale, torch.float64, (n,))
    return _lp_run(who, lib.kgcn_lp_propagate_f64, (ptr(W), ptr(scale)), n, labels, task_col, variant, alpha, tol, max_iter,
                   iters_per_check, W.device)


# ---- the same without a stored W: every tile of it is rebuilt from the points where it is consumed, bit for bit ----------------
def _lp_points(who, name, X, gamma, rows=(1, LP_MAX_ROWS)):
    """-> (rows, d, gamma) of a point set; refused before any launch: a shape out of range, a gamma that is not positive and finite,
    values that are not finite."""
    n, d = _operand(who, name, X, torch.float64, (rows, (1, None))).shape
    gamma = float(gamma)
    if not 0.0 < gamma < float("inf"):
        raise _lib.KgcnHipError("%s: gamma must be positive and finite, got %r" % (who, gamma))
    if not bool(torch.isfinite(X).all()):
        raise _lib.KgcnHipError("%s: %s holds values that are not finite; refused before any launch" % (who, name))
    return n, d, gamma


@torch.no_grad()
def rbf_apply(Xq, Xr, gamma, G, same_set=False, zero_diagonal=False):
    """out [m, K] = sum_j w(q_i, r_j) G_jc with w the entries rbf_affinity would store, for queries Xq [m, d], references Xr [n, d]
    (n <= LP_MAX_ROWS; m is not bounded) and G [n, K], K <= LP_MAX_COLS, without forming the [m, n] kernel: per (i, c) lane l adds
    the rounded products of j = l (mod 64) in ascending order, then the lane tree (lp_propagate's product).  same_set: Xq is Xr
    (the same tensor), the diagonal distance is 0 and zero_diagonal counts w_ii as +0.0."""
    who = "rbf_apply"
    n, d, gamma = _lp_points(who, "Xr", Xr, gamma)
    K = _operand(who, "G", G, torch.float64, (n, (1, LP_MAX_COLS))).shape[1]
    if same_set:
        if Xq is not Xr and (Xq.data_ptr() != Xr.data_ptr() or Xq.shape != Xr.shape):
            raise ValueError("%s: same_set takes one tensor as Xq and Xr" % who)
        Xq, m = Xr, n
    else:
        if zero_diagonal:
            raise ValueError("%s: zero_diagonal takes same_set" % who)
        m = _lp_points(who, "Xq", Xq, gamma, (1, None))[0]
        _operand(who, "Xq", Xq, torch.float64, (m, d))
    out = torch.empty((m, K), device=Xr.device, dtype=torch.float64)
    norms = torch.empty((n + (0 if same_set else m),), device=Xr.device, dtype=torch.float64)
    check(lib.kgcn_rbf_apply_f64(ptr(Xq), m, ptr(Xr), n, d, ctypes.byref(ctypes.c_double(gamma)), ptr(G), K, 1 if same_set else 0,
                                 1 if zero_diagonal else 0, ptr(out), _ptr_if(norms[n:], 0 if same_set else m), ptr(norms[:n]),
                                 current_stream()), "kgcn_rbf_apply_f64")
    return out


@torch.no_grad()
def rbf_degrees(X, gamma):
    """lp_degrees(rbf_affinity(X, gamma)) without the matrix: -> (s, d) [n] float64, the same bits."""
    n, d, gamma = _lp_points("rbf_degrees", "X", X, gamma)
    out = torch.empty((3, n), device=X.device, dtype=torch.float64)      # s | d | the squared norms
    check(lib.kgcn_rbf_degrees_f64(ptr(X), n, d, ctypes.byref(ctypes.c_double(gamma)), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                   current_stream()), "kgcn_rbf_degrees_f64")
    return out[0], out[1]


@torch.no_grad()
def lp_propagate_free(X, gamma, scale, labels, task_col, variant, alpha=0.2, tol=1e-3, max_iter=1000, iters_per_check=None):
    """lp_propagate over the affinity matrix of X [n, d] without storing it (scale = s or d of rbf_degrees): the same return values,
    the same bits, O(n (d + K)) memory; every step rebuilds the tiles of W on the matrix pipe."""
    who = "lp_propagate_free"
    n, d, gamma = _lp_points(who, "X", X, gamma)
    _operand(who, "scale", scale, torch.float64, (n,))
    norms = torch.empty((n,), device=X.device, dtype=torch.float64)
    c_gamma = ctypes.c_double(gamma)
    return _lp_run(who, lib.kgcn_lp_propagate_free_f64, (ptr(X), d, ctypes.byref(c_gamma), ptr(norms), ptr(scale)), n, labels,
                   task_col, variant, alpha, tol, max_iter, iters_per_check, X.device)


@torch.no_grad()
def lp_scores(dist, task_col, cand):
    """Uncertainty scores of the rows cand [m] (int32, device) of dist [n, K] -> [5, m] float64, row LP_SCORES[name]: "E" the entropy
    summed over tasks; "LC_MEAN" / "MS_MEAN" least confidence and margin of the mean distribution over tasks
    (query_next_data_points; NaN unless all tasks have the same number of classes); "LC_TASKS" / "MS_TASKS" the mean of the
    tasks' maxima and the sum of their margins (ActiveLearner.query)."""
    who = "lp_scores"
    tc, T, K = _lp_task_col(task_col, who)
    n = _operand(who, "dist", dist, torch.float64, ((1, LP_MAX_ROWS), K)).shape[0]
    m = int(_operand(who, "cand", cand, torch.int32, (None,)).numel())
    scores = torch.empty((5, m), device=dist.device, dtype=torch.float64)
    d_tc = torch.from_numpy(tc).to(dist.device)
    check(lib.kgcn_lp_scores_f64(ptr(dist), n, ptr(d_tc), T, K, ptr(cand), m, ptr(scores), current_stream()),
          "kgcn_lp_scores_f64")
    return scores


@torch.no_grad()
def lp_select(score, cand, n, k, largest, active=None, labels=None, truth=None, log=None):
    """The k picks among the candidates cand [m] (rows of an n-row problem) by score [m] -> out [k] int32 positions into cand (-1
    where fewer take part), in the order of a STABLE ascending sort with NaN last: its last k entries (largest) or its first k.
    active [n] int32: rows with 0 take no part.  truth [n, T] (k = 1): the picked row is taught on the device -- labels[row] =
    truth[row], active[row] = 0, log[0] = the position -- so a query-and-teach loop needs no read-back for it."""
    who = "lp_select"
    m, n, k = int(_operand(who, "cand", cand, torch.int32, (None,)).numel()), int(n), int(k)
    _operand(who, "score", score, torch.float64, (m,))
    if not 1 <= k <= LP_MAX_PICKS or not 1 <= n <= LP_MAX_ROWS:
        raise _lib.KgcnHipError("%s: %d picks (1..%d) among rows of %d" % (who, k, LP_MAX_PICKS, n))
    if active is not None:
        _operand(who, "active", active, torch.int32, (n,))
    T = 0
    if truth is not None:
        if k != 1 or labels is None or truth.dim() != 2:
            raise _lib.KgcnHipError("%s: teaching takes the single pick (k = 1), labels and truth [n, T]" % who)
        T = int(truth.shape[1])
        _operand(who, "truth", truth, torch.int32, (n, T)), _operand(who, "labels", labels, torch.int32, (n, T))
        if log is not None:
            _operand(who, "log", log, torch.int32, (1,))
    out = torch.empty((k,), device=cand.device, dtype=torch.int32)
    check(lib.kgcn_lp_select_f64(ptr(score), ptr(cand), m, n, ptr(active), k, 1 if largest else 0, ptr(out),
                                 ptr(labels if truth is not None else None), ptr(truth), T, ptr(log), current_stream()),
          "kgcn_lp_select_f64")
    return out
