"""The Conv1D + max-pool kernels (csrc/conv1d.hip) through ops.conv1d_pool against the fp64 oracle tests/seqcnn_oracle.py fed the
same fp32-rounded inputs: forward, dX, dW, dbias and d table, at the smallest shapes at which each mechanism can go wrong (a
reduction that is no multiple of the MFMA depth or spans several LDS chunks, one filter and a ragged filter tile, even and odd
same-padding, L < k, L no multiple of pool, more than one position tile with the tile edge inside a sequence, several sequences
in a launch, both input modes, relu and tanh).

Error figure: max |err| / max |ref| per tensor; bounds from tests/golden/seqcnn_bounds.json (ten times the largest figure
measured over these cases on an MI355X, the project's rule; the measured values are stored beside them;
KGCN_SEQCNN_RECORD=<file> writes the errors of a run, of this file and of test_gpu_seqcnn.py).  Max-pooling and relu
can route differently in fp32 and fp64 where two candidates of a window, or a pre-activation and zero, are closer than the
arithmetic error: before any comparison the test asserts, on the oracle's fp64 values, that every pre-activation of a relu layer
is farther from zero, and the two largest distinct candidates of every window farther apart, than the forward bound times the
largest pre-activation.  The inputs of a case are drawn from the first seed at or after the case's base seed for which that
holds (a CPU search over the oracle alone)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_bounds  # noqa: E402
import seqcnn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

# FB.check: max|got - ref| / max|ref| (0 where there is nothing to compare, absolute where ref is all zero), held to the stored bound
FB = family_bounds.FAMILIES["seqcnn"]

# B, L, Cin, F, k, pool, act, token mode
CASES = [
    (1, 26, 25, 33, 4, 4, "relu", True),       # the model's first layer in small: Cin < one chunk, ragged filter tile
    (3, 150, 37, 70, 3, 3, "relu", False),     # two chunks, two filter tiles, three position tiles (63 rows each), L % pool == 0
    (3, 150, 70, 33, 2, 2, "tanh", False),     # three chunks, even k, tanh
    (1, 150, 1, 1, 4, 1, "tanh", False),       # one channel, one filter, no pooling: the model's last layer
    (3, 26, 1, 70, 3, 4, "relu", True),        # L % pool != 0: positions 24, 25 outside every window
    (3, 3, 25, 33, 4, 2, "relu", False),       # L < k
    (3, 1, 37, 1, 2, 1, "tanh", True),         # L = 1
    (1, 3, 70, 70, 4, 4, "relu", False),       # L < pool: no pooled output, zero gradients
    (3, 150, 25, 70, 4, 4, "relu", True),      # token mode over several tiles and sequences
    (1, 150, 37, 33, 3, 2, "tanh", True),
]


def _draw(seed, B, L, Cin, F, k, token):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((k, Cin, F)) / np.sqrt(k * Cin)).astype(np.float32)
    b = (0.3 * rng.standard_normal(F)).astype(np.float32)
    if token:
        S = 26
        src = dict(tokens=rng.integers(0, S - 2, (B, L)).astype(np.int32), table=rng.standard_normal((S, Cin)).astype(np.float32))
    else:
        src = dict(x=rng.standard_normal((B, L, Cin)).astype(np.float32))
    g = rng.standard_normal((B, L // 1, F)).astype(np.float32)
    return w, b, src, g


def well_conditioned(c, bound):
    """The flip precondition on a forward cache (see the module docstring) -> (ok, near_zero, gap, margin)."""
    T = c["pre"].shape[1] // c["pool"]
    if T == 0:
        return True, np.inf, np.inf, 0.0
    margin = bound * float(np.abs(c["pre"]).max())
    near_zero, gap = O.window_margins(c)
    return near_zero > margin and gap > margin, near_zero, gap, margin


def make_case(idx):
    B, L, Cin, F, k, pool, act, token = CASES[idx]
    for seed in range(1000 * idx, 1000 * idx + 50):
        w, b, src, g = _draw(seed, B, L, Cin, F, k, token)
        g = g[:, :L // pool]
        c = O.conv1d_pool_fwd(w, b, pool, act, **src)
        ok, near_zero, gap, margin = well_conditioned(c, FB.bound("forward"))
        if ok:
            return w, b, src, g, c, (near_zero, gap, margin)
    raise AssertionError("no well-conditioned seed for case %d" % idx)


def run(w, b, src, g, pool, act):
    import torch
    from kgcn_amd import ops
    dev = torch.device("cuda:0")
    tw, tb = (torch.as_tensor(v, device=dev).requires_grad_(True) for v in (w, b))
    if "tokens" in src:
        tx = None
        tt = torch.as_tensor(src["table"], device=dev).requires_grad_(True)
        out = ops.conv1d_pool(None, tw, tb, pool, act, tokens=torch.as_tensor(src["tokens"], device=dev), table=tt)
    else:
        tt = None
        tx = torch.as_tensor(src["x"], device=dev).requires_grad_(True)
        out = ops.conv1d_pool(tx, tw, tb, pool, act)
    out.backward(torch.as_tensor(g, device=dev))
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu().numpy(), dw=tw.grad.cpu().numpy(), db=tb.grad.cpu().numpy())
    if tx is not None:
        res["dx"] = tx.grad.cpu().numpy()
    else:
        res["dtable"] = tt.grad.cpu().numpy()
    return res


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["B%d-L%d-Cin%d-F%d-k%d-p%d-%s-%s" % (c[:7] + ("tok" if c[7] else "dense",))
                                                        for c in CASES])
def test_conv1d_pool_against_the_oracle(idx):
    B, L, Cin, F, k, pool, act, token = CASES[idx]
    w, b, src, g, c, (near_zero, gap, margin) = make_case(idx)
    assert near_zero > margin and gap > margin                 # the flip precondition, on the oracle's fp64 values
    ref = O.conv1d_pool_bwd(c, g)
    a, again = run(w, b, src, g, pool, act), run(w, b, src, g, pool, act)
    assert a["out"].shape == (B, L // pool, F)
    FB.check("forward", a["out"], c["out"])
    FB.check("dw", a["dw"], ref["dw"])
    FB.check("dbias", a["db"], ref["db"])
    if token:
        FB.check("dtable", a["dtable"], ref["dtable"])
        unused = np.setdiff1d(np.arange(src["table"].shape[0]), src["tokens"])
        assert len(unused) >= 2 and not a["dtable"][unused].any()          # rows of unused symbols are exactly zero
    else:
        FB.check("dx", a["dx"], ref["dx"])
        dead = L // pool * pool + O.same_padding(k)[1]                         # input rows no pooled window reaches
        assert not a["dx"][:, dead:].any()
    for key in a:                                                             # two identical calls: identical bits
        assert a[key].tobytes() == again[key].tobytes(), key


def test_embedding_grad():
    """ops.embedding_grad alone: d table from a given d embedded, rows of unused symbols exactly zero, bitwise repeatable."""
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(77)
    B, L, S, E = 3, 150, 26, 37
    tokens = rng.integers(0, S - 3, (B, L)).astype(np.int32)
    d = rng.standard_normal((B, L, E)).astype(np.float32)
    dev = torch.device("cuda:0")
    tt, td = torch.as_tensor(tokens, device=dev), torch.as_tensor(d, device=dev)
    a, again = ops.embedding_grad(tt, td, S).cpu().numpy(), ops.embedding_grad(tt, td, S).cpu().numpy()
    ref = O.embedding_grad(tokens, d, S)
    assert not a[S - 3:].any() and a.tobytes() == again.tobytes()
    FB.check("dtable", a, ref, "embedding_grad")


@pytest.mark.parametrize("shape", [
    dict(L=8193), dict(Cin=1025), dict(F=1025), dict(k=9), dict(pool=9), dict(S=1025)])
def test_every_limit_plus_one_is_refused(shape):
    """KgcnHipError from the argument checks; nothing is launched (the tensors are never read: `out` is not even allocated)."""
    import torch
    from kgcn_amd import _lib, ops
    dev = torch.device("cuda:0")
    L, Cin, F, k, pool, S = (shape.get(n, d) for n, d in (("L", 8), ("Cin", 3), ("F", 4), ("k", 2), ("pool", 2), ("S", None)))
    w, b = torch.zeros((k, Cin, F), device=dev), torch.zeros(F, device=dev)
    with pytest.raises(_lib.KgcnHipError):
        if S is None:
            ops.conv1d_pool(torch.zeros((1, L, Cin), device=dev), w, b, pool, "relu")
        else:
            ops.conv1d_pool(None, w, b, pool, "relu", tokens=torch.zeros((1, L), device=dev, dtype=torch.int32),
                            table=torch.zeros((S, Cin), device=dev))
    # the same shape handed to the C ABI directly is refused there as well, before any launch
    one = _lib.ptr(w)
    rc = _lib.lib.kgcn_conv1d_pool_fwd_f32(None if S else one, one if S else None, one if S else None, S or 0, 1, L, Cin, one, one, k, F,
                                           pool, 2, one, None, _lib.current_stream())
    assert rc != 0 and _lib.lib.kgcn_last_error()
    torch.cuda.synchronize()


def test_argument_checks():
    import torch
    from kgcn_amd import _lib, ops
    dev = torch.device("cuda:0")
    w, b, x = torch.zeros((2, 3, 4), device=dev), torch.zeros(4, device=dev), torch.zeros((1, 8, 3), device=dev)
    tok, tab = torch.zeros((1, 8), device=dev, dtype=torch.int32), torch.zeros((5, 3), device=dev)
    for bad in (lambda: ops.conv1d_pool(x, w, b, 2, "sigmoid"), lambda: ops.conv1d_pool(x, w, b, 2, "relu", tokens=tok, table=tab),
                lambda: ops.conv1d_pool(None, w, b, 2, "relu", tokens=tok), lambda: ops.conv1d_pool(x[:, :, :2], w, b, 2, "relu"),
                lambda: ops.conv1d_pool(x, w, b[:3], 2, "relu"), lambda: ops.conv1d_pool(None, w, b, 2, "relu", tokens=tok.long(), table=tab),
                lambda: ops.conv1d_pool(x.cpu(), w, b, 2, "relu")):
        with pytest.raises(_lib.KgcnHipError):
            bad()
