"""CPU checks of the protein-sequence CNN's oracle (tests/seqcnn_oracle.py), fixture and ABI; no GPU needed.

  * the vectorised Conv1D + max-pool equals the plain loop transcription (both input modes, relu / tanh / none, even and odd k);
  * its gradients, and the whole model's, equal central differences in fp64;
  * the loss equals cnn.py:84-90 evaluated literally at B = 1 (the one batch size at which the reference's broadcast is defined);
  * include/kgcn_hip.h declares the new entry points, kgcn_amd._lib binds exactly those, and a shape beyond a limit is refused by
    the library before any launch;
  * the committed fixture is what tests/golden/make_golden_seqcnn.py writes.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import seqcnn_oracle as O  # noqa: E402

NEW_SYMBOLS = ("kgcn_conv1d_pool_workspace_bytes", "kgcn_conv1d_pool_fwd_f32", "kgcn_conv1d_pool_bwd_f32", "kgcn_embedding_grad_f32")


def _case(rng, B, L, Cin, F, k, token_mode, S=7):
    w, b = rng.standard_normal((k, Cin, F)), rng.standard_normal(F)
    if token_mode:
        return w, b, dict(tokens=rng.integers(0, S, (B, L)), table=rng.standard_normal((S, Cin)))
    return w, b, dict(x=rng.standard_normal((B, L, Cin)))


@pytest.mark.parametrize("B,L,Cin,F,k,pool,act,token_mode", [
    (2, 9, 3, 4, 4, 2, "relu", False), (2, 9, 3, 4, 3, 3, "tanh", True), (1, 7, 2, 3, 2, 1, "tanh", False),
    (3, 1, 2, 2, 3, 1, "relu", True), (2, 10, 1, 1, 5, 4, None, False), (1, 3, 2, 2, 4, 4, "relu", False)])
def test_vectorised_conv_pool_equals_the_loop(B, L, Cin, F, k, pool, act, token_mode):
    rng = np.random.default_rng(B * 100 + L)
    w, b, src = _case(rng, B, L, Cin, F, k, token_mode)
    c = O.conv1d_pool_fwd(w, b, pool, act, **src)
    out, arg = O.conv1d_pool_loop(w, b, pool, act, **src)
    assert c["out"].shape == (B, L // pool, F)
    np.testing.assert_allclose(c["out"], out, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(c["arg"], arg)


def test_same_padding_is_the_multimodal_oracles_rule():
    import multimodal_oracle as M
    for k in range(1, 9):
        assert O.same_padding(k) == M.same_padding(k)


def _central(fn, v, h=1e-6):
    g = np.zeros_like(v)
    it = np.nditer(v, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        old = v[i]
        v[i] = old + h
        up = fn()
        v[i] = old - h
        dn = fn()
        v[i] = old
        g[i] = (up - dn) / (2 * h)
    return g


@pytest.mark.parametrize("act,k,pool,token_mode", [("relu", 4, 2, False), ("tanh", 3, 3, True), ("relu", 2, 1, True), (None, 3, 2, False)])
def test_conv_pool_gradients_equal_central_differences(act, k, pool, token_mode):
    rng = np.random.default_rng(5)
    B, L, Cin, F = 2, 8, 3, 4
    w, b, src = _case(rng, B, L, Cin, F, k, token_mode)
    g = rng.standard_normal((B, L // pool, F))

    def f():
        return float((O.conv1d_pool_fwd(w, b, pool, act, **src)["out"] * g).sum())

    r = O.conv1d_pool_bwd(O.conv1d_pool_fwd(w, b, pool, act, **src), g)
    np.testing.assert_allclose(r["dw"], _central(f, w), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(r["db"], _central(f, b), rtol=1e-6, atol=1e-7)
    if token_mode:
        np.testing.assert_allclose(r["dtable"], _central(f, src["table"]), rtol=1e-6, atol=1e-7)
        unused = np.setdiff1d(np.arange(src["table"].shape[0]), src["tokens"])
        assert not r["dtable"][unused].any()
    else:
        np.testing.assert_allclose(r["dx"], _central(f, src["x"]), rtol=1e-6, atol=1e-7)


def test_positions_past_the_last_window_get_no_gradient():
    rng = np.random.default_rng(1)
    w, b, src = _case(rng, 1, 7, 2, 3, 1, False)            # k = 1: position l only reaches conv output l
    c = O.conv1d_pool_fwd(w, b, 3, "tanh", **src)
    r = O.conv1d_pool_bwd(c, rng.standard_normal((1, 2, 3)))
    assert not r["dx"][:, 6:].any() and r["dx"][:, :6].any()


@pytest.mark.parametrize("token_mode", [True, False])
def test_model_gradients_equal_central_differences(token_mode):
    rng = np.random.default_rng(11)
    B, L, S, E = 2, 48, 5, 3
    p = {k: v.astype(np.float64) for k, v in O.init_params(rng, S, E, L, widths=(6, 5, 4), hidden=3).items()}
    labels = np.eye(2)[rng.integers(0, 2, B)]
    cw, mask = np.array([1.5, 3.0]), np.array([1.0, 0.5])
    tokens = rng.integers(0, S, (B, L))
    emb = rng.standard_normal((B, L, E))
    kw = dict(tokens=tokens) if token_mode else dict(embedded=emb)

    def f():
        c = O.model_fwd(p, labels, cw, mask, **kw)
        return 0.7 * c["cost_opt"] + 0.3 * c["cost_sum"]

    g = O.model_bwd(O.model_fwd(p, labels, cw, mask, **kw), 0.7, 0.3)
    for name in O.PARAMS:
        if name == "embeddings" and not token_mode:
            continue
        np.testing.assert_allclose(g[name], _central(f, p[name]), rtol=2e-6, atol=1e-8, err_msg=name)
    if not token_mode:
        np.testing.assert_allclose(g["d_embedded"], _central(f, emb), rtol=2e-6, atol=1e-8)


def test_loss_equals_the_reference_expression_at_batch_one():
    rng = np.random.default_rng(2)
    for C in (2, 3):
        cw = rng.uniform(1, 5, C)
        for label in range(C):
            logits, labels = rng.standard_normal((1, C)), np.eye(C)[[label]]
            opt, tot, _ = O.loss(logits, labels, cw)
            ref_opt, ref_sum = O.loss_reference_literal(logits, labels, cw)
            assert abs(opt - ref_opt) <= 1e-14 * abs(ref_opt) and abs(tot - ref_sum) <= 1e-14 * abs(ref_sum)


def test_loss_mask_drops_padded_rows():
    rng = np.random.default_rng(3)
    logits, labels, cw = rng.standard_normal((3, 2)), np.eye(2)[[0, 1, 1]], np.array([1.2, 4.0])
    opt, tot, cost = O.loss(logits, labels, cw, mask=[1, 1, 0])
    assert abs(tot - cost[:2].sum()) < 1e-14
    assert abs(opt - (cost[0] * 1.2 + cost[1] * 4.0) / 6.0) < 1e-14


# ---- ABI and limits without a GPU ---------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_entry_points():
    from kgcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "kgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr), name
    bound = sorted(n for n in _lib.SIGNATURES if n.startswith("kgcn_conv1d") or n.startswith("kgcn_embedding"))
    assert bound == sorted(NEW_SYMBOLS)
    assert "#define KGCN_HIP_ABI_VERSION 2" in header
    from kgcn_amd import ops
    for macro, val in (("KGCN_CONV1D_MAX_CHANNELS", ops.CONV1D_MAX_CHANNELS), ("KGCN_CONV1D_MAX_KERNEL", ops.CONV1D_MAX_KERNEL),
                       ("KGCN_CONV1D_MAX_POOL", ops.CONV1D_MAX_POOL), ("KGCN_CONV1D_MAX_LENGTH", ops.CONV1D_MAX_LENGTH),
                       ("KGCN_CONV1D_MAX_SYMBOLS", ops.CONV1D_MAX_SYMBOLS)):
        assert "#define %s %d" % (macro, val) in header


@pytest.mark.parametrize("args", [
    (2, 8193, 25, 4, 50, 4), (2, 100, 1025, 4, 50, 4), (2, 100, 25, 9, 50, 4), (2, 100, 25, 4, 1025, 4), (2, 100, 25, 4, 50, 9),
    (2, 0, 25, 4, 50, 4), (2, 100, 0, 4, 50, 4), (2, 100, 25, 0, 50, 4), (2, 100, 25, 4, 0, 4), (2, 100, 25, 4, 50, 0)])
def test_shapes_beyond_the_limits_are_refused_by_the_library(args):
    """(batch, length, in_dim, kernel_size, filters, pool): validation precedes every launch, so this needs no GPU."""
    from kgcn_amd import _lib
    B, L, Cin, k, F, pool = args
    assert _lib.lib.kgcn_conv1d_pool_workspace_bytes(B, L, Cin, k, F, pool) == -1
    one = ctypes.c_void_p(16)                                # never dereferenced: the shape check comes first
    rc = _lib.lib.kgcn_conv1d_pool_fwd_f32(one, None, None, 0, B, L, Cin, one, one, k, F, pool, 2, one, None, None)
    assert rc != 0 and b"outside" in _lib.lib.kgcn_last_error()
    rc = _lib.lib.kgcn_conv1d_pool_bwd_f32(one, None, None, 0, B, L, Cin, one, k, F, pool, 2, one, one, one, one, one, one, one, 1 << 40,
                                           None)
    assert rc != 0 and b"outside" in _lib.lib.kgcn_last_error()


def test_bad_symbol_counts_and_activations_are_refused_by_the_library():
    from kgcn_amd import _lib
    one = ctypes.c_void_p(16)
    assert _lib.lib.kgcn_conv1d_pool_fwd_f32(None, one, one, 1025, 2, 100, 25, one, one, 4, 50, 4, 2, one, None, None) != 0
    assert b"symbols" in _lib.lib.kgcn_last_error()
    assert _lib.lib.kgcn_conv1d_pool_fwd_f32(one, None, None, 0, 2, 100, 25, one, one, 4, 50, 4, 1, one, None, None) != 0
    assert b"activation" in _lib.lib.kgcn_last_error()
    assert _lib.lib.kgcn_embedding_grad_f32(one, 2, 100, one, 1025, 25, one, None) != 0
    assert _lib.lib.kgcn_embedding_grad_f32(one, 2, 100, one, 26, 1025, one, None) != 0


def test_fixture_is_what_its_generator_writes():
    import make_golden_seqcnn as G
    z = np.load(os.path.join(ROOT, "tests", "golden", "g9_seqcnn.npz"))
    made = G.make()
    assert sorted(z.files) == sorted(made)
    for k in made:
        np.testing.assert_array_equal(z[k], made[k])
    seq, lab = z["sequence"], z["label"]
    assert seq.min() == 0 and seq.max() <= 25 and int(z["sequence_symbol_num"]) == seq.max() + 1
    for i in range(seq.shape[0]):                             # padded with 0 past the length; the motif marks class 1
        assert not seq[i, z["sequence_length"][i]:].any()
        assert (22 in seq[i]) == bool(lab[i, 1])
    v = lab.sum(axis=0)
    np.testing.assert_allclose(z["class_weight"], v.sum() / v)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g9_seqcnn.npz")) < 100 * 1024
