"""CPU tests of the multimodal model's fp64 oracle (tests/multimodal_oracle.py), the sequence loader and the new ABI symbols.
The oracle is held to a literal loop transcription and to finite differences; the TF semantics it restates (SAME padding,
go_backwards, hard_sigmoid edges, the pooling tie rule) are each pinned on a hand case."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_oracle as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g7_sample_multimodal.npz")
NEW_SYMBOLS = ("kgcn_seq_convpool_workspace_bytes", "kgcn_seq_convpool_fwd_f32", "kgcn_seq_convpool_bwd_f32",
               "kgcn_seq_lstm_stash_floats", "kgcn_seq_lstm_workspace_bytes", "kgcn_seq_lstm_fwd_f32", "kgcn_seq_lstm_bwd_f32",
               "kgcn_graph_gather_bwd_ld_f32")


# ---- hand cases ---------------------------------------------------------------------------------------------------------
def test_same_padding_is_one_left_two_right_for_k4():
    assert M.same_padding(4) == (1, 2)
    assert M.same_padding(3) == (1, 1)
    assert M.same_padding(1) == (0, 0)
    # identity embedding, E = 1: token value t at position l; kernel taps pick position l + dk - 1
    tok = np.array([[1, 2, 3, 4, 5]])
    table = np.arange(6, dtype=np.float64).reshape(6, 1)
    for dk, expect in ((0, [0, 1, 2, 3, 4]), (1, [1, 2, 3, 4, 5]), (2, [2, 3, 4, 5, 0]), (3, [3, 4, 5, 0, 0])):
        w = np.zeros((4, 1, 1))
        w[dk, 0, 0] = 1.0
        _, conv = M.conv_same(tok, table, w, np.zeros(1))
        assert conv[0, :, 0].tolist() == expect


def test_pooling_floor_and_lowest_index_tie_rule():
    tok = np.array([[1, 1, 1, 1, 2, 2, 2]])          # L = 7: T' = 1, positions 4..6 dropped
    table = np.array([[0.0], [1.0], [5.0]])
    w = np.zeros((4, 1, 1))
    w[1, 0, 0] = 1.0                                  # conv = embedding of the same position
    pooled, arg, _ = M.conv_pool_fwd(tok, table, w, np.zeros(1), 4)
    assert pooled.shape == (1, 1, 1) and pooled[0, 0, 0] == 1.0 and arg[0, 0, 0] == 0
    dtab, dw, db = M.conv_pool_bwd(tok, table, w, np.zeros(1), 4, np.ones((1, 1, 1)))
    assert db[0] == 1.0 and dtab[1, 0] == 1.0 and dtab[2, 0] == 0.0        # one routed position, not four
    # all padding: relu(0) = 0 everywhere, the routed position passes no gradient
    tok0 = np.zeros((1, 8), np.int64)
    pooled, arg, _ = M.conv_pool_fwd(tok0, table, w, np.zeros(1), 4)
    assert np.all(pooled == 0) and np.all(arg == 0)
    assert not np.any(M.conv_pool_bwd(tok0, table, w, np.zeros(1), 4, np.ones((1, 2, 1)))[0])
    assert M.conv_pool_fwd(np.zeros((2, 3), np.int64), table, w, np.zeros(1), 4)[0].shape == (2, 0, 1)


def test_hard_sigmoid_edges_pass_the_gradient():
    z = np.array([-3.0, -2.5, -1.0, 0.0, 2.5, 3.0])
    assert M.hard_sigmoid(z).tolist() == [0.0, 0.0, 0.3, 0.5, 1.0, 1.0]
    assert M.hard_sigmoid_grad(z).tolist() == [0.0, 0.2, 0.2, 0.2, 0.2, 0.0]


def test_go_backwards_processes_the_last_step_first_and_returns_h_after_step_0():
    # D = H = 1, only the input gate path: a sequence and its reverse give different outputs, and the output equals a forward
    # LSTM over the reversed sequence
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 5, 1))
    wx, wh, b = rng.standard_normal((1, 4)), rng.standard_normal((1, 4)), rng.standard_normal(4)
    h = M.lstm_fwd(x, wx, wh, b)[0]
    # forward-order reference written out by hand
    hh, cc = 0.0, 0.0
    for t in (4, 3, 2, 1, 0):
        z = x[0, t, 0] * wx[0] + hh * wh[0] + b
        i, f, g, o = M.hard_sigmoid(z[0]), M.hard_sigmoid(z[1]), np.tanh(z[2]), M.hard_sigmoid(z[3])
        cc = f * cc + i * g
        hh = o * np.tanh(cc)
    assert np.isclose(h[0, 0], hh, rtol=0, atol=1e-15)
    assert not np.isclose(M.lstm_fwd(x[:, ::-1], wx, wh, b)[0][0, 0], hh)


# ---- the oracle against a loop transcription and finite differences -----------------------------------------------------
@pytest.mark.parametrize("L,k,pool", [(9, 4, 4), (7, 3, 2), (3, 4, 4), (12, 5, 3)])
def test_conv_pool_against_loop(L, k, pool):
    rng = np.random.default_rng(L * k)
    tok = rng.integers(0, 5, size=(3, L))
    table, w, b = rng.standard_normal((5, 3)), rng.standard_normal((k, 3, 4)), rng.standard_normal(4)
    assert np.allclose(M.conv_pool_fwd(tok, table, w, b, pool)[0], M.conv_pool_loop(tok, table, w, b, pool), rtol=0, atol=1e-12)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_lstm_against_loop(act):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 6, 3))
    wx, wh, b = rng.standard_normal((3, 8)), rng.standard_normal((2, 8)), rng.standard_normal(8)
    assert np.allclose(M.lstm_fwd(x, wx, wh, b, act)[0], M.lstm_loop(x, wx, wh, b, act), rtol=0, atol=1e-12)


# the corners of the shape box of include/kgcn_hip.h that tests/test_gpu_seq_shapes.py holds the kernels to, at small B and L
CONV_CORNERS = [(9, k, pool, E, F) for k in (1, 8) for pool in (1, 8) for E in (1, 32) for F in (1, 64)] + \
               [(5, 8, 1, 3, 4), (5, 8, 2, 32, 1), (6, 7, 3, 2, 5), (5, 4, 8, 3, 4)]      # k > L; odd k; pool > L (T' = 0)


@pytest.mark.parametrize("L,k,pool,E,F", CONV_CORNERS)
def test_conv_pool_against_loop_at_the_corner_shapes(L, k, pool, E, F):
    rng = np.random.default_rng([L, k, pool, E, F])
    tok = rng.integers(0, 5, size=(2, L))
    table, w, b = rng.standard_normal((5, E)), rng.standard_normal((k, E, F)), rng.standard_normal(F)
    out = M.conv_pool_fwd(tok, table, w, b, pool)[0]
    assert out.shape == (2, L // pool, F)
    assert np.allclose(out, M.conv_pool_loop(tok, table, w, b, pool), rtol=0, atol=1e-12)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("D,H", [(D, H) for D in (1, 64) for H in (1, 17, 64)])
def test_lstm_against_loop_at_the_corner_shapes(D, H, act):
    rng = np.random.default_rng([D, H])
    x = rng.standard_normal((2, 3, D))
    wx, wh, b = rng.standard_normal((D, 4 * H)) * 0.3, rng.standard_normal((H, 4 * H)) * 0.3, rng.standard_normal(4 * H)
    assert np.allclose(M.lstm_fwd(x, wx, wh, b, act)[0], M.lstm_loop(x, wx, wh, b, act), rtol=0, atol=1e-12)


def test_fp32_evaluation_is_the_same_expressions_in_fp32():
    """dtype=np.float32 (the yardstick of the GPU shape sweep): fp32 results throughout, within fp32 rounding of the fp64 ones."""
    rng = np.random.default_rng(8)
    f32 = np.float32
    tok = rng.integers(0, 9, size=(3, 40))
    table, w, b = rng.standard_normal((9, 5)).astype(f32), (rng.standard_normal((3, 5, 6)) * 0.4).astype(f32), rng.standard_normal(6).astype(f32)
    g = rng.standard_normal((3, 10, 6)).astype(f32)
    pairs = [(M.conv_pool_fwd(tok, table, w, b, 4, f32)[0], M.conv_pool_fwd(tok, table, w, b, 4)[0])]
    pairs += list(zip(M.conv_pool_bwd(tok, table, w, b, 4, g, f32), M.conv_pool_bwd(tok, table, w, b, 4, g)))
    wx, wh, bias = (rng.standard_normal(s).astype(f32) * f32(0.3) for s in ((6, 28), (7, 28), (28,)))
    gh = rng.standard_normal((3, 7)).astype(f32)
    for act in ("hard_sigmoid", "sigmoid"):
        h32, c32 = M.lstm_fwd(pairs[0][0], wx, wh, bias, act, f32)
        h64, c64 = M.lstm_fwd(pairs[0][0], wx, wh, bias, act)
        pairs += [(h32, h64)] + list(zip(M.lstm_bwd(c32, gh), M.lstm_bwd(c64, gh)))
    for a32, a64 in pairs:
        assert a32.dtype == np.float32 and a64.dtype == np.float64 and a32.shape == a64.shape
        err = np.abs(a32 - a64).max() / np.abs(a64).max()
        assert 0 < err < 1e-5, err


def test_hard_sigmoid_edges_in_fp32_and_fp64():
    """What the device test of the clip edges relies on.  0.2 z + 0.5 at z = +-2.5 is exactly 1 / 0 in fp32 and in fp64, so the
    kernel and the oracle stand on the same side.  The float above 2.5 does NOT separate in fp32: 0.2f z rounds to 0.5 + 2^-24
    and the sum 1 + 2^-24 is a tie that rounds to 1, while fp64 gives y > 1 -- a derivative mask taken from the rounded fp32 y
    passes a gradient there.  The kernel's rec_act_grad therefore tests z itself, which this pins as equivalent to the oracle."""
    f32 = np.float32
    up, lo = f32(2.5), f32(-2.5)
    above, below = np.nextafter(up, f32(3)), np.nextafter(lo, f32(-3))
    under, over = np.nextafter(up, f32(0)), np.nextafter(lo, f32(0))
    assert f32(0.2) * up + f32(0.5) == f32(1.0) and 0.2 * float(up) + 0.5 == 1.0
    assert f32(0.2) * lo + f32(0.5) == f32(0.0) and 0.2 * float(lo) + 0.5 == 0.0
    assert f32(0.2) * above + f32(0.5) == f32(1.0) and 0.2 * float(above) + 0.5 > 1.0          # the fp32 tie
    assert f32(0.2) * below + f32(0.5) < 0 and 0.2 * float(below) + 0.5 < 0.0
    z = np.array([below, lo, over, under, up, above], f32)
    assert M.hard_sigmoid_grad(z).tolist() == [0.0, 0.2, 0.2, 0.2, 0.2, 0.0]
    assert (M.hard_sigmoid_grad(z) != 0).tolist() == ((z >= lo) & (z <= up)).tolist()          # the kernel's test on z
    assert M.hard_sigmoid(z).tolist()[:2] == [0.0, 0.0] and M.hard_sigmoid(z).tolist()[-2:] == [1.0, 1.0]


def _fd(f, a, eps=1e-6, n=12, rng=None):
    """central differences of scalar f at n random entries of array a (in place) -> (indices, values)."""
    rng = rng or np.random.default_rng(0)
    idx = [tuple(int(rng.integers(0, s)) for s in a.shape) for _ in range(n)]
    out = []
    for i in idx:
        old = a[i]
        a[i] = old + eps
        fp = f()
        a[i] = old - eps
        fm = f()
        a[i] = old
        out.append((fp - fm) / (2 * eps))
    return idx, np.array(out)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
def test_encoder_gradients_against_finite_differences(act):
    rng = np.random.default_rng(2)
    B, L, S, E = 3, 13, 6, 3
    tok = rng.integers(0, S, size=(B, L))
    tok[0, 8:] = 0
    table, w, b = rng.standard_normal((S, E)), rng.standard_normal((4, E, 5)) * 0.5, rng.standard_normal(5) * 0.1
    wx, wh, bias = rng.standard_normal((5, 16)) * 0.4, rng.standard_normal((4, 16)) * 0.4, rng.standard_normal(16) * 0.3
    gh = rng.standard_normal((B, 4))

    def loss():
        pooled = M.conv_pool_fwd(tok, table, w, b, 4)[0]
        return float((M.lstm_fwd(pooled, wx, wh, bias, act)[0] * gh).sum())

    pooled = M.conv_pool_fwd(tok, table, w, b, 4)[0]
    h, cache = M.lstm_fwd(pooled, wx, wh, bias, act)
    dx, dwx, dwh, dbias = M.lstm_bwd(cache, gh)
    dtab, dw, db = M.conv_pool_bwd(tok, table, w, b, 4, dx)
    for arr, grad in ((table, dtab), (w, dw), (b, db), (wx, dwx), (wh, dwh), (bias, dbias)):
        idx, num = _fd(loss, arr)
        ana = np.array([grad[i] for i in idx])
        assert np.allclose(ana, num, rtol=1e-5, atol=1e-7), (ana, num)


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("L,E,k,F,pool,H", [(6, 1, 1, 1, 1, 1), (17, 32, 8, 64, 8, 64), (5, 3, 8, 5, 1, 17), (9, 32, 1, 1, 8, 17),
                                            (9, 1, 8, 64, 1, 1)])
def test_encoder_gradients_against_finite_differences_at_the_corner_shapes(L, E, k, F, pool, H, act):
    rng = np.random.default_rng([L, E, k, F, pool, H])
    B, S = 2, 6
    tok = rng.integers(0, S, size=(B, L))
    table, w, b = rng.standard_normal((S, E)), rng.standard_normal((k, E, F)) / np.sqrt(k * E), rng.standard_normal(F) * 0.1 + 0.2
    wx, wh = rng.standard_normal((F, 4 * H)) * 0.4 / np.sqrt(F), rng.standard_normal((H, 4 * H)) * 0.4 / np.sqrt(H)
    bias = rng.standard_normal(4 * H) * 0.3
    gh = rng.standard_normal((B, H))

    def loss():
        pooled = M.conv_pool_fwd(tok, table, w, b, pool)[0]
        return float((M.lstm_fwd(pooled, wx, wh, bias, act)[0] * gh).sum())

    pooled = M.conv_pool_fwd(tok, table, w, b, pool)[0]
    assert pooled.shape == (B, L // pool, F) and L // pool >= 1
    h, cache = M.lstm_fwd(pooled, wx, wh, bias, act)
    dx, dwx, dwh, dbias = M.lstm_bwd(cache, gh)
    dtab, dw, db = M.conv_pool_bwd(tok, table, w, b, pool, dx)
    for arr, grad in ((table, dtab), (w, dw), (b, db), (wx, dwx), (wh, dwh), (bias, dbias)):
        idx, num = _fd(loss, arr)
        ana = np.array([grad[i] for i in idx])
        assert np.allclose(ana, num, rtol=1e-5, atol=1e-7), (ana, num)


def test_model_gradients_against_finite_differences():
    from oracle import kgcn_oracle as K
    rng = np.random.default_rng(3)
    B, N, Fi, L, S = 4, 5, 3, 10, 4
    adjs = K.synth_mol_graphs(rng, B, N, 1)
    x = rng.standard_normal((B, N, Fi))
    tok = rng.integers(0, S, size=(B, L))
    lab = np.eye(2)[rng.integers(0, 2, size=B)]
    mask = np.array([1.0, 1.0, 1.0, 0.0])
    p = {"conv_w": [rng.standard_normal((Fi, 50)) * 0.3], "conv_b": [rng.standard_normal(50) * 0.1],
         "dense_w": rng.standard_normal((50, 50)) * 0.2, "dense_b": rng.standard_normal(50) * 0.1,
         "embeddings": rng.standard_normal((S, 4)), "conv_kernel": rng.standard_normal((4, 4, 50)) * 0.3,
         "conv_bias": rng.standard_normal(50) * 0.1, "kernel": rng.standard_normal((50, 128)) * 0.2,
         "recurrent_kernel": rng.standard_normal((32, 128)) * 0.2, "bias": rng.standard_normal(128) * 0.2,
         "hidden_w": rng.standard_normal((82, 52)) * 0.2, "hidden_b": rng.standard_normal(52) * 0.1,
         "out_w": rng.standard_normal((52, 2)) * 0.3, "out_b": rng.standard_normal(2) * 0.1}
    _, _, _, cache = M.model_fwd(p, x, adjs, tok, lab, mask)
    g = M.model_bwd(p, cache)
    for name in M.PARAM_NAMES:
        arr, grad = (p[name][0], g[name][0]) if isinstance(p[name], list) else (p[name], g[name])
        idx, num = _fd(lambda: M.model_fwd(p, x, adjs, tok, lab, mask)[1], arr, n=6)
        ana = np.array([grad[i] for i in idx])
        assert np.allclose(ana, num, rtol=1e-5, atol=1e-8), (name, ana, num)


# ---- the sequence loader against the reference feed -------------------------------------------------------------------
def test_sequence_loader_matches_the_reference_feed_bit_for_bit():
    import torch
    from kgcn_amd import data_util as D
    g = np.load(GOLDEN)
    tokens, S = D.sequence_table({"sequence": g["sequence"], "sequence_symbol_num": g["sequence_symbol_num"]}, "cpu")
    assert S == int(g["info_sequence_symbol_num"]) and tokens.shape[1] == int(g["info_sequence_max_length"])
    assert tokens.dtype == torch.int32
    B = int(g["feed_batch_size"])
    for idx, ref in zip(g["feed_batch_idx"], g["feed_sequences"]):
        out = np.zeros((B, tokens.shape[1]), np.int32)          # StaticBatch.add_table: zero rows for the dummy graphs
        real = idx[idx >= 0]
        out[:len(real)] = tokens.numpy()[real]
        assert out.dtype == ref.dtype and np.array_equal(out, ref)


def test_sequence_loader_refuses_bad_tokens_and_shapes_on_the_host():
    from kgcn_amd import _lib, data_util as D
    ok = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError):
        D.sequence_table({"sequence": ok, "sequence_symbol_num": 2}, "cpu")            # token 2 outside [0, 2)
    with pytest.raises(ValueError):
        D.sequence_table({"sequence": -ok, "sequence_symbol_num": 3}, "cpu")
    with pytest.raises(ValueError):
        D.sequence_table({"sequence": ok}, "cpu")
    with pytest.raises(_lib.KgcnHipError):
        D.sequence_table({"sequence": ok, "sequence_symbol_num": 1025}, "cpu")
    with pytest.raises(_lib.KgcnHipError):
        D.sequence_table({"sequence": np.zeros((1, 8193), np.int32), "sequence_symbol_num": 3}, "cpu")


# ---- ABI and limits without a GPU ---------------------------------------------------------------------------------------
def test_header_and_library_export_the_new_symbols():
    from kgcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "kgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr), name
    assert "#define KGCN_HIP_ABI_VERSION 2" in header


@pytest.mark.parametrize("args", [
    (2, 100, 25, 33, 4, 50, 4),      # E > 32
    (2, 100, 25, 4, 4, 65, 4),       # F > 64
    (2, 100, 25, 4, 9, 50, 4),       # k > 8
    (2, 100, 25, 4, 4, 50, 9),       # pool > 8
    (2, 100, 1025, 4, 4, 50, 4),     # S > 1024
    (2, 8193, 25, 4, 4, 50, 4),      # L > 8192
])
def test_convpool_limits_refused_without_a_gpu(args):
    from kgcn_amd import _lib
    lib = _lib.lib
    assert lib.kgcn_seq_convpool_workspace_bytes(*args) == -1
    assert lib.kgcn_seq_convpool_fwd_f32(None, args[0], args[1], None, args[2], args[3], None, None, args[4], args[5], args[6], None,
                                         None, None) != 0
    assert lib.kgcn_seq_convpool_workspace_bytes(2, 100, 25, 4, 4, 50, 4) > 0


def test_convpool_forwards_validate_under_their_own_name_without_a_gpu():
    """The three forwards share one launcher; each validates first, under its own name, and fails before any HIP call."""
    from kgcn_amd import _lib
    lib = _lib.lib
    L, S, E, k, F, p = 16, 4, 8, 4, 8, 4
    conv = (L, None, S, E, None, None, k, F, p, None, None, None)      # length .. stream, the operands NULL

    def calls(batch, rep):
        return (("kgcn_seq_convpool_fwd_f32", lambda: lib.kgcn_seq_convpool_fwd_f32(None, batch, *conv)),
                ("kgcn_seq_convpool_scaled_fwd_f32", lambda: lib.kgcn_seq_convpool_scaled_fwd_f32(None, batch, rep, None, *conv)),
                ("kgcn_seq_convpool_perturbed_fwd_f32",
                 lambda: lib.kgcn_seq_convpool_perturbed_fwd_f32(None, batch, rep, None, None, None, None, 0, *conv)))

    for name, call in calls(4, 2):
        assert call() != 0
        assert lib.kgcn_last_error().decode().startswith(name + ":"), name
    for name, call in calls(0, 2):
        assert call() == 0, name
    input_grad = ("kgcn_seq_convpool_input_grad_f32",
                  lambda: lib.kgcn_seq_convpool_input_grad_f32(None, 3, 2, L, None, S, E, None, k, F, p, None, None, None, 0, None, None))
    for name, call in calls(3, 2)[1:] + (input_grad,):                  # 3 rows are not whole groups of 2 copies
        assert call() != 0
        assert "whole groups" in lib.kgcn_last_error().decode(), name


@pytest.mark.parametrize("D,H", [(65, 32), (50, 65), (0, 32)])
def test_lstm_limits_refused_without_a_gpu(D, H):
    from kgcn_amd import _lib, layers, ops
    assert _lib.lib.kgcn_seq_lstm_fwd_f32(None, 2, 10, D, None, None, None, H, 0, None, H, None, None) != 0
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_limits_check(units=H, in_dim=D)
    with pytest.raises(_lib.KgcnHipError):
        layers.SequenceEncoder(25, 4, filters=D, units=H)
    assert _lib.lib.kgcn_seq_lstm_fwd_f32(None, 2, 10, 50, None, None, None, 32, 2, None, 32, None, None) != 0   # activation code


def test_sequence_encoder_keras_initialisers():
    import torch
    from kgcn_amd import layers
    torch.manual_seed(0)
    enc = layers.SequenceEncoder(25, 4)
    assert tuple(enc.embeddings.shape) == (25, 4) and float(enc.embeddings.detach().abs().max()) <= 0.05
    assert tuple(enc.conv_kernel.shape) == (4, 4, 50) and float(enc.conv_kernel.detach().abs().max()) <= np.sqrt(6.0 / (16 + 200))
    assert not torch.any(enc.conv_bias)
    r = enc.recurrent_kernel.detach().double().numpy()
    assert r.shape == (32, 128) and np.allclose(r @ r.T, np.eye(32), atol=1e-6)
    b = enc.bias.detach().numpy()
    assert np.all(b[32:64] == 1) and not np.any(b[:32]) and not np.any(b[64:])
