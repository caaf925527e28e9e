"""CPU checks of the graph VAE (example_model/model_vae.py): the fp64 oracle against an op-by-op transcription with the dense
[B, C, N, N] logits and against central finite differences, the numpy Philox / Box-Muller restatement against np.random.Philox,
the Keras random_uniform initialiser, and the new C entry points in the header and the library."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vae_oracle as V  # noqa: E402
from oracle import kgcn_oracle as K  # noqa: E402

VAE_SYMBOLS = ("kgcn_philox4x64_raw", "kgcn_normal_f32", "kgcn_vae_sample_fwd_f32", "kgcn_vae_sample_bwd_f32",
               "kgcn_vae_recon_workspace_bytes", "kgcn_vae_recon_fwd_f32", "kgcn_vae_recon_bwd_f32")


def make_batch(rng, B, N, F, C, real=None, weights=False):
    """B graphs of N nodes (the last B - real are dummies: no adjacency entries, zero features), C channels."""
    real = B if real is None else real
    adjs = []
    for b in range(B):
        row = []
        for c in range(C):
            if b < real:
                idx, val, shp = K.synth_mol_graphs(rng, 1, N, 2)[0][0]
                val = np.asarray(val, np.float32)
                if weights:
                    val = (val * rng.uniform(0.2, 1.5, len(val))).astype(np.float32)
                row.append((idx, val, shp))
            else:
                row.append((np.zeros((0, 2), np.int32), np.zeros(0, np.float32), [N, N]))
        adjs.append(row)
    x = (rng.random((B, N, F)) < 0.4).astype(np.float64)
    x[real:] = 0
    mask = (np.arange(B) < real).astype(np.float64)
    return adjs, x, mask


# ---- noise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(0, 0), (1234, 1), (2 ** 63 + 5, 77), (2 ** 64 - 1, 2 ** 40)])
def test_philox_restatement_is_numpys_philox(seed, step):
    ours = V.philox_blocks(seed, step, 9)
    ref = V.numpy_philox_blocks(seed, step, 9)
    assert np.array_equal(ours, ref)


def test_box_muller_moments_and_range():
    z = V.noise(7, 3, (1 << 16,))
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1) < 0.02
    assert abs((z ** 3).mean()) < 0.05 and abs((z ** 4).mean() - 3) < 0.1
    assert np.all(np.isfinite(z)) and np.abs(z).max() < np.sqrt(-2 * np.log(2.0 ** -24)) + 1e-9
    assert not np.array_equal(V.noise(7, 3, (64,)), V.noise(7, 4, (64,)))        # a new step draws new noise


# ---- model pieces against the literal transcription / finite differences --------------------------------------------
def _fd(f, x, idx, h=1e-6):
    x0 = x[idx]
    x[idx] = x0 + h
    fp = f()
    x[idx] = x0 - h
    fm = f()
    x[idx] = x0
    return (fp - fm) / (2 * h)


def test_sample_gradient_finite_differences_and_clip_edges():
    rng = np.random.default_rng(0)
    B, N, D = 3, 4, 6
    m = rng.standard_normal((B, D)) * 3
    s = rng.standard_normal((B, D)) * 2
    m[0, 0], m[0, 1] = 100.0, 130.0                 # at the clip limit (gradient passes) and beyond (blocked)
    s[1, 0] = np.log(np.expm1(25.0))                # sqrt(softplus) = 5 exactly: gradient passes at equality
    s[1, 1] = 40.0                                  # beyond 5: blocked
    s[2, 0] = 1e-3                                  # softplus near 0
    eps = rng.standard_normal((B, N, D))
    gz = rng.standard_normal((B, N, D))
    gk = rng.standard_normal(B)

    def f():
        z, kl = V.sample_fwd(m, s, eps)
        return (gz * z).sum() + (gk * kl).sum()

    dm, ds = V.sample_bwd(m, s, eps, gz, gk)
    assert dm[0, 1] == 0 and ds[1, 1] == 0
    assert dm[0, 0] != 0 and ds[1, 0] != 0
    for idx in [(0, 2), (1, 3), (2, 5), (2, 0)]:
        assert abs(_fd(f, m, idx) - dm[idx]) < 1e-5 * max(1, abs(dm[idx]))
        assert abs(_fd(f, s, idx) - ds[idx]) < 1e-5 * max(1, abs(ds[idx]))


def test_recon_matches_dense_transcription_and_finite_differences():
    rng = np.random.default_rng(1)
    B, N, F, C, D = 5, 7, 4, 3, 8
    adjs, x, mask = make_batch(rng, B, N, F, C, real=3, weights=True)
    A = V.dense_labels(adjs, B, C, N)
    ys = [rng.random((B, N, D)) for _ in range(C)]
    ws = [rng.uniform(-1, 1, D) for _ in range(C)]
    xf = rng.standard_normal((B, N, F))
    kl = rng.standard_normal(B)
    res = V.recon_fwd(ys, ws, A, xf, x, mask, kl)
    # dense [B, C, N, N] form, op by op
    logits = np.transpose(np.stack([np.einsum("bik,bjk->bij", y * w, y) for y, w in zip(ys, ws)]), [1, 0, 2, 3])
    cost = mask * (V.sig_ce(xf, x).mean(axis=2).mean(axis=1) + V.sig_ce(logits, A).mean(axis=3).mean(axis=2).mean(axis=1))
    assert np.isclose(res["cost_sum"], cost.mean(), rtol=1e-12)
    assert np.isclose(res["cost_opt"], cost.mean() - 0.5 * kl.mean(), rtol=1e-12)
    ce = ((logits.max(axis=1) > 0) == (A.max(axis=1) > 0.5)).astype(float)
    assert np.isclose(res["correct_count"], (mask * ce.mean(axis=(1, 2))).sum(), rtol=1e-12)
    go, gs = 0.7, 0.4
    dys, dws, dxf, dkl = V.recon_bwd(ys, ws, A, xf, x, mask, go, gs)

    def f():
        r = V.recon_fwd(ys, ws, A, xf, x, mask, kl)
        return go * r["cost_opt"] + gs * r["cost_sum"]

    for c in range(C):
        for idx in [(0, 1, 2), (2, 6, 7), (4, 0, 0)]:
            assert abs(_fd(f, ys[c], idx) - dys[c][idx]) < 1e-8
        for k in (0, 5):
            assert abs(_fd(f, ws[c], (k,)) - dws[c][k]) < 1e-8
    for idx in [(0, 0, 0), (2, 3, 1), (4, 6, 3)]:
        assert abs(_fd(f, xf, idx) - dxf[idx]) < 1e-8
    assert abs(_fd(f, kl, (1,)) - dkl[1]) < 1e-8


@pytest.mark.parametrize("C,real", [(1, 4), (2, 3)])
def test_model_oracle_against_literal_transcription_and_finite_differences(C, real):
    rng = np.random.default_rng(2 + C)
    B, N, F = 4, 6, 3
    adjs, x, mask = make_batch(rng, B, N, F, C, real=real)
    A = V.dense_labels(adjs, B, C, N)
    p = V.init_params(rng, F, C)
    eps = rng.standard_normal((B, N, V.LATENT))
    res, cache = V.forward(p, x, adjs, A, mask, eps)
    lit = V.literal_cost(p, x, adjs, A, mask, eps)
    assert np.allclose([res["cost_opt"], res["cost_sum"], res["correct_count"]], lit, rtol=1e-12, atol=0)
    g = V.backward(p, cache, 1.0, 0.0)

    def f():
        return V.literal_cost(p, x, adjs, A, mask, eps)[0]

    def check(arr, garr, picks=2):
        flat_idx = rng.choice(arr.size, size=min(picks, arr.size), replace=False)
        for fi in flat_idx:
            idx = np.unravel_index(fi, arr.shape)
            num = _fd(f, arr, idx)
            assert abs(num - garr[idx]) < 2e-6 * max(1.0, abs(num)), (idx, num, garr[idx])

    for name in ("dense", "mean", "std", "node"):
        check(p[name][0], g[name][0])
        check(p[name][1], g[name][1])
    for name in ("conv1", "conv2"):
        for c in range(C):
            check(p[name][0][c], g[name][0][c])
            check(p[name][1][c], g[name][1][c].reshape(p[name][1][c].shape))
    for name in ("bn1", "bn2"):
        check(p[name]["gamma"], g[name]["gamma"])
        check(p[name]["beta"], g[name]["beta"])
    for q, gq in zip(p["links"], g["links"]):
        check(q["d1"][0], gq["d1"][0])
        check(q["d2"][1], gq["d2"][1])
        check(q["bn"]["gamma"], gq["bn"]["gamma"])
        check(q["w"], gq["w"])


# ---- interface -------------------------------------------------------------------------------------------------------
def test_random_uniform_initializer_bounds():
    import torch
    from kgcn_amd import layers
    torch.manual_seed(0)
    t = layers._init_tensor((64, 100), "random_uniform", "cpu")
    assert t.abs().max() <= 0.05 and t.abs().max() > 0.049 and abs(float(t.mean())) < 0.002
    v = layers._init_vector(4096, "random_uniform", "cpu")
    assert v.abs().max() <= 0.05 and v.abs().max() > 0.049


def test_keras_dense_kernel_initializer():
    from kgcn_amd import models
    assert models.KerasDense(8).kernel_initializer == "glorot_uniform"
    assert models.KerasDense(8, kernel_initializer="random_uniform").kernel_initializer == "random_uniform"


def test_header_and_library_carry_the_vae_entry_points():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_abi import declared_functions
    from kgcn_amd import _lib
    names = declared_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in VAE_SYMBOLS:
        assert name in names, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "kgcn_hip.h")).read()
    for lim, val in (("KGCN_VAE_MAX_NODES", 128), ("KGCN_VAE_MAX_CHANNELS", 8), ("KGCN_VAE_MAX_DIM", 64)):
        assert "#define %s %d" % (lim, val) in hdr


def test_recon_limits_are_refused_without_a_gpu():
    """Shape validation runs before any launch: out-of-range shapes fail with a message (no silent fallback)."""
    from kgcn_amd import _lib
    lib = _lib.lib
    csr = (_lib.CsrBatch * 9)()
    for c in range(9):
        csr[c].num_graphs, csr[c].rows, csr[c].cols = 2, 10, 10
        csr[c].rowptr = 1                                       # never dereferenced: the call fails on the shape first
    ys = (ctypes.c_void_p * 9)(*([8] * 9))
    for C, d, n in ((9, 8, 10), (1, 65, 10), (1, 8, 129)):
        for c in range(C):
            csr[c].rows = csr[c].cols = n
        rc = lib.kgcn_vae_recon_fwd_f32(csr, C, ys, ys, d, 8, 8, 3, None, None, 8, 8, None)
        assert rc != 0
        msg = lib.kgcn_last_error().decode()
        assert "supported" in msg, msg
    assert lib.kgcn_vae_sample_fwd_f32(8, 8, 2, 3, 65, 130, None, 0, None, 8, None, None) != 0
