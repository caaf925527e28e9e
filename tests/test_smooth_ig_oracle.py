"""CPU tests of the smooth attribution methods: the noise contract of include/kgcn_hip.h as tests/smooth_ig_oracle.py restates it
(against vae_oracle's blocks, numpy's Philox and its own statistics), the row plan of kgcn_amd.visualization.smooth_rows, and the
oracle's smooth loop against the clean methods at noise_scale = 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_ig_oracle as IG  # noqa: E402
import smooth_ig_oracle as SO  # noqa: E402
import vae_oracle as VO  # noqa: E402


def test_noise_is_the_vae_block_stream_for_counter_j_0_0_0():
    seed, n = 1234, 64
    z = SO.noise(seed, 0, 0, 0, 1, 4 * n)[0]
    assert np.array_equal(z, VO.normals(VO.philox_blocks(seed, 0, n)))
    assert np.array_equal(z[:4 * 8], VO.normals(VO.numpy_philox_blocks(seed, 0, 8)))
    # a [R, W] array: row r starts at block r ceil(W / 4), column w is normal w & 3 of block w >> 2 of the row
    R, W = 3, 6
    a = SO.noise(seed, 0, 0, 0, R, W)
    flat = VO.normals(VO.philox_blocks(seed, 0, R * 2)).reshape(R, 8)
    assert np.array_equal(a, flat[:, :W])
    # k, g and s are counter words 1, 2, 3
    w = SO.noise_words(seed, 0x100, 7, 5, 2, 1)
    ctr = np.array([[2, 5, 7, 0x100]], np.uint64)
    assert np.array_equal(w, VO.philox4x64_10(ctr, np.array([[seed, 0]], np.uint64)))
    assert SO.noise(seed, 1, 0, 0, 1, 0).shape == (1, 0)


def test_noise_statistics_and_independence_of_the_streams():
    n = 2 ** 20
    z = SO.noise(1234, 0, 0, 0, 1024, 1024).reshape(-1)
    cap_mean, cap_var = 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n)
    mean, var = z.mean(), z.var()
    print("mean %.2e (cap %.2e)  var - 1 %.2e (cap %.2e)" % (mean, cap_mean, var - 1, cap_var))
    assert abs(mean) <= cap_mean and abs(var - 1.0) <= cap_var
    for name, (s, g, k) in (("k = 1", (0, 0, 1)), ("g = 1", (0, 1, 0)), ("s = 0x100", (0x100, 0, 0))):
        other = SO.noise(1234, s, g, k, 1024, 1024).reshape(-1)
        cross = float((z * other).mean())
        print("product-mean against %s: %.2e" % (name, cross))
        assert abs(other.mean()) <= cap_mean and abs(other.var() - 1.0) <= cap_var
        assert abs(cross) <= cap_mean              # the product of two independent N(0, 1) has variance 1


def test_smooth_rows_plan_and_ig_scales_still_refuses():
    from kgcn_amd import visualization as V
    assert V.SMOOTH_METHODS == ("smooth_grad", "smooth_ig")
    assert V.IG_METHODS == ("ig", "grad_prod", "grad")
    D = 4
    sc, sg, smp, wt, start, end = V.smooth_rows("smooth_ig", D, 0.1)
    assert sc == [0.0, 1.0, 0.25, 0.5, 0.75, 1.0] and sg == [0.0, 0.0, 0.1, 0.1, 0.1, 0.1]
    assert smp == [0, 0, 0, 1, 2, 3] and wt == [0.0, 0.0, 0.25, 0.25, 0.25, 0.25] and (start, end) == (0, 1)
    sc, sg, smp, wt, start, end = V.smooth_rows("smooth_grad", D, 0.3)
    assert sc == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0] and sg == [0.0, 0.0, 0.3, 0.3, 0.3, 0.3]
    assert smp == [0, 0, 0, 1, 2, 3] and wt == [0.0, 0.0, 0.25, 0.25, 0.25, 0.25] and (start, end) == (0, 1)
    for bad in (dict(method="ig"), dict(divide_number=0), dict(noise_scale=-0.1), dict(noise_scale=float("nan"))):
        kw = dict(method="smooth_grad", divide_number=3, noise_scale=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.smooth_rows(**kw)
    for m in V.SMOOTH_METHODS:
        with pytest.raises(ValueError):
            V.ig_scales(m, 10)


def _small_case(seed=0, N=4, F=3, L=9, E=3, S=5, C=2):
    rng = np.random.default_rng(seed)
    p = IG.random_params(rng, S, E, F, C=C)
    x = rng.standard_normal((N, F))
    A = (rng.random((C, N, N)) < 0.5).astype(float) * rng.uniform(0.5, 1.5, (C, N, N))
    return p, x, A, A != 0, p["embeddings"][rng.integers(0, S, L)]


@pytest.mark.parametrize("modal", ["all", "features", "adjs", "embedded_layer"])
def test_zero_noise_is_the_clean_method(modal):
    p, x, A, Sm, emb = _small_case()
    mask = np.array([0.0, 1.0])
    D = 6
    for smooth, clean in (("smooth_grad", "grad"), ("smooth_ig", "ig")):
        a = SO.smooth(p, x, A, Sm, emb, mask, D, modal, smooth, 0.0, 1234, 3)
        b = IG.integrated_gradients_literal(p, x, A, Sm, emb, mask, D, modal, clean)
        for key in b:
            assert np.abs(np.asarray(a[key]) - np.asarray(b[key])).max() <= 1e-12, (smooth, key)


def test_smooth_depends_on_seed_compound_and_noise_scale_only_through_the_noise():
    p, x, A, Sm, emb = _small_case(1)
    mask = np.array([1.0, 0.0])
    base = SO.smooth(p, x, A, Sm, emb, mask, 4, "all", "smooth_ig", 0.1, 1234, 0)
    again = SO.smooth(p, x, A, Sm, emb, mask, 4, "all", "smooth_ig", 0.1, 1234, 0)
    for key in base:
        assert np.array_equal(np.asarray(base[key]), np.asarray(again[key]))
    for kw in (dict(seed=1235), dict(g=1), dict(noise_scale=0.2)):
        args = dict(noise_scale=0.1, seed=1234, g=0)
        args.update(kw)
        other = SO.smooth(p, x, A, Sm, emb, mask, 4, "all", "smooth_ig", **args)
        assert not np.array_equal(base["features_IG"], other["features_IG"]), kw
        assert base["check_score"] == other["check_score"]            # the clean feeds
    # the values of EVERY channel are perturbed, the gradient is channel 0's
    xs, As, es = SO.perturbed_inputs(x, A, Sm, emb, ["adjs"], 1.0, 0.1, 1234, 0, 0)
    assert xs is x and es is emb
    assert np.all((As != A) == Sm) and np.all(As[~Sm] == 0)
