"""The numpy oracle of the hash graph kernels (tests/hash_kernel_oracle.py) against what the reference's own pieces produced
(tests/golden/g14_hash_kernel.npz, made by tests/golden/make_golden_hash_kernel.py), and the host parts of
kgcn_amd.graph_kernel.hash_graph_kernel: the seeded draws and the argument refusals.  No GPU.

Bounds
  buckets  equal as partitions: the fixture's projected values keep >= 1e-9 from every bucket boundary (re-checked here), the
           summation-order error of a projected value z is about 1e-15 |z|.
  scaling  within Nv 2^-52 of the column's largest magnitude: the only difference to sklearn is the summation order of Nv terms.
  Gram     within (C + 8) 2^-53 relative, C the fixture's column count: the reference rounds 1 / R, its square root and the two
           scaled counts, the product, and C - 1 additions, against one rounding in exact / R.  The normalised Gram: doubled."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import graph_kernel_oracle as O  # noqa: E402
import hash_kernel_oracle as H  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_hash_kernel.npz")
CASES = {"wl_u0": ("wl", None), "wl_u1": ("wl", "node"), "sp_u0": ("sp", None)}


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def small(z):
    return O.unpack_graphs(z, "small_")


@pytest.fixture(scope="module")
def scaled(z):
    return H.scale_attributes(z["small_attr"])[0]


def test_fixture_holds_the_edge_cases(z, small):
    sizes = [g[0] for g in small]
    assert len(small) == 41 and sizes[0] > 0 and 0 in sizes and 1 in sizes and max(sizes) == 13
    assert z["small_attr"].shape == (272, 5) and sum(sizes) == 272              # two chunks of the column sums: 256 + 16
    assert z["r3_V"].shape == (3, 5) and z["r20_V"].shape == (20, 5) and z["two_attr"].shape[1] == 5


def test_scaled_attributes_equal_sklearn_within_the_summation_order(z, scaled):
    ref = z["small_scaled"]
    bound = 272 * 2.0 ** -52 * np.abs(ref).max(axis=0)
    err = np.abs(scaled - ref).max(axis=0)
    print("scaling: max |oracle - sklearn| per column", err, "bound", bound)
    assert np.all(err <= bound)


def test_constant_column_scales_to_zero():
    X = np.stack([np.arange(7.0), np.full(7, 3.25)], 1)
    s, mean, std = H.scale_attributes(X)
    assert std[1] == 0.0 and not s[:, 1].any() and mean[1] == 3.25
    np.testing.assert_allclose(s[:, 0].std(), 1.0, rtol=1e-15)


@pytest.mark.parametrize("R", [3, 20])
def test_buckets_equal_the_recorded_hashes_as_partitions(z, scaled, R):
    V, b, hashes = z["r%d_V" % R], z["r%d_b" % R], z["r%d_hashes" % R]
    dist = H.boundary_distance(scaled, V, b, 1.0)
    print("R", R, "smallest distance to a bucket boundary", dist, "recorded", float(z["r%d_min_dist" % R]))
    assert dist >= 1e-9 and float(z["r%d_min_dist" % R]) >= 1e-9
    mine = H.buckets(scaled, V, b, 1.0)
    assert mine.shape == hashes.shape == (R, 272) and mine.min() < 0 < mine.max()
    for r in range(R):
        np.testing.assert_array_equal(O.first_occurrence(mine[r]), O.first_occurrence(hashes[r]), err_msg="draw %d" % r)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("R", [3, 20])
def test_oracle_gram_equals_the_reference_within_its_rounding(z, small, scaled, R, name):
    base, labels = CASES[name]
    feats = H.hash_features(small, H.buckets(scaled, z["r%d_V" % R], z["r%d_b" % R], 1.0), base, 3, labels)
    C = int(z["r%d_%s_columns" % (R, name)])
    assert H.columns(feats) == C
    exact = H.exact_gram(feats)
    ref = z["r%d_%s" % (R, name)]
    bound = (C + 8) * 2.0 ** -53
    err = np.abs(ref - exact)
    print(name, "R", R, "columns", C, "max relative difference %.3g, bound %.3g" % (float((err / np.where(exact == 0, 1, exact)).max()), bound))
    assert np.all(err <= bound * np.abs(exact))
    norm, ref_norm = O.normalize(exact), z["r%d_%s_norm" % (R, name)]
    assert np.all(np.abs(ref_norm - norm) <= 2 * bound * np.abs(norm))
    empty = [g[0] for g in small].index(0)
    assert not exact[empty].any() and not norm[:, empty].any()


def test_joint_classes_are_finer_than_either_colouring(z, small, scaled):
    bucket = H.buckets(scaled, z["r3_V"], z["r3_b"], 1.0)[0]
    plain, joint = H.wl_hash_features(small, bucket, 3, None), H.wl_hash_features(small, bucket, 3, "node")
    assert joint.shape[1] > plain.shape[1] and joint.shape[1] > O.wl_features(small, 3, "node").shape[1]
    assert H.sp_hash_features(small, bucket, "node").shape[1] > H.sp_hash_features(small, bucket, None).shape[1]
    np.testing.assert_array_equal(np.asarray(joint.sum(axis=1)).reshape(-1), 4 * np.array([g[0] for g in small]))


def test_lsh_draws_are_reproducible_by_seed():
    from kgcn_amd.graph_kernel import lsh_draws
    V, b = lsh_draws(7, 20, 5, sigma=1.5, bin_width=0.5)
    V2, b2 = lsh_draws(7, 20, 5, sigma=1.5, bin_width=0.5)
    assert V.shape == (20, 5) and b.shape == (20,) and V.dtype == b.dtype == np.float64
    np.testing.assert_array_equal(V, V2)
    np.testing.assert_array_equal(b, b2)
    assert np.all((b >= 0) & (b < 0.75)) and not np.array_equal(V, lsh_draws(8, 20, 5, 1.5, 0.5)[0])
    np.testing.assert_array_equal(lsh_draws(7, 3, 5, 1.5, 0.5)[0], V[:3])            # draw after draw: a prefix


def test_argument_refusals_that_need_no_gpu():
    from kgcn_amd import graph_kernel as gk
    with pytest.raises(ValueError, match='base must be "wl" or "sp"'):
        gk.hash_graph_kernel([], [], np.zeros((0, 1, 1)), base="rw")
    with pytest.raises(ValueError, match="labels must be None"):
        gk.hash_graph_kernel([], [], np.zeros((0, 1, 1)), labels="colour")
    with pytest.raises(ValueError, match="needs attributes"):
        gk.hash_graph_kernel([], [])
    gs = types.SimpleNamespace(T=2, num_nodes_host=np.array([2, 3]))
    good = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
    rows = gk._attribute_rows(good, gs)
    assert rows.dtype == np.float64 and rows.tolist() == [[0, 1], [2, 3], [6, 7], [8, 9], [10, 11]]
    bad = good.copy()
    bad[0, 2, 0] = np.nan                                                            # a row that does not exist: not read
    gk._attribute_rows(bad, gs)
    bad[1, 1, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or Inf at 1 of 5"):
        gk._attribute_rows(bad, gs)
    with pytest.raises(ValueError, match="float32 or float64"):
        gk._attribute_rows(good.astype(np.int64), gs)
    with pytest.raises(ValueError, match="at least 3 nodes"):
        gk._attribute_rows(good[:, :2], gs)
    assert gk.dataset_attributes({"feature": good}) is not None and gk.dataset_attributes({"label": [0]}) is None
