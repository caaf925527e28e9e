"""The hash graph kernels on the GPU (csrc/hashkern.hip and the copies route of csrc/graphkern.hip through kgcn_amd/ops.py and
kgcn_amd.graph_kernel.hash_graph_kernel) against the numpy oracle (tests/hash_kernel_oracle.py) on the fixture the reference
produced (tests/golden/g14_hash_kernel.npz).  Every comparison is exact: scaled attributes and Grams bit for bit, buckets and
runs as integers, colours as partitions."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import graph_kernel_oracle as O  # noqa: E402
import hash_kernel_oracle as H  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_hash_kernel.npz")
CASES = {"wl_u0": ("wl", None), "wl_u1": ("wl", "node"), "sp_u0": ("sp", None)}


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def small_set():
    return tuple(O.unpack_graphs(fixture(), "small_"))


@functools.lru_cache(maxsize=None)
def scaled():
    return H.scale_attributes(fixture()["small_attr"])[0]


@functools.lru_cache(maxsize=None)
def oracle_buckets(R):
    return H.buckets(scaled(), fixture()["r%d_V" % R], fixture()["r%d_b" % R], 1.0)


@functools.lru_cache(maxsize=None)
def oracle_gram(name, R):
    base, labels = CASES[name]
    return H.exact_gram(H.hash_features(list(small_set()), oracle_buckets(R), base, 3, labels))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, ref):
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.uint64), ref.view(np.uint64))


@functools.lru_cache(maxsize=None)
def graph_set():
    from kgcn_amd import graph_kernel as gk
    adjs, nn, lab = O.to_adjs(list(small_set()), 13)
    return gk.GraphSet(adjs, nn, lab)


def padded(per_node, R):
    """[R, Nv] over the existing nodes -> [R, T*M] int32 with -1 where no node exists."""
    gs = graph_set()
    full = np.full((R, gs.T * gs.M), -1, np.int32)
    full[:, gs.exists.reshape(-1)] = per_node
    return full


# ---- 1. attr_scale -----------------------------------------------------------------------------------------------------------
def scale_inputs():
    rng = np.random.default_rng(3)
    X = fixture()["small_attr"]
    const = rng.standard_normal((300, 5))
    const[:, 2] = -7.125                                              # a column of equal values
    return {"fixture 272 x 5 (256 + 16)": X, "one row": X[:1], "256 rows exactly": rng.standard_normal((256, 5)) * 3 + 1,
            "257 rows": rng.standard_normal((257, 3)), "d = 1": X[:, :1], "constant column": const,
            "large offset": rng.standard_normal((1000, 2)) * 1e-3 + 1e6}


@pytest.mark.parametrize("case", sorted(scale_inputs()))
def test_attr_scale_equals_the_oracle_bit_for_bit(case):
    from kgcn_amd import ops
    X = np.ascontiguousarray(scale_inputs()[case], np.float64)
    s, mean, std = (t.cpu().numpy() for t in ops.attr_scale(dev(X)))
    rs, rmean, rstd = H.scale_attributes(X)
    same_bits(mean, rmean)
    same_bits(std, rstd)
    same_bits(s, rs)
    if case == "constant column":
        assert std[2] == 0.0 and not s[:, 2].any()
    if case == "one row":
        assert not s.any() and not std.any()


# ---- 2. lsh_buckets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("R", [1, 3])
def test_lsh_buckets_equal_the_oracle_floor(R, d):
    from kgcn_amd import ops
    X = np.ascontiguousarray(scaled()[:, :d])
    V, b = fixture()["r3_V"][:R, :d].copy(), fixture()["r3_b"][:R].copy()
    got = ops.lsh_buckets(dev(X), dev(V), dev(b), 1.0).cpu().numpy()
    ref = H.buckets(X, V, b, 1.0)
    assert got.dtype == np.int64 and got.shape == (R, 272) and ref.min() < 0 < ref.max()      # negative buckets
    np.testing.assert_array_equal(got, ref)
    got = ops.lsh_buckets(dev(X), dev(V), dev(b), 0.37).cpu().numpy()                          # another width
    np.testing.assert_array_equal(got, H.buckets(X, V, b, 0.37))


def test_lsh_bucket_boundary_and_many_rows():
    """An offset that puts a value exactly on a boundary, and more rows than one workgroup stages with a row length that is no
    power of two."""
    from kgcn_amd import ops
    rng = np.random.default_rng(11)
    X = np.round(rng.standard_normal((1000, 7)) * 8) / 8              # eighths: the dot products below are exact
    V = np.round(rng.standard_normal((3, 7)) * 4) / 4
    z0 = H.projected(X, V[1], 0.0, 1.0)
    b = np.array([0.25, np.ceil(z0[17]) - z0[17] + 2.0, -0.5])       # row 17 of draw 1 lands on an integer
    ref = H.buckets(X, V, b, 1.0)
    assert H.projected(X, V[1], b[1], 1.0)[17] == ref[1, 17]
    np.testing.assert_array_equal(ops.lsh_buckets(dev(X), dev(V), dev(b), 1.0).cpu().numpy(), ref)
    X = rng.standard_normal((70, 129))                                # 129 + 1 doubles a staged row: 63 rows a workgroup
    V, b = rng.standard_normal((5, 129)), rng.random(5)
    np.testing.assert_array_equal(ops.lsh_buckets(dev(X), dev(V), dev(b), 0.5).cpu().numpy(), H.buckets(X, V, b, 0.5))


def test_lsh_refuses_what_no_bucket_holds():
    from kgcn_amd import _lib, ops
    X = scaled()[:, :2].copy()
    V, b = dev(np.array([[1.0, 1.0]])), dev(np.array([0.5]))
    ops.lsh_buckets(dev(X), V, b, 1.0)
    X[5, 1] = 1e300
    with pytest.raises(_lib.KgcnHipError, match="1 of 272 projected values.*not finite or reach 2\\^62"):
        ops.lsh_buckets(dev(X), V, b, 1.0)
    X[9, 0] = np.inf
    with pytest.raises(_lib.KgcnHipError, match="2 of 272"):
        ops.lsh_buckets(dev(X), V, b, 1.0)
    with pytest.raises(_lib.KgcnHipError, match="bin width"):
        ops.lsh_buckets(dev(scaled()), dev(fixture()["r3_V"]), dev(fixture()["r3_b"]), 0.0)
    with pytest.raises(_lib.KgcnHipError, match="float64"):
        ops.lsh_buckets(dev(scaled().astype(np.float32)), V, b, 1.0)
    with pytest.raises(_lib.KgcnHipError, match="v must be a contiguous"):
        ops.lsh_buckets(dev(scaled()), V, b, 1.0)


# ---- 3. rank_pairs -----------------------------------------------------------------------------------------------------------
def rank_pairs_reference(hi, lo, mark=None):
    exists = np.ones(len(hi), bool) if mark is None else mark >= 0
    out = np.full(len(hi), -1, np.int64)
    if exists.any():
        out[exists] = np.unique(np.stack([hi[exists], lo[exists]], 1), axis=0, return_inverse=True)[1].reshape(-1)
    return out, int(out.max()) + 1 if len(out) else 0


def rank_pair_inputs():
    rng = np.random.default_rng(2)
    big = 2 ** 62
    return {"n = 0": (np.zeros(0, np.int64), np.zeros(0, np.int64), None),
            "n = 1": (np.array([-5]), np.array([7]), None),
            "all equal": (np.full(300, 4), np.full(300, -9), None),
            "high word only": (np.arange(300) % 7 - 3, np.zeros(300, np.int64), None),
            "low word only": (np.zeros(300, np.int64), (np.arange(300) * 37) % 11 - 5, None),
            "negative and wide": (rng.choice([-big, -1, 0, 1, big, -2 ** 63], 500), rng.choice([-2 ** 63, -3, 0, 2 ** 63 - 1], 500), None),
            "rows that do not exist": (rng.integers(-3, 3, 700), rng.integers(-2, 2, 700),
                                       np.where(rng.random(700) < 0.3, -1, 0).astype(np.int32)),
            "no row exists": (np.arange(5), np.arange(5), np.full(5, -1, np.int32))}


@pytest.mark.parametrize("case", sorted(rank_pair_inputs()))
def test_rank_pairs(case):
    from kgcn_amd import ops
    hi, lo, mark = rank_pair_inputs()[case]
    hi, lo = np.asarray(hi, np.int64), np.asarray(lo, np.int64)
    import torch
    h = dev(hi) if len(hi) else torch.zeros(0, dtype=torch.int64, device="cuda")
    lw = dev(lo) if len(lo) else torch.zeros(0, dtype=torch.int64, device="cuda")
    ranks, info = ops.rank_pairs(h, lw, None if mark is None else dev(mark))
    ref, classes = rank_pairs_reference(hi, lo, mark)
    assert ranks.dtype == torch.int32
    np.testing.assert_array_equal(ranks.cpu().numpy(), ref)
    assert info.cpu().numpy().tolist() == [classes, 0]


def test_rank_pairs_counts_a_high_word_it_cannot_tell_from_a_missing_row():
    from kgcn_amd import ops
    hi = np.array([0, 2 ** 63 - 1, 3], np.int64)
    _, info = ops.rank_pairs(dev(hi), dev(np.zeros(3, np.int64)), dev(np.array([0, 0, -1], np.int32)))
    assert int(info[1].item()) == 1


# ---- 4. the copies kernels against R separate runs ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def copies_colourings(R=3, iterations=3):
    """-> (colours of the copies route after every refinement [iterations + 1] x [R, T*M], the same from R separate wl_colourings)."""
    import copy
    import torch
    from kgcn_amd import graph_kernel as gk, ops
    gs = graph_set()
    bucket = oracle_buckets(R)
    full = np.zeros((R, gs.T * gs.M), np.int64)
    full[:, gs.exists.reshape(-1)] = bucket
    mark = dev((gs.exists.reshape(-1).astype(np.int32) - 1)).repeat(R)
    draw = torch.arange(R, device="cuda", dtype=torch.int64)[:, None].expand(R, gs.T * gs.M).reshape(-1)
    col, info = ops.rank_pairs(draw, dev(full).reshape(-1), mark)
    together = [col]
    for _ in range(iterations):
        s, hi, lo = ops.wl_refine_copies(gs.csr, gs.num_nodes, col, R)
        col, info = ops.wl_rank_copies(gs.csr, gs.num_nodes, col, R, s, hi, lo)
        assert int(info[1].item()) == 0
        together.append(col)
    apart = []
    for r in range(R):
        one = copy.copy(gs)
        one.node_labels = full[r].reshape(gs.T, gs.M)
        apart.append([c.reshape(-1) for c in gk.wl_colourings(one, iterations=iterations)[0]])
    return [c.view(R, -1).cpu().numpy() for c in together], [[c.cpu().numpy() for c in a] for a in apart]


def test_copies_colours_are_the_per_draw_partitions_and_never_shared():
    together, apart = copies_colourings()
    gs = graph_set()
    exists = gs.exists.reshape(-1)
    assert (gs.T, gs.M) == (41, 13) and 0 in gs.num_nodes_host and 1 in gs.num_nodes_host
    ref = [O.wl_colours(H.with_labels(list(small_set()), O.dense_ranks(oracle_buckets(3)[r])), 3) for r in range(3)]
    for it, c in enumerate(together):
        assert c.dtype == np.int32 and c.shape == (3, 41 * 13)
        assert np.all(c[:, ~exists] == -1) and np.all(c[:, exists] >= 0)
        seen = [set(c[r, exists].tolist()) for r in range(3)]
        assert not (seen[0] & seen[1]) and not (seen[0] & seen[2]) and not (seen[1] & seen[2]), it
        assert sorted(seen[0] | seen[1] | seen[2]) == list(range(sum(len(s) for s in seen))), it      # dense over all draws
        for r in range(3):
            np.testing.assert_array_equal(O.first_occurrence(c[r, exists]), O.first_occurrence(apart[r][it][exists]),
                                          err_msg="iteration %d draw %d" % (it, r))
            np.testing.assert_array_equal(O.first_occurrence(c[r, exists]), O.first_occurrence(ref[r][it]))


def test_wl_runs_copies_equal_the_per_draw_runs_with_their_offsets():
    import torch
    from kgcn_amd import ops
    _, apart = copies_colourings()
    gs = graph_set()
    for it in (0, 3):
        colours = torch.stack([dev(apart[r][it]) for r in range(3)]).contiguous()
        col, graph, count = ops.wl_runs_copies(colours.reshape(-1), gs.num_nodes, gs.T, gs.M, 3, it << 32, 4 << 32)
        ref = [ops.wl_runs(colours[r].contiguous(), gs.num_nodes, gs.T, gs.M, (r * 4 + it) << 32) for r in range(3)]
        for i, got in enumerate((col, graph, count)):
            np.testing.assert_array_equal(got.cpu().numpy(), torch.cat([x[i] for x in ref]).cpu().numpy())
        assert int(count.sum().item()) == 3 * 272


def sp_copies_against_per_draw(graphs, labels, M):
    """labels [R, Nv] dense per draw -> asserts sp_features_copies == the per-draw sp_features with the draw in the column."""
    import torch
    from kgcn_amd import graph_kernel as gk, ops
    adjs, nn, lab = O.to_adjs(list(graphs), M)
    gs = gk.GraphSet(adjs, nn, lab)
    R = labels.shape[0]
    full = np.full((R, gs.T * gs.M), -1, np.int32)
    full[:, gs.exists.reshape(-1)] = labels
    lab_dev = dev(full)
    count = int(labels.max()) + 1
    col, graph, n = ops.sp_features_copies(gs.csr, gs.num_nodes, lab_dev.reshape(-1), R, count)
    ref = [ops.sp_features(gs.csr, gs.num_nodes, lab_dev[r].contiguous(), count) for r in range(R)]
    np.testing.assert_array_equal(col.cpu().numpy(), torch.cat([x[0] + (r << 32) for r, x in enumerate(ref)]).cpu().numpy())
    np.testing.assert_array_equal(graph.cpu().numpy(), torch.cat([x[1] for x in ref]).cpu().numpy())
    np.testing.assert_array_equal(n.cpu().numpy(), torch.cat([x[2] for x in ref]).cpu().numpy())
    return col.cpu().numpy(), n.cpu().numpy()


def test_sp_features_copies_on_the_fixture_set():
    labels = np.stack([O.dense_ranks(bk) for bk in oracle_buckets(3)])
    _, n = sp_copies_against_per_draw(small_set(), labels, 13)
    assert int(n.sum()) == 3 * sum(g[0] ** 2 for g in small_set())


def test_sp_features_copies_on_a_128_node_path():
    """The LDS maximum: 128 nodes, distances up to 127, 16,384 keys a copy sorted twice over the same distance bytes."""
    path = (128, O.both_ways([(i + 1, i) for i in range(127)]), np.zeros(128, np.int64))
    labels = np.stack([np.arange(128) % 3, (np.arange(128) // 5) % 4])
    col, n = sp_copies_against_per_draw([path], labels, 128)
    assert int(n.sum()) == 2 * 128 * 128 and int((col & 0xff).max()) == 127


def test_copies_refuse_more_rows_than_int32_positions_index():
    import torch
    from kgcn_amd import _lib, ops
    gs = graph_set()
    col = torch.zeros(gs.T * gs.M, dtype=torch.int32, device="cuda")
    too_many = (2 ** 31 - 1) // (gs.T * gs.M) + 1
    for call in (lambda: ops.wl_runs_copies(col, gs.num_nodes, gs.T, gs.M, too_many, 0, 1 << 32),
                 lambda: ops.wl_refine_copies(gs.csr, gs.num_nodes, col, too_many),
                 lambda: ops.sp_features_copies(gs.csr, gs.num_nodes, col, too_many, 1),
                 lambda: ops.wl_runs_copies(col, gs.num_nodes, gs.T, gs.M, 0, 0, 1 << 32)):
        with pytest.raises(_lib.KgcnHipError, match="at least one copy and fewer than 2\\^31 - 1 rows in all"):
            call()
    rc = _lib.lib.kgcn_wl_rank_copies_workspace_bytes(gs.T * gs.M, too_many)                        # the C entry refuses as well
    assert rc == -1 and b"copies" in _lib.lib.kgcn_last_error()


def test_forced_hash_collisions_raise_in_both_routes():
    from kgcn_amd import _lib, graph_kernel as gk
    z = fixture()
    attrs = H.to_attributes(list(small_set()), z["small_attr"], 13)
    for batched in (True, False):
        with pytest.raises(_lib.KgcnHipError, match="differ in their signatures"):
            gk.hash_graph_kernel(graph_set(), attributes=attrs, projections=z["r3_V"], offsets=z["r3_b"], batched=batched, hash_mask=0xF)


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("R", [3, 20])
def test_hash_graph_kernel_equals_the_oracle_bit_for_bit(R, name):
    from kgcn_amd import graph_kernel as gk
    z = fixture()
    base, labels = CASES[name]
    attrs = H.to_attributes(list(small_set()), z["small_attr"], 13)
    kw = dict(attributes=attrs, base=base, labels=labels, projections=z["r%d_V" % R], offsets=z["r%d_b" % R])
    raw = {b: gk.hash_graph_kernel(graph_set(), normalize=False, batched=b, **kw).cpu().numpy() for b in (True, False)}
    same_bits(raw[True], oracle_gram(name, R))
    same_bits(raw[False], raw[True])
    norm = {b: gk.hash_graph_kernel(graph_set(), batched=b, **kw).cpu().numpy() for b in (True, False)}
    same_bits(norm[True], O.normalize(oracle_gram(name, R)))
    same_bits(norm[False], norm[True])
    same_bits(gk.hash_graph_kernel(graph_set(), **kw).cpu().numpy(), norm[True])                   # two runs, the module default
    feats = gk.hash_graph_kernel(graph_set(), return_gram=False, **kw)
    assert feats.shape[0] == 41 and H.columns([feats]) == H.columns(H.hash_features(list(small_set()), oracle_buckets(R), base, 3, labels))
    bound = (int(z["r%d_%s_columns" % (R, name)]) + 8) * 2.0 ** -53                                # the reference's own rounding
    assert np.all(np.abs(raw[True] - z["r%d_%s" % (R, name)]) <= bound * np.abs(raw[True]))


@pytest.mark.parametrize("labels", ["node", "degree"])
def test_sp_joint_classes_and_float32_attributes(labels):
    from kgcn_amd import graph_kernel as gk
    z = fixture()
    graphs = list(small_set())
    X32 = z["small_attr"].astype(np.float32)
    attrs = H.to_attributes(graphs, X32.astype(np.float64), 13).astype(np.float32)
    kw = dict(attributes=attrs, base="sp", labels=labels, projections=z["r3_V"], offsets=z["r3_b"], normalize=False)
    ref = H.hash_gram(graphs, X32.astype(np.float64), z["r3_V"], z["r3_b"], 1.0, "sp", 3, labels)
    for batched in (True, False):
        same_bits(gk.hash_graph_kernel(graph_set(), batched=batched, **kw).cpu().numpy(), ref)
    unscaled = gk.hash_graph_kernel(graph_set(), scale_attributes=False, bin_width=2.0, **kw).cpu().numpy()
    same_bits(unscaled, H.hash_gram(graphs, X32.astype(np.float64), z["r3_V"], z["r3_b"], 2.0, "sp", 3, labels, scale=False))


def test_sp_refuses_more_classes_than_its_key_holds():
    from kgcn_amd import _lib, graph_kernel as gk
    rng = np.random.default_rng(4)
    graphs = [(128, np.zeros((0, 2), np.int64), np.zeros(128, np.int64)) for _ in range(40)]        # 5,120 nodes, no edges
    adjs, nn, lab = O.to_adjs(graphs, 128)
    attrs = rng.permutation(40 * 128).reshape(40, 128, 1).astype(np.float64)                        # every node its own bucket
    for batched in (True, False):
        with pytest.raises(_lib.KgcnHipError, match="5120 hash classes in one draw, up to 4096.*12 \\+ 12 \\+ 8 bits"):
            gk.hash_graph_kernel(adjs, nn, attrs, base="sp", scale_attributes=False, projections=np.ones((1, 1)),
                                 offsets=np.zeros(1), batched=batched)


def test_two_class_example_set_end_to_end():
    from kgcn_amd import graph_kernel as gk
    z13 = np.load(os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz"), allow_pickle=False)
    graphs = O.unpack_graphs(z13, "two_")
    adjs, nn, lab = O.to_adjs(graphs)
    attrs = H.to_attributes(graphs, fixture()["two_attr"])
    gs = gk.GraphSet(adjs, nn, lab)
    for base in ("wl", "sp"):
        K = gk.hash_graph_kernel(gs, attributes=attrs, base=base, hash_iterations=20, seed=0).cpu().numpy()
        again = gk.hash_graph_kernel(gs, attributes=attrs, base=base, hash_iterations=20, seed=0).cpu().numpy()
        same_bits(K, again)
        V, b = gk.lsh_draws(0, 20, 5)
        same_bits(K, H.hash_gram(graphs, fixture()["two_attr"], V, b, 1.0, base, 3, None, normalize=True))
        assert K.shape == (120, 120) and np.array_equal(K, K.T)
        result = gk.svm_cv(K, z13["two_y"], test_splits=3)
        print("hgk-%s on the two-class set: svm_cv mean accuracy %.3f (std %.3f)" % (base, result["mean"], result["std"]))
