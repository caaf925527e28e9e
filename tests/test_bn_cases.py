"""CPU checks of tests/bn_cases.py, the cases tests/test_gpu_bn_cases.py runs on the device: every case reaches the kernel, template
instance or grid cap it names according to route() (the restatement of bn.hip's host rules, itself checked against the source's
constants here), the bounds made from the float32 restatement stay tight (4 * E32 <= 1e-3), relu pre-activations keep their
distance from 0, `clamped` and `all_empty` hold what they say, and the offset cases' views are really misaligned.  The E32 table
is printed (pytest -s / -rP); the docstring of tests/bn_cases.py carries the same figures."""
import os
import re

import numpy as np
import pytest

import bn_cases as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kgcn_amd", "csrc")


def test_route_restates_the_constants_of_the_source():
    bn = open(os.path.join(CSRC, "bn.hip")).read()
    common = open(os.path.join(CSRC, "kgcn_common.h")).read()
    assert int(re.search(r"constexpr int BN_BLOCKS = (\d+);", bn).group(1)) == B.BN_BLOCKS
    assert int(re.search(r"constexpr int kNumCU = (\d+);", common).group(1)) == B.NUM_CU
    assert int(re.search(r"if \(dv <= (\d+)\) \{", bn).group(1)) == B.COL_GROUPS
    assert "if (nb > (long)kNumCU * 8) nb = (long)kNumCU * 8;" in bn
    assert "if (b > (long)kNumCU * 16) b = (long)kNumCU * 16;" in bn
    assert "long nb = (rows + 8L * rpp - 1) / (8L * rpp);" in bn
    assert bn.count("tests/bn_cases.py") >= 4                            # whoever moves them sees where to follow


def test_route_on_the_shapes_the_suite_had():
    """the widths of test_graph_batch_normalization_both_phases (108 rows): all of them bn_apply_cols_kernel, no cap reached"""
    for d, kernel in ((50, "cols2"), (64, "cols4"), (3, "cols1"), (256, "cols4"), (300, "cols4")):
        r = B.route(d, 0, 108)
        assert r["apply"] == kernel and not (r["apply_capped"] or r["reduce_capped"] or r["dx_capped"])
    assert B.route(300, 0, 108)["cb"] == [256, 44]


@pytest.mark.parametrize("name", B.NAMES)
def test_case_reaches_the_route_it_names(name):
    r = B.expected_route(name)
    for key, want in B.SPECS[name].expect.items():
        assert r[key] == want, (name, key, r[key], want)
    T, N, D = B.shape3(name)
    assert T * N * D * 4 <= 17 << 20                                     # the largest case: 17 MB


def test_every_kernel_instance_and_cap_has_a_case():
    routes = {n: B.expected_route(n) for n in B.NAMES}
    assert {r["apply"] for r in routes.values()} == {"cols1", "cols2", "cols4", "vec", "scalar"}
    for kernel in ("cols4", "cols2", "vec"):                             # each capped apply kernel, and both other caps
        assert any(r["apply"] == kernel and r["apply_capped"] for r in routes.values()), kernel
    assert any(r["reduce_capped"] and r["reduce_rpp"][0] == 1 for r in routes.values())
    assert any(r["reduce_capped"] and r["reduce_rpp"][0] > 1 for r in routes.values())
    assert any(r["dx_capped"] for r in routes.values())
    assert any(len(r["cb"]) > 1 and r["cb"][-1] == 1 for r in routes.values())
    for act in ("sigmoid", "relu", "tanh"):
        assert {routes["act_%s_%d" % (act, d)]["apply"] for d in (3, 64, 1028)} == {"cols1", "cols4", "vec"}
    assert [n for n in B.NAMES if not B.SPECS[n].with_dx] == ["no_dx"]


def test_enabled_rows():
    for name in B.NAMES:
        f, spec = B.facts(name), B.SPECS[name]
        T, N, D = B.shape3(name)
        if spec.enabled == "ragged":
            assert f.enabled.shape == (T,) and f.enabled.min() == 0 and f.enabled.max() == N
            assert len(np.unique(f.enabled)) > 2 and 0 < f.valid_rows < T * N
    f = B.facts("clamped")
    assert (f.enabled > 12).sum() >= 2 and (f.enabled < 0).sum() >= 2 and f.enabled.dtype == np.int32
    assert np.array_equal(f.clipped, [12, 0, 12, 0, 12, 3, 0, 12, 1]) and f.valid_rows == 52
    f = B.facts("all_empty")
    assert f.valid_rows == 0 and not f.enabled.any()
    assert B.facts("squeezed").enabled is None and B.SPECS["squeezed"].shape == (12, 50)
    c = B.build("const_cols")
    assert np.all(c.x[:, :, [2, 7]] == np.float32(3.3)) and not c.x[:, :, 11].any()
    assert all(np.ptp(c.x[:, :, k]) > 1 for k in range(16) if k not in (2, 7, 11))
    for phase in (0, 1):                                                 # an empty batch: zeros, and statistics that only decay
        r = B.build("all_empty").ref[phase]
        assert not (r.y.any() or r.dx.any() or r.dgamma.any() or r.dbeta.any())
    r, c = B.build("all_empty").ref[1], B.build("all_empty")
    assert not (r.mean.any() or r.var.any())
    assert np.allclose(r.mm, 0.99 * c.mm.astype(np.float64), rtol=1e-15) and np.allclose(r.mv, 0.99 * c.mv.astype(np.float64), rtol=1e-15)


def test_offset_views_are_misaligned():
    assert B.OFFSET_CASES == ["off1_64", "off2_64", "off1_300"]
    for name, mod in (("off1_64", 4), ("off2_64", 8), ("off1_300", 4)):
        c = B.SPECS[name]
        T, N, D = c.shape
        n = T * N * D
        raw = np.zeros(c.off + n + 4, np.float32)
        base = (-raw.ctypes.data % 16) // 4                              # a 16-byte-aligned base inside the allocation
        buf = raw[base:base + c.off + n]
        assert buf.ctypes.data % 16 == 0
        view = buf[c.off:c.off + n].reshape(T, N, D)
        assert view.ctypes.data % 16 == mod == (4 * c.off) % 16 and view.flags.c_contiguous
        assert np.shares_memory(view, raw)


def test_relu_pre_activations_keep_their_distance():
    for name in B.NAMES:
        if B.SPECS[name].act == "relu":
            d = B.facts(name).relu_distance
            print("%s: min |pre-activation| over the valid rows of both phases %.3e" % (name, d))
            assert d >= B.RELU_MARGIN, (name, d)


def test_bounds_from_the_float32_restatement_stay_tight():
    """4 * E32 <= 1e-3 for every case, phase and quantity; prints the table"""
    worst = 0.0
    print("%-18s %5s %-7s %10s %10s" % ("case", "phase", "q", "E32", "bound"))
    for name in B.NAMES:
        e32 = B.facts(name).e32
        for phase in (0, 1):
            assert set(q for p, q in e32 if p == phase) == set(B.QUANTITIES[phase])
            for q in B.QUANTITIES[phase]:
                e = e32[phase, q]
                mark = " *" if 4 * e > B.WRITTEN[q] else ""
                print("%-18s %5d %-7s %10.2e %10.2e%s" % (name, phase, q, e, B.bound(name, phase, q), mark))
                assert np.isfinite(e) and 4 * e <= B.E32_CAP, (name, phase, q, e)
                assert B.bound(name, phase, q) == max(B.WRITTEN[q], 4 * e)
                worst = max(worst, e)
    print("largest E32 %.2e" % worst)


def test_docstring_table_is_what_is_computed():
    """the table in the docstring of bn_cases.py: each of its lines within 10 % of the figure computed here (the activations'
    exp and tanh may differ in the last place between numpy builds), and no comparison clearly above its written form missing"""
    table = {}
    for line in B.__doc__.splitlines():
        m = re.match(r"\s+(\w+)\s+([01])\s+(\w+)\s+(\d\.\d\de-\d\d)\s+(\d\.\d\de-\d\d)$", line)
        if m:
            table[m.group(1), int(m.group(2)), m.group(3)] = (float(m.group(4)), float(m.group(5)))
    assert len(table) >= 30
    for (name, phase, q), (e, bound) in table.items():
        have = B.facts(name).e32[phase, q]
        assert abs(have - e) <= 0.1 * e, (name, phase, q, have, e)
        assert abs(bound - 4 * e) <= 0.01 * bound and bound > B.WRITTEN[q]
    for name in B.NAMES:
        for (phase, q), e in B.facts(name).e32.items():
            if 4 * e > 1.25 * B.WRITTEN[q]:
                assert (name, phase, q) in table, (name, phase, q, e)


def test_bounds_see_a_single_pass_variance_and_a_dropped_row():
    """what the bounds are for, on the reference alone: var as E[x^2] - mean^2 in float32, and the statistics of the batch with one
    valid row left out, both miss the bound of `offset30`'s var by far"""
    c = B.build("offset30")
    rows = np.concatenate([c.x[t, :c.clipped[t]] for t in range(c.T)]).astype(np.float32)
    mean = rows.mean(0, dtype=np.float32)
    single = (rows * rows).mean(0, dtype=np.float32) - mean * mean
    ref = c.ref[1].var
    off = float(np.abs(single - ref).max() / np.abs(ref).max())
    print("offset30: float32 single-pass variance off by %.2e of max|var|, bound %.2e" % (off, B.bound("offset30", 1, "var")))
    assert off > 100 * B.bound("offset30", 1, "var")
    c = B.build("grid_256")
    rows = np.concatenate([c.g[t, :c.clipped[t]] for t in range(c.T)]).astype(np.float64)
    for phase in (0, 1):
        ref = c.ref[phase].dbeta
        assert np.allclose(rows.sum(0), ref, rtol=1e-12, atol=1e-12)
        dropped = float(np.abs(rows[-1]).max() / np.abs(ref).max())
        print("grid_256 phase %d: dbeta without one of %d rows off by %.2e of max|dbeta|, bound %.2e"
              % (phase, rows.shape[0], dropped, B.bound("grid_256", phase, "dbeta")))
        assert dropped > 100 * B.bound("grid_256", phase, "dbeta")
