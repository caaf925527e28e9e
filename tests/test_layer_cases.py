"""CPU checks of tests/layer_cases.py, the cases tests/test_gpu_gat_maxpool.py runs on the device: every case reaches the kernel
branch it names, tells the wrong variants it claims to rule out from the reference by a hundred tolerances, and keeps the margins
without which an fp32 kernel and the fp64 reference may legitimately disagree.  Every test prints its figures (pytest -s / -rP)."""
import numpy as np
import pytest

import layer_cases as L
from oracle import kgcn_oracle as K

ALL = sorted(L.CASES)
GAT = [c for c in ALL if L.CASES[c].get("gat", True)]
# the tolerances tests/test_gpu_gat_maxpool.py writes: (atol, rel)
TOL = {"gat_out": (2e-5, 0.0), "gat_dx": (2e-5, 1e-5), "gat_dwa": (2e-5, 2e-5), "mp": (1e-5, 0.0), "mpg_out": (0.0, 0.0),
       "mpg_dx": (2e-6, 0.0)}


def _tol(what, ref):
    atol, rel = TOL[what]
    return atol + rel * float(np.abs(ref).max())


def _dense(adj, d, x):
    """the densified products [M, K, D] of one channel and the mask of its stored positions"""
    idx, val, shape = adj
    prod = np.zeros((int(shape[0]), int(shape[1]), x.shape[1]), d)
    stored = np.zeros((int(shape[0]), int(shape[1])), bool)
    prod[idx[:, 0], idx[:, 1]] = np.asarray(val, d)[:, None] * x[idx[:, 1]]
    stored[idx[:, 0], idx[:, 1]] = True
    return prod, stored


# ---- the wrong variants -----------------------------------------------------------------------------------------------------
def maxpool_always_zero(x, adjs, g, dtype=np.float64):
    """(a) the implicit zero is a candidate of EVERY row, full ones included (has_zero = true; one more zero in the count)"""
    x, g = np.asarray(x, dtype), np.asarray(g, dtype)
    out = np.zeros((len(adjs), int(adjs[0][0][2][0]), x.shape[2]), dtype)
    dx = np.zeros_like(x)
    for b in range(len(adjs)):
        for adj in adjs[b]:
            idx, val = adj[0], np.asarray(adj[1], dtype)
            prod, stored = _dense(adj, dtype, x[b])
            wide = np.concatenate([prod, np.zeros_like(prod[:, :1])], axis=1)      # the extra candidate
            full = stored.all(axis=1)
            m = np.where(full[:, None], wide.max(axis=1), prod.max(axis=1))
            out[b] += m
            ind = prod == m[:, None, :]
            cnt = ind.sum(axis=1) + (full[:, None] & (m == 0))
            share = ind / cnt[:, None, :] * g[b][:, None, :]
            np.add.at(dx[b], idx[:, 1], val[:, None] * share[idx[:, 0], idx[:, 1]])
    return out, dx


def transposed(adjs):
    """(b) every channel's structure transposed (the values follow their entries)"""
    return [[(np.ascontiguousarray(idx[:, ::-1]), val, [shape[1], shape[0]]) for idx, val, shape in chans] for chans in adjs]


def gat_fwd_variant(x, adjs, weight_a, at_row=False, eps=1.0e-10):
    """(c) at_row: the denominator gathered at the ROW index; (d) eps: another constant.  The defaults are K.gat_fwd."""
    x = np.asarray(x, np.float64)
    B, N, D = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        for c, (idx, _val, _shape) in enumerate(adjs[b]):
            r, col = idx[:, 0], idx[:, 1]
            wa = np.asarray(weight_a[c], np.float64).reshape(-1)
            t = x[b][col] @ wa[:D] + x[b][r] @ wa[D:]
            e = np.exp(np.where(t > 0, t, 0.2 * t))
            denom = np.zeros(N)
            np.add.at(denom, r, e)
            al = e / (denom[r if at_row else col] + eps)
            rr = np.zeros((N, D))
            np.add.at(rr, r, al[:, None] * x[b][col])
            out[b] += 1.0 / (1.0 + np.exp(-rr))
    return out


# ---- reach ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL)
def test_reach(case):
    d = L.make_case(case)
    M, K_, D = d["M"], d["K"], d["D"]
    rs, cs = d["sizes"], d["col_sizes"]
    assert (rs == 0).any() and (rs == M).any()
    for data in (d["x"], d["x_pool"], d["xg"]):
        assert not data[np.arange(K_)[None, :] >= cs[:, None]].any()
    for data in (d["x"], d["x_pool"]):
        assert np.abs(data[np.arange(K_)[None, :] < cs[:, None]]).min() >= 0.05
    assert (d["x"] != d["x_pool"]).any(axis=2).sum() == (2 if d["faint"] else 0)
    neg_full = one_zero = sinks_ref = entries = oneway = longest = 0
    for t, chans in enumerate(d["adjs"]):
        for c, (idx, val, shape) in enumerate(chans):
            assert list(shape) == [M, K_] and len(idx) == len(val)
            assert len(idx) == 0 or (idx[:, 0].max() < rs[t] and idx[:, 1].max() < cs[t])     # padded rows: empty, unreferenced
            assert len(np.unique(idx[:, 0] * K_ + idx[:, 1])) == len(idx)                      # no duplicates
            assert len(val) == 0 or (0.2 <= np.abs(val).min() and np.abs(val).max() <= 0.8)
            per_row = np.bincount(idx[:, 0], minlength=M)
            longest = max(longest, int(per_row.max()))
            prod, stored = _dense((idx, val, shape), np.float64, d["x_pool"][t])
            if (t, c) in d["full"]:
                assert rs[t] == M
                fr, nb = d["full"][(t, c)]
                assert per_row[fr] == K_
                neg_full += int(prod[fr, :, 0].max() < 0)
                if nb is not None:
                    assert per_row[nb] == K_ - 1
                    one_zero += int(prod[nb, :, 0].max() == 0 and (prod[nb, stored[nb], 0] < 0).all())
            else:
                assert per_row.max(initial=0) < K_ or M == 1
            special = set(x for x in d["full"].get((t, c), ()) if x is not None) | {d["hubs"].get((t, c))}
            sink = d["sinks"].get((t, c), (None, None))[0]
            for r in range(int(rs[t])):
                if r == sink:
                    assert per_row[r] == 0
                    refs = set(idx[idx[:, 1] == r, 0])
                    assert 0 in refs and len(refs) >= 2
                    sinks_ref += 1
                elif r not in special and M > 1:
                    assert 1 <= per_row[r] <= 6                                               # sinks are the only valid empty rows
            if (t, c) in d["hubs"]:
                assert per_row[d["hubs"][(t, c)]] == L.HUB_LEN > 64
            entries += len(idx)
            oneway += int((~stored.T[idx[:, 0], idx[:, 1]]).sum()) if M == K_ else len(idx)
    print("%s: full rows with a negative feature-0 maximum %d, neighbours whose maximum is their one implicit zero %d, "
          "referenced sinks %d, entries %d (%.0f %% one-way), longest row %d, faint sink %s"
          % (case, neg_full, one_zero, sinks_ref, entries, 100.0 * oneway / entries, longest, d["faint"]))
    assert neg_full >= 1
    assert one_zero >= 1 or M < 3
    if d["gat"] and case != "one_node":
        assert sinks_ref >= 1 and (d["faint"] is not None) == ("d" in d["rules_out"]) == (D >= 2 * d["C"])
    if M > 1:                                                # one node: every entry is its own reverse
        assert 2 * oneway >= entries
    if d["C"] > 1:                                           # the channels differ in structure
        assert any(not np.array_equal(ch[0][0], ch[1][0]) for ch in d["adjs"])
    # the split of gat_bwd_dots_kernel, as kgcn_gat_bwd_f32 computes it: (nodes per workgroup, workgroups, nodes of the last one)
    nodes = d["T"] * M
    nblk = min(nodes, 512)
    npb = -(-nodes // nblk)
    nblk = -(-nodes // npb)
    want = {"narrow": (1, 259, 1), "wave_plus_one": (2, 260, 2), "exactly_512": (1, 512, 1), "short_last_block": (2, 257, 1)}
    assert case not in want or (npb, nblk, nodes - (nblk - 1) * npb) == want[case]
    assert {"one_node": D == 1, "narrow": D <= 4, "wave_plus_one": D == 65, "exactly_512": D % 2 == 0 and D % 4 != 0,
            "wide": D > 256 and 32 < M <= 64}.get(case, True)
    if case == "hub":
        assert longest == 70 and d["hubs"]
    if case == "rect":
        assert M != K_


# ---- discrimination ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL)
def test_wrong_variants_are_told_apart(case):
    """every variant a case claims to rule out differs from the reference by >= 100 x the tolerance of the GPU comparison"""
    d = L.make_case(case)
    ref, x, g, wa = d["ref"], d["x"], d["g"], d["weight_a"]
    ratio = {}
    # (a) judged on the generic data: forward and gradient
    out_a, dx_a = maxpool_always_zero(d["x_pool"], d["adjs"], g)
    ratio["a"] = min(np.abs(out_a - ref["mp_out"]).max() / _tol("mp", ref["mp_out"]),
                     np.abs(dx_a - ref["mp_dx"]).max() / _tol("mp", ref["mp_dx"]))
    if d["M"] == d["K"]:
        at = transposed(d["adjs"])
        ratio["b_maxpool"] = np.abs(K.graph_maxpool_bwd(d["x_pool"], at, g) - ref["mp_dx"]).max() / _tol("mp", ref["mp_dx"])
    if d["gat"]:
        with np.errstate(over="ignore"):
            assert np.array_equal(gat_fwd_variant(x, d["adjs"], wa), ref["gat_out"])
            dx_b, dwa_b = K.gat_bwd(x, at, wa, g)
            ratio["b_gat_dx"] = np.abs(dx_b - ref["gat_dx"]).max() / _tol("gat_dx", ref["gat_dx"])
            ratio["b_gat_dwa"] = min(np.abs(dwa_b[c] - ref["gat_dwa"][c]).max() / _tol("gat_dwa", ref["gat_dwa"][c])
                                     for c in range(d["C"]))
            ratio["c"] = np.abs(gat_fwd_variant(x, d["adjs"], wa, at_row=True) - ref["gat_out"]).max() / _tol("gat_out", 0)
            ratio["d"] = np.abs(gat_fwd_variant(x, d["adjs"], wa, eps=1.0e-6) - ref["gat_out"]).max() / _tol("gat_out", 0)
    print("%s: |variant - reference| / tolerance: %s" % (case, ", ".join("%s %.3g" % kv for kv in sorted(ratio.items()))))
    for v in d["rules_out"]:
        hit = [k for k in ratio if k[0] == v]
        assert hit and all(ratio[k] >= 100.0 for k in hit), (case, v, ratio)


# ---- margins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GAT)
def test_leaky_relu_margin(case):
    """|t_e| >= D 2^-23 sum_k (|x[c,k] wa[k]| + |x[r,k] wa[D+k]|), the worst-case rounding error of the fp32 dot: no entry's score
    can fall on the other side of the leaky-relu kink in fp32"""
    d = L.make_case(case)
    D = d["D"]
    worst = np.inf
    for t, chans in enumerate(d["adjs"]):
        x = d["x"][t].astype(np.float64)
        for c, (idx, _v, _s) in enumerate(chans):
            wa = d["weight_a"][c].astype(np.float64).reshape(-1)
            tt = x[idx[:, 1]] @ wa[:D] + x[idx[:, 0]] @ wa[D:]
            bound = D * 2.0 ** -23 * (np.abs(x[idx[:, 1]] * wa[:D]).sum(1) + np.abs(x[idx[:, 0]] * wa[D:]).sum(1))
            if len(tt):
                worst = min(worst, float((np.abs(tt) / bound).min()))
    print("%s: smallest |t_e| / rounding bound of the fp32 dot = %.3g" % (case, worst))
    assert worst >= 1.0


@pytest.mark.parametrize("case", ALL)
def test_maxpool_tie_gap(case):
    """generic data: the two largest candidates of every densified row and feature differ by >= 1e-6 max(1, |m|), 8 x the
    rounding of the two fp32 products -- unless they are equal by construction (two implicit zeros)"""
    d = L.make_case(case)
    worst = np.inf
    for t, chans in enumerate(d["adjs"]):
        for adj in chans:
            prod, stored = _dense(adj, np.float64, d["x_pool"][t])
            if prod.shape[1] < 2:
                continue
            top = np.sort(prod, axis=1)[:, -2:, :]
            gap = (top[:, 1] - top[:, 0]) / np.maximum(1.0, np.abs(top[:, 1]))
            by_construction = ((~stored).sum(1) >= 2)[:, None] & (top[:, 1] == 0) & (top[:, 0] == 0)
            assert not (stored[:, :, None] & (prod == 0)).any()          # a stored product is never 0 on this data
            if (~by_construction).any():
                worst = min(worst, float(gap[~by_construction].min()))
    print("%s: smallest relative gap between the two largest max-pooling candidates = %.3g" % (case, worst))
    assert worst >= 1e-6


@pytest.mark.parametrize("case", ALL)
def test_grid_data_has_real_ties(case):
    """the grid data is there for the tie rules: maxima shared by several stored entries, by a stored entry and the implicit zeros,
    and inside full rows (where a 0 product ties with NO implicit zero)"""
    d = L.make_case(case)
    among = with_zero = in_full = 0
    for t, chans in enumerate(d["adjs_grid"]):
        for c, adj in enumerate(chans):
            assert set(np.abs(adj[1]).tolist()) <= {0.5, 1.0}
            prod, stored = _dense(adj, np.float32, d["xg"][t])
            hits = (prod == prod.max(axis=1, keepdims=True)) & stored[:, :, None]
            n = hits.sum(axis=1)
            has_zero = ~stored.all(axis=1)
            among += int((n >= 2).sum())
            with_zero += int(((n >= 1) & has_zero[:, None] & (prod.max(axis=1) == 0)).sum())
            if (t, c) in d["full"]:
                in_full += int((n[d["full"][(t, c)][0]] >= 2).sum())
    print("%s: grid data: maxima shared by >= 2 stored entries %d, by stored entries and implicit zeros %d, inside full rows %d"
          % (case, among, with_zero, in_full))
    assert set(np.unique(d["xg"]).tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    if d["K"] > 1:
        assert among >= 1 and with_zero >= 1 and in_full >= 1


@pytest.mark.parametrize("case", GAT)
def test_saturation_cap_and_finite_reference(case):
    """at most 10 % of a case's valid per-channel sigmoids are exactly 0 or 1 in fp64: the comparison is not mostly about
    saturated values; the faint sink's outputs are NOT saturated"""
    d = L.make_case(case)
    with np.errstate(over="ignore"):
        _, cache = K.gat_fwd(d["x"], d["adjs"], d["weight_a"], want_cache=True)
    sat = tot = 0
    for (b, c, r, col, wa, t, e, denom, al, sg) in cache:
        v = sg[:int(d["sizes"][b])]
        sat += int(((v == 0) | (v == 1)).sum())
        tot += v.size
        if d["faint"] == (b, c):
            s0 = sg[0]
            assert ((s0 > 1e-3) & (s0 < 1 - 1e-3)).mean() >= 0.5, s0
            k = np.flatnonzero((r == 0) & (col == d["sinks"][(b, c)][0]))[0]
            assert denom[col[k]] == 0 and 0.5 < np.abs(al[k] * d["x"][b][col[k]]).max() < 3.0, al[k]
    print("%s: saturated share %.2f %% of %d" % (case, 100.0 * sat / tot, tot))
    assert sat <= 0.1 * tot
    for k in ("gat_out", "gat_dx", "mp_out", "mp_dx"):
        assert np.isfinite(d["ref"][k]).all(), k
    assert all(np.isfinite(w).all() for w in d["ref"]["gat_dwa"])
    pad = np.arange(d["M"])[None, :] >= d["sizes"][:, None]
    assert (d["ref"]["gat_out"][pad] == 0.5 * d["C"]).all() and not d["ref"]["mp_out"][pad].any()


@pytest.mark.parametrize("case", GAT)
def test_fp32_oracle_distance(case):
    """the numpy fp32 evaluation of the oracle stays inside the GPU tolerances (measured; printed per tensor)"""
    d = L.make_case(case)
    ref = d["ref"]
    with np.errstate(over="ignore"):
        out = K.gat_fwd(d["x"], d["adjs"], d["weight_a"], dtype=np.float32)
        dx, dwa = K.gat_bwd(d["x"], d["adjs"], d["weight_a"], d["g"], dtype=np.float32)
    e = {"gat_out": (np.abs(out - ref["gat_out"]).max(), _tol("gat_out", ref["gat_out"])),
         "gat_dx": (np.abs(dx - ref["gat_dx"]).max(), _tol("gat_dx", ref["gat_dx"])),
         "gat_dwa": max(((np.abs(dwa[c] - ref["gat_dwa"][c]).max(), _tol("gat_dwa", ref["gat_dwa"][c])) for c in range(d["C"])),
                        key=lambda p: p[0] / p[1])}
    print("%s: fp32 oracle - fp64 oracle (tolerance): %s; max |dx| %.3g, max |dweight_a| %.3g"
          % (case, ", ".join("%s %.2e (%.2e)" % (k, v[0], v[1]) for k, v in e.items()), np.abs(ref["gat_dx"]).max(),
             max(np.abs(w).max() for w in ref["gat_dwa"])))
    assert all(v[0] <= v[1] for v in e.values()), e


# ---- the reference against central differences, on the cases' own structure ---------------------------------------------------
@pytest.mark.parametrize("case", ["narrow", "one_node", "hub"])
def test_reference_gradients_by_central_differences(case):
    """as tests/test_oracle_math.py: h = 1e-6 in fp64, 1e-6 of max(1, |fd|).  Saturated rows have gradient 0 on both sides; hub
    adds the faint sink, whose gradient runs through alpha = E / (0 + 1e-10)."""
    d = L.make_case(case)
    rng = np.random.default_rng(1)
    x, x_pool = d["x"].astype(np.float64), d["x_pool"].astype(np.float64)
    wa = [w.astype(np.float64) for w in d["weight_a"]]
    g = d["g"].astype(np.float64)
    h = 1e-6
    valid = np.argwhere(np.arange(d["M"])[None, :] < d["sizes"][:, None])
    picks = [tuple(valid[i]) + (int(rng.integers(0, d["D"])),) for i in rng.choice(len(valid), 12, replace=False)]
    if d["faint"] is not None:
        picks += [(d["faint"][0], 0, 0), (d["faint"][0], d["sinks"][d["faint"]][0], d["D"] - 1)]
    worst = 0.0
    with np.errstate(over="ignore"):
        for i in picks:
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            fd = ((K.gat_fwd(xp, d["adjs"], wa) - K.gat_fwd(xm, d["adjs"], wa)) * g).sum() / (2 * h)
            err = abs(fd - d["ref"]["gat_dx"][i]) / max(1.0, abs(fd))
            worst = max(worst, err)
            assert err < 1e-6, (i, fd, d["ref"]["gat_dx"][i])
            xp, xm = x_pool.copy(), x_pool.copy()
            xp[i] += h
            xm[i] -= h
            fd = ((K.graph_maxpool_fwd(xp, d["adjs"]) - K.graph_maxpool_fwd(xm, d["adjs"])) * g).sum() / (2 * h)
            assert abs(fd - d["ref"]["mp_dx"][i]) < 1e-6 * max(1.0, abs(fd)), (i, fd, d["ref"]["mp_dx"][i])
        for c in range(d["C"]):
            for k in range(2 * d["D"]):
                wp, wm = [w.copy() for w in wa], [w.copy() for w in wa]
                wp[c][k, 0] += h
                wm[c][k, 0] -= h
                fd = ((K.gat_fwd(x, d["adjs"], wp) - K.gat_fwd(x, d["adjs"], wm)) * g).sum() / (2 * h)
                err = abs(fd - d["ref"]["gat_dwa"][c][k, 0]) / max(1.0, abs(fd))
                worst = max(worst, err)
                assert err < 1e-6, (c, k, fd, d["ref"]["gat_dwa"][c][k, 0])
    print("%s: largest |fd - gradient| / max(1, |fd|) = %.2e" % (case, worst))
