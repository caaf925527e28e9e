"""fp64 numpy restatement of example_model/model_vae.py (forward and backward) and of the noise the HIP kernels draw.

Built from the layer oracles of oracle/ (graphconv_*, graphdense_*, graph_bn_*, gather_*, gram_*), which it only calls.
Two forms of the cost:
  forward() / backward()  the factorisation the kernels use (per channel L = gram_fwd(Y_c, w_c), its gradient through gram_bwd);
  literal_cost()          an op-by-op transcription of the TF graph with the dense [B, C, N, N] logits (tf.tile, tf.stack,
                          tf.transpose, the reduce_means in the file's order), the independent check of forward() / backward().
Noise: philox4x64_10() restates Random123's Philox4x64-10 (np.random.Philox is the same generator), normals() Box-Muller in
fp64 from the same 24-bit uniforms as the kernels (include/kgcn_hip.h)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import kgcn_oracle as K  # noqa: E402

LATENT = 64            # encoder_output_dim (model_vae.py:154) = internal_dim (:64, :117)
KL_EPS = 1.0e-10       # :177

_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
_W = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B))
_LO32 = np.uint64(0xFFFFFFFF)


def _mulhilo(a, b):
    """(hi, lo) 64-bit halves of the 128-bit products of uint64 arrays a * b."""
    with np.errstate(over="ignore"):
        a_lo, a_hi, b_lo, b_hi = a & _LO32, a >> np.uint64(32), b & _LO32, b >> np.uint64(32)
        ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
        mid = (ll >> np.uint64(32)) + (lh & _LO32) + (hl & _LO32)
        hi = hh + (lh >> np.uint64(32)) + (hl >> np.uint64(32)) + (mid >> np.uint64(32))
        return hi, a * b


def philox4x64_10(ctr, key):
    """ctr: uint64 [..., 4], key: uint64 [..., 2] -> uint64 [..., 4] (Random123 philox4x64, 10 rounds)."""
    x = [np.array(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.array(key[..., i], dtype=np.uint64) for i in range(2)]
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(np.broadcast_to(_M[0], x[0].shape), x[0])
            hi1, lo1 = _mulhilo(np.broadcast_to(_M[1], x[2].shape), x[2])
            x = [hi1 ^ x[1] ^ k[0], lo1, hi0 ^ x[3] ^ k[1], lo0]
            k = [k[0] + _W[0], k[1] + _W[1]]
    return np.stack(x, axis=-1)


def philox_blocks(seed, step, num_blocks):
    """Words of blocks 0 .. num_blocks-1 for (seed, step): counter (j, step, 0, 0), key (seed, 0) -> uint64 [num_blocks, 4]."""
    j = np.arange(num_blocks, dtype=np.uint64)
    ctr = np.zeros((num_blocks, 4), np.uint64)
    ctr[:, 0] = j
    ctr[:, 1] = np.uint64(step % 2 ** 64)
    key = np.zeros((num_blocks, 2), np.uint64)
    key[:, 0] = np.uint64(seed % 2 ** 64)
    return philox4x64_10(ctr, key)


def numpy_philox_blocks(seed, step, num_blocks):
    """The same words drawn from np.random.Philox: numpy increments the 256-bit counter BEFORE each block, so block j of
    counter (j, step, 0, 0) is the first output of a generator started at that counter minus one."""
    out = np.empty((num_blocks, 4), np.uint64)
    for j in range(num_blocks):
        c = (int(step) % 2 ** 64) * 2 ** 64 + j - 1
        c %= 2 ** 256
        ctr = np.array([(c >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)
        bg = np.random.Philox(counter=ctr, key=np.array([seed % 2 ** 64, 0], dtype=np.uint64))
        out[j] = bg.random_raw(4)
    return out


def normals(words):
    """uint64 [nb, 4] -> fp64 [4 nb] Box-Muller values, from the 24-bit uniforms the kernels use."""
    w = np.asarray(words, np.uint64)
    u1 = ((w[:, 0::2] >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1::2] >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty((w.shape[0], 4))
    out[:, 0::2] = r * np.cos(2 * np.pi * u2)
    out[:, 1::2] = r * np.sin(2 * np.pi * u2)
    return out.reshape(-1)


def noise(seed, step, shape):
    n = int(np.prod(shape))
    return normals(philox_blocks(seed, step, (n + 3) // 4))[:n].reshape(shape)


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def softplus(s):
    return np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))


def sig_ce(logits, labels):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log(1 + exp(-|x|))."""
    return np.maximum(logits, 0) - logits * labels + np.log1p(np.exp(-np.abs(logits)))


# ---- reparameterisation (model_vae.py:89-96, 169-181) -------------------------------------------------------------
def sample_fwd(m_pre, s_pre, eps):
    """-> z [B, N, D], kl [B] = N sum_k (1 + 2 log(std + 1e-10) - mean^2 - std)."""
    m_pre, s_pre, eps = (np.asarray(t, np.float64) for t in (m_pre, s_pre, eps))
    N = eps.shape[1]
    mean = np.clip(m_pre, -100, 100)
    std = np.clip(np.sqrt(softplus(s_pre)), -5, 5)
    z = mean[:, None, :] + std[:, None, :] * eps
    kl = N * (1 + 2 * np.log(std + KL_EPS) - mean ** 2 - std).sum(axis=1)
    return z, kl


def clip_grad(x, lo, hi):
    """tf.clip_by_value's gradient (_ClipByValueGrad): passes where lo <= x <= hi, equality included."""
    return ((x >= lo) & (x <= hi)).astype(np.float64)


def sample_bwd(m_pre, s_pre, eps, dz, dkl):
    m_pre, s_pre, eps, dz = (np.asarray(t, np.float64) for t in (m_pre, s_pre, eps, dz))
    N = eps.shape[1]
    dkl = np.zeros(m_pre.shape[0]) if dkl is None else np.asarray(dkl, np.float64)
    mean = np.clip(m_pre, -100, 100)
    sq = np.sqrt(softplus(s_pre))
    std = np.clip(sq, -5, 5)
    gmean = dz.sum(axis=1) + dkl[:, None] * (-2 * N * mean)
    gstd = (dz * eps).sum(axis=1) + dkl[:, None] * N * (2 / (std + KL_EPS) - 1)
    dm = gmean * clip_grad(m_pre, -100, 100)
    ds = gstd * clip_grad(sq, -5, 5) * 0.5 / sq * sigmoid(s_pre)
    return dm, ds


# ---- reconstruction cost (model_vae.py:203-253) --------------------------------------------------------------------
def dense_labels(adjs, B, C, N):
    """adjs[b][c] COO triples (indices, values, shape) -> dense [B, C, N, N]; a repeated (i, j): the last entry."""
    A = np.zeros((B, C, N, N))
    for b in range(min(B, len(adjs))):
        for c in range(C):
            idx, val = np.asarray(adjs[b][c][0]).reshape(-1, 2), np.asarray(adjs[b][c][1], np.float64).reshape(-1)
            for (i, j), v in zip(idx, val):
                A[b, c, int(i), int(j)] = v
    return A


def recon_fwd(ys, ws, A, xf, tf, mask=None, kl=None):
    """-> dict: feat [B], link [B], correct [B] (unmasked per graph), cost_opt, cost_sum, correct_count."""
    B, C, N, _ = A.shape
    mask = np.ones(B) if mask is None else np.asarray(mask, np.float64)
    L = [K.gram_fwd(ys[c], ws[c]) for c in range(C)]
    link = sum(sig_ce(L[c], A[:, c]).sum(axis=(1, 2)) for c in range(C)) / (C * N * N)
    xf, tf = np.asarray(xf, np.float64), np.asarray(tf, np.float64)
    feat = sig_ce(xf, tf).mean(axis=(1, 2))
    lpos = np.any(np.stack([l > 0 for l in L]), axis=0)
    apos = np.any(A > 0.5, axis=1)
    correct = (lpos == apos).mean(axis=(1, 2))
    cost = mask * (feat + link)
    cost_sum = cost.mean()
    klterm = 0.0 if kl is None else -0.5 * np.asarray(kl, np.float64).mean()
    return dict(feat=feat, link=link, correct=correct, L=L, cost_sum=cost_sum, cost_opt=cost_sum + klterm,
                correct_count=(mask * correct).sum())


def recon_bwd(ys, ws, A, xf, tf, mask=None, g_opt=1.0, g_sum=0.0):
    """-> dys, dws, dxf, dkl for the incoming gradients g_opt (cost_opt) and g_sum (cost_sum)."""
    B, C, N, _ = A.shape
    mask = np.ones(B) if mask is None else np.asarray(mask, np.float64)
    gb = mask * (g_opt + g_sum) / B
    dys, dws = [], []
    for c in range(C):
        L = K.gram_fwd(ys[c], ws[c])
        G = (sigmoid(L) - A[:, c]) * (gb / (C * N * N))[:, None, None]
        dy, dw = K.gram_bwd(ys[c], ws[c], G)
        dys.append(dy)
        dws.append(dw)
    xf, tf = np.asarray(xf, np.float64), np.asarray(tf, np.float64)
    F = xf.shape[2]
    dxf = (sigmoid(xf) - tf) * (gb / (N * F))[:, None, None]
    dkl = np.full(B, -0.5 * g_opt / B)
    return dys, dws, dxf, dkl


# ---- the whole model ----------------------------------------------------------------------------------------------
def init_params(rng, F, C, scale=1.0):
    """Random parameters of the model's shapes (names follow models.GraphVAE's attributes)."""
    def gl(i, o):
        return K.glorot_uniform(rng, i, o).astype(np.float64) * scale

    def bnp(d):
        return dict(gamma=1 + 0.1 * rng.standard_normal(d), beta=0.1 * rng.standard_normal(d), mean=0.1 * rng.standard_normal(d),
                    var=1 + 0.2 * rng.random(d))

    H = LATENT
    p = dict(conv1=([gl(F, H) for _ in range(C)], [0.1 * rng.standard_normal(H) for _ in range(C)]), bn1=bnp(H),
             conv2=([gl(H, H) for _ in range(C)], [0.1 * rng.standard_normal(H) for _ in range(C)]), bn2=bnp(H), dense=(gl(H, H), 0.1 * rng.standard_normal(H)), mean=(rng.uniform(-0.05, 0.05, (H, H)), 0.1 * rng.standard_normal(H)),
             std=(gl(H, H), 0.1 * rng.standard_normal(H)), node=(rng.uniform(-0.05, 0.05, (H, F)), 0.1 * rng.standard_normal(F)),
             links=[dict(d1=(gl(H, H), 0.1 * rng.standard_normal(H)), bn=bnp(H), d2=(gl(H, H), 0.1 * rng.standard_normal(H)),
                         w=rng.uniform(-0.3, 0.3, H)) for _ in range(C)])
    return p


def _bn(x, q, en):
    return K.graph_bn_fwd(x, q["gamma"], q["beta"], q["mean"], q["var"], en)[0]


def forward(p, x, adjs, A, mask, eps, enabled=None):
    """-> (result dict of recon_fwd + kl / mean / std pre-activations, cache for backward)."""
    x = np.asarray(x, np.float64)
    c = dict(x=x)
    c["a1"] = K.graphconv_fwd(x, adjs, *p["conv1"])
    c["h1"] = np.tanh(_bn(c["a1"], p["bn1"], enabled))
    c["a2"] = K.graphconv_fwd(c["h1"], adjs, *p["conv2"])
    c["h2"] = np.tanh(_bn(c["a2"], p["bn2"], enabled))
    c["h3"] = sigmoid(K.graphdense_fwd(c["h2"], *p["dense"]))
    c["g"] = K.gather_fwd(c["h3"])
    c["m"] = c["g"] @ p["mean"][0] + p["mean"][1]
    c["s"] = c["g"] @ p["std"][0] + p["std"][1]
    c["eps"] = np.asarray(eps, np.float64)
    c["z"], c["kl"] = sample_fwd(c["m"], c["s"], c["eps"])
    c["xf"] = K.graphdense_fwd(c["z"], *p["node"])
    c["u"], c["v"], c["y"] = [], [], []
    for q in p["links"]:
        u = K.graphdense_fwd(c["z"], *q["d1"])
        v = sigmoid(_bn(u, q["bn"], enabled))
        c["u"].append(u)
        c["v"].append(v)
        c["y"].append(sigmoid(K.graphdense_fwd(v, *q["d2"])))
    res = recon_fwd(c["y"], [q["w"] for q in p["links"]], A, c["xf"], x, mask, c["kl"])
    c.update(A=A, mask=mask, enabled=enabled, adjs=adjs)
    return res, c


def backward(p, c, g_opt=1.0, g_sum=0.0):
    """Gradients of g_opt * cost_opt + g_sum * cost_sum with respect to every parameter (same nesting as p)."""
    A, mask, en = c["A"], c["mask"], c["enabled"]
    ws = [q["w"] for q in p["links"]]
    dys, dws, dxf, dkl = recon_bwd(c["y"], ws, A, c["xf"], c["x"], mask, g_opt, g_sum)
    g = {"links": []}
    dz = np.zeros_like(c["z"])
    for q, y, u, v, dy, dw in zip(p["links"], c["y"], c["u"], c["v"], dys, dws):
        dpre = dy * y * (1 - y)
        dv, dk2, db2 = K.graphdense_bwd(v, q["d2"][0], dpre)
        dbn_out = dv * v * (1 - v)
        du, dgam, dbet = K.graph_bn_bwd(u, q["bn"]["gamma"], q["bn"]["mean"], q["bn"]["var"], dbn_out, en)
        dzc, dk1, db1 = K.graphdense_bwd(c["z"], q["d1"][0], du)
        dz += dzc
        g["links"].append(dict(d1=(dk1, db1), bn=dict(gamma=dgam, beta=dbet), d2=(dk2, db2), w=dw))
    dzn, dkn, dbn = K.graphdense_bwd(c["z"], p["node"][0], dxf)
    dz += dzn
    g["node"] = (dkn, dbn)
    dm, ds = sample_bwd(c["m"], c["s"], c["eps"], dz, dkl if g_opt else None)
    g["mean"] = (c["g"].T @ dm, dm.sum(0))
    g["std"] = (c["g"].T @ ds, ds.sum(0))
    dg = dm @ p["mean"][0].T + ds @ p["std"][0].T
    dh3 = K.gather_bwd(dg, c["h3"].shape[1])
    dpre = dh3 * c["h3"] * (1 - c["h3"])
    dh2, dkd, dbd = K.graphdense_bwd(c["h2"], p["dense"][0], dpre)
    g["dense"] = (dkd, dbd)
    dt2 = dh2 * (1 - c["h2"] ** 2)
    da2, dgam2, dbet2 = K.graph_bn_bwd(c["a2"], p["bn2"]["gamma"], p["bn2"]["mean"], p["bn2"]["var"], dt2, en)
    g["bn2"] = dict(gamma=dgam2, beta=dbet2)
    w2, b2 = p["conv2"]
    dh1, dw2, db2 = K.graphconv_bwd(c["h1"], c["adjs"], w2, b2, da2)
    dt1 = dh1 * (1 - c["h1"] ** 2)
    da1, dgam1, dbet1 = K.graph_bn_bwd(c["a1"], p["bn1"]["gamma"], p["bn1"]["mean"], p["bn1"]["var"], dt1, en)
    g["bn1"] = dict(gamma=dgam1, beta=dbet1)
    w1, b1 = p["conv1"]
    _, dw1, db1 = K.graphconv_bwd(c["x"], c["adjs"], w1, b1, da1)
    g["conv1"] = (dw1, db1)
    g["conv2"] = (dw2, db2)
    return g


def literal_cost(p, x, adjs, A, mask, eps, enabled=None):
    """Op-by-op transcription of model_vae.py's graph with the dense [B, C, N, N] logits -> (cost_opt, cost_sum, correct_count)."""
    x = np.asarray(x, np.float64)
    B, N, F = x.shape
    w1, b1 = p["conv1"]
    w2, b2 = p["conv2"]
    layer = np.tanh(_bn(K.graphconv_fwd(x, adjs, w1, b1), p["bn1"], enabled))                 # :75-79
    layer = np.tanh(_bn(K.graphconv_fwd(layer, adjs, w2, b2), p["bn2"], enabled))             # :80-84
    layer = sigmoid(layer.reshape(-1, LATENT) @ p["dense"][0] + p["dense"][1]).reshape(B, N, LATENT)   # :85-86
    layer = layer.sum(axis=1)                                                                 # :87
    mean_layer = np.clip(layer @ p["mean"][0] + p["mean"][1], -100, 100)                      # :89-91, 95
    std_layer = np.clip(np.sqrt(np.log(1 + np.exp(layer @ p["std"][0] + p["std"][1]))), -5, 5)  # :92-94, 96
    mean_t = np.tile(mean_layer.reshape(B, 1, LATENT), (1, N, 1))                             # :170-171
    std_t = np.tile(std_layer.reshape(B, 1, LATENT), (1, N, 1))                               # :172-173
    layer = mean_t + std_t * np.asarray(eps, np.float64)                                      # :175
    kl_el = 1 + 2 * np.log(std_t + KL_EPS) - mean_t ** 2 - std_t                              # :178
    klqp_loss = -1 / 2.0 * kl_el.sum(axis=2).sum(axis=1).mean(axis=0)                         # :179-181
    decoded_features = layer.reshape(-1, LATENT) @ p["node"][0] + p["node"][1]                # :109-111
    decoded_features = decoded_features.reshape(B, N, F)
    decoded = []
    for q in p["links"]:                                                                      # :115-133, 197-199
        h = sigmoid(_bn((layer.reshape(-1, LATENT) @ q["d1"][0] + q["d1"][1]).reshape(B, N, LATENT), q["bn"], enabled))
        h = sigmoid((h.reshape(-1, LATENT) @ q["d2"][0] + q["d2"][1]).reshape(B, N, LATENT))
        decoded.append(np.einsum("bik,bjk->bij", h * q["w"][None, None, :], h))               # GraphDecoderDistMult
    decoded_adjs = np.transpose(np.stack(decoded), [1, 0, 2, 3])                               # :200-201
    pair_adjs = A                                                                             # :204-214
    cost_features = sig_ce(decoded_features, x).mean(axis=2)                                  # :217-222
    cost_links = sig_ce(decoded_adjs, pair_adjs).mean(axis=3).mean(axis=2)                    # :224-228
    cost = mask * (cost_features.mean(axis=1) + cost_links.mean(axis=1))                      # :230-232
    cost_opt = cost.mean() + klqp_loss                                                        # :237
    cost_sum = cost.mean()                                                                    # :239
    correct_exist = ((decoded_adjs.max(axis=1) > 0.0) == (pair_adjs.max(axis=1) > 0.5)).astype(np.float64)  # :244-249
    correct_count = (mask * correct_exist.mean(axis=(1, 2))).sum()                            # :251-253
    return cost_opt, cost_sum, correct_count
