"""Model definitions mirroring the reference's model plugins line for line in LAYER CALLS
(SURVEY 8f, row N1).  The layers of the hot path run in HIP kernels (kgcn_amd.layers); the elementwise
activation the reference writes as its own TF op after a layer (tf.sigmoid(layer), tf.nn.relu(layer)) is
handed to the layer as `activation=` and computed in the epilogue of the kernel that produces the tensor
(aggregation or GEMM) -- same function, one pass over HBM less per layer; where a BatchNormalization sits
between layer and activation it is one HIP elementwise kernel (ops.activation).  The loss is torch.

  GCN  -- example_model/model.py:41-61      GraphConv(50) x3, BN, GraphDense(50), GraphGather, Dense(2)
  GIN  -- example_model/model_gin.py:40-67  2 x [GINAggregate, GraphDense(50) x2], Gather x2, Dense(2)
  GATNet -- example_model/model_gat.py:40-62  3 x [GraphDense(50), GAT], Gather of blocks 2 and 3, Dense(2)
  MultitaskGCN -- example_model/model_multitask.py:45-101  GraphConv 256/256, GraphDense 256, GraphConv 50, BN,
                  GraphDense 50, Gather, Dense(label_dim); masked (weighted) sigmoid cross entropy
  SparseGCN    -- example_model/sparse.py:45-134  block-diagonal batch of one: 3 x [GraphConv(256) relu],
                  GraphDense(256), BN, relu, per-molecule sum, tanh, Dense(num_classes); summed sparse softmax CE
  GraphVAE     -- example_model/model_vae.py:63-253  GraphConv/BN encoder, reparameterisation, node and DistMult link
                  decoders; fused reconstruction loss (csrc/vae.hip)
  MultimodalGCN -- example_model/model_multimodal.py:53-118  GraphConv(50), GraphDense(50), Gather | Embedding, Conv1D(50, 4),
                  MaxPooling1D(4), LSTM(32, go_backwards) (csrc/seq.hip); concat, Dense(52) relu, Dense(label_dim)

  SeqCNN       -- sample_protein/sequence/cnn.py:36-90  Embedding, 3 x [Conv1D relu, MaxPooling1D], Conv1D(1, tanh), BN, Dense(52), BN,
                  relu, Dense(label_dim) (csrc/conv1d.hip); class-weighted softmax CE
  CPIMultitaskNet -- sample_chem/compound-protein_interaction/multitask.py:35-86  GraphConv(512) sigmoid, GraphGather, Dense(2 T)
                  read as [B, 2, T]; two-way softmax cross entropy per task under mask_label (csrc/cvloss.hip)
  MultimodalVecGCN -- example_model/model_multimodal_vec.py:56-127  GraphConv(50), GraphDense(50), Gather | Dense+BN+relu 300/100/64
                  on the per-graph vector (csrc/shortm.hip); concat, Dense(52)+BN+relu, Dense(label_dim); masked softmax CE
  MultimodalRegressionGCN -- example_model/model_multimodal_regression.py:60-101  3 x [GraphDense(32), BN], Gather, tanh |
                  Dense(8)+BN+relu on the vector; concat, Dense(label_dim); masked squared error (csrc/regress.hip)

Keras learning-phase semantics (quirk Q6): the reference calls BatchNormalization / Dropout
without `training=`; under TF1 graph mode that is inference behaviour -- BN normalises with its
moving statistics (0, 1) and Dropout is the identity.  That is what is implemented here
(layers.GraphBatchNormalization).
"""
import math

import torch
from torch import nn

from . import layers, ops, ragged as _ragged


GraphBatchNormalization = layers.GraphBatchNormalization


class KerasDense(nn.Module):
    """K.layers.Dense(units) on [B, D] (model.py:55): kernel glorot-uniform (or `kernel_initializer`, a Keras name such as
    'random_uniform': model_vae.py:89), bias zeros."""

    def __init__(self, units, kernel_initializer="glorot_uniform"):
        super().__init__()
        self.units = units
        self.kernel_initializer = kernel_initializer
        self.kernel = None
        self.bias = None

    def build(self, din, device):
        if self.kernel is None:
            self.kernel = nn.Parameter(layers._init_tensor((din, self.units), self.kernel_initializer, device))
            self.bias = nn.Parameter(torch.zeros(self.units, device=device))

    def forward(self, x):
        self.build(x.shape[1], x.device)
        return ops.dense(x, self.kernel, self.bias)


def masked_softmax_ce(logits, labels, mask):
    """model.py:56-61: cost = mask * softmax_cross_entropy(labels, logits);
    cost_opt = reduce_mean(cost) over the PADDED batch (quirk Q5); cost_sum = reduce_sum(cost).
    One HIP pass (csrc/train.hip: per-graph cost, d cost_sum / d logits, fixed-order sums)."""
    return ops.masked_softmax_ce(logits, labels, mask)


class GCN(nn.Module):
    """example_model/model.py:30-71."""

    def __init__(self, adj_channel_num=1, num_classes=2, ragged=False):
        """ragged: run on the valid node rows only when enabled_node_nums is given (kgcn_amd.ragged; same results as the
        padded formulation, which computes every layer on all max_node_num rows)."""
        super().__init__()
        self.ragged = bool(ragged)
        self.conv1 = layers.GraphConv(50, adj_channel_num, activation="sigmoid")    # :42-43 tf.sigmoid(layer)
        self.conv2 = layers.GraphConv(50, adj_channel_num, activation="sigmoid")    # :44-45
        self.conv3 = layers.GraphConv(50, adj_channel_num)
        self.bn = GraphBatchNormalization(activation="sigmoid")                     # :48-50 tf.sigmoid(bn(...)), one pass
        self.dense = layers.GraphDense(50, activation="sigmoid")                    # :52-53
        self.gather = layers.GraphGather()
        self.out = KerasDense(num_classes)

    def forward(self, features, adjs, enabled_node_nums=None):
        features, adjs, enabled_node_nums, rb = _ragged.enter(self.ragged, features, adjs, enabled_node_nums)
        if rb is None:
            adjs = layers._pack(adjs, features)         # list-of-lists feed: packed ONCE per forward, not per layer
            # small graphs (N <= 32, widths <= 64, one channel): the whole node-level body in one launch per direction
            pooled = layers.fused_stack([self.conv1, self.conv2, self.conv3, self.bn, self.dense], features, adjs,
                                        enabled_node_nums=enabled_node_nums, gather=True)
            if pooled is not None:
                return self.out(pooled)
        layer = self.conv1(features, adj=adjs)
        layer = self.conv2(layer, adj=adjs)
        layer = self.conv3(layer, adj=adjs)
        layer = self.bn(layer, max_node_num=features.shape[1], enabled_node_nums=enabled_node_nums)
        # K.layers.Dropout(dropout_rate): identity (Q6)
        layer = self.dense(layer)
        layer = self.gather(layer, ragged=rb)
        return self.out(layer)


_GIN_JOIN = __import__("os").environ.get("KGCN_GIN_JOIN") != "0"          # (development A/B: "0" = torch.cat of the read-outs)


class GIN(nn.Module):
    """example_model/model_gin.py:29-78."""

    def __init__(self, adj_channel_num=1, num_classes=2, width=50):
        """width: units of the four GraphDense layers (50 in the file; BASELINE config 5 quotes the layer at 256)."""
        super().__init__()
        self.agg = nn.ModuleList([layers.GINAggregate(adj_channel_num) for _ in range(2)])
        self.dense = nn.ModuleList([layers.GraphDense(width, activation="relu") for _ in range(4)])   # :45-54 tf.nn.relu
        self.gather = layers.GraphGather()
        self.out = KerasDense(num_classes)

    def forward(self, features, adjs, enabled_node_nums=None):
        adjs = layers._pack(adjs, features)
        layer = features
        outs = []
        # tf.concat of the two read-outs (model_gin.py:61): each is written into its column block of ONE buffer (and its gradient
        # read out of the column block of d buffer): no concatenation pass, no copies of the strided gradient blocks
        width = self.dense[1].output_dim
        joined = features.new_empty((features.shape[0], 2 * width)) if width % 4 == 0 and _GIN_JOIN else None
        for blk in range(2):
            # (block 0: the features need no gradient, so d epsilon is formed inside the dense layer's dX GEMM -- layers.gin_graph_dense)
            layer = layers.gin_graph_dense(self.agg[blk], self.dense[2 * blk], layer, adj=adjs)
            # the block output is read out (and, for block 0, passed on): d pooled joins the gradient inside the layer's dX GEMM
            layer, pooled = layers.graph_dense_gather(self.dense[2 * blk + 1], layer, join=joined, join_col=blk * width)
            outs.append(pooled)
        return self.out(torch.cat(outs, dim=1) if joined is None else ops.join_columns(joined, outs))


def masked_sigmoid_ce(logits, labels, mask, mask_label, pos_weight=None):
    """model_multitask.py:66-79: cost = mask * sum_tasks mask_label * (weighted) sigmoid cross entropy;
    cost_opt = reduce_mean over the padded batch, cost_sum = reduce_sum.  Formulas of
    tf.nn.sigmoid_cross_entropy_with_logits / tf.nn.weighted_cross_entropy_with_logits; one HIP pass (csrc/train.hip)."""
    return ops.masked_sigmoid_ce(logits, labels, mask, mask_label, pos_weight)


def sparse_softmax_ce_sum(logits, labels):
    """sparse.py:112-113: loss_to_minimize = reduce_sum(sparse_softmax_cross_entropy_with_logits)."""
    return ops.sparse_softmax_ce_sum(logits, labels)


class MultitaskGCN(nn.Module):
    """example_model/model_multitask.py:32-101."""

    def __init__(self, adj_channel_num=1, label_dim=12, ragged=False):
        """ragged: run on the valid node rows only when enabled_node_nums is given (kgcn_amd.ragged) -- the reference
        computes GraphConv / GraphDense on all max_node_num rows and only its BN on the valid ones (:58-60); the results
        are the same, the padded rows' constant contribution to GraphGather included."""
        super().__init__()
        self.ragged = bool(ragged)
        self.conv1 = layers.GraphConv(256, adj_channel_num, activation="sigmoid")   # :51-52
        self.conv2 = layers.GraphConv(256, adj_channel_num, activation="sigmoid")   # :53-54
        self.dense1 = layers.GraphDense(256, activation="sigmoid")                  # :55-56
        self.conv3 = layers.GraphConv(50, adj_channel_num)
        self.bn = layers.GraphBatchNormalization(activation="sigmoid")              # :58-60 tf.sigmoid(bn(...)), one pass
        self.dense2 = layers.GraphDense(50, activation="sigmoid")                   # :61-62
        self.gather = layers.GraphGather()
        self.out = KerasDense(label_dim)

    def forward(self, features, adjs, enabled_node_nums=None):
        features, adjs, enabled_node_nums, rb = _ragged.enter(self.ragged, features, adjs, enabled_node_nums)
        if rb is None:
            adjs = layers._pack(adjs, features)
        layer = self.conv1(features, adj=adjs)
        layer = self.conv2(layer, adj=adjs)
        layer = self.dense1(layer)
        layer = self.conv3(layer, adj=adjs)
        layer = self.bn(layer, max_node_num=features.shape[1], enabled_node_nums=enabled_node_nums)
        layer = self.dense2(layer)
        layer = self.gather(layer, ragged=rb)
        return self.out(layer)                      # prediction = sigmoid(logits)


class CPIMultitaskNet(nn.Module):
    """sample_chem/compound-protein_interaction/multitask.py:35-51 (singletask.py: label_dim = 1): GraphConv(512) -> sigmoid ->
    GraphGather -> Dense(2 label_dim), read as logits [B, 2, label_dim] (logits[b, c, t] = out[b, c label_dim + t]) with a
    two-way softmax per task.  enabled_node_nums is accepted and unused, as in the file."""

    WIDTH = 512

    def __init__(self, adj_channel_num=1, label_dim=1):
        super().__init__()
        self.label_dim = int(label_dim)
        self.conv = layers.GraphConv(self.WIDTH, adj_channel_num, activation="sigmoid")     # :39-40
        self.gather = layers.GraphGather()                                                  # :41
        self.out = KerasDense(2 * self.label_dim)                                           # :42

    def forward(self, features, adjs, enabled_node_nums=None):
        adjs = layers._pack(adjs, features)
        layer = self.gather(self.conv(features, adj=adjs))
        return self.out(layer).view(-1, 2, self.label_dim)                                  # :44

    @staticmethod
    def loss(logits, labels, mask_label, accum=None):
        """compute_metrics (:53-86) -> (cost_opt, cost_sum): the same tensor, the sum over tasks of the summed cross entropy
        of the rows with mask_label != 0.  accum: ops.multitask_softmax2_ce's device accumulator block."""
        cost = ops.multitask_softmax2_ce(logits, labels, mask_label, accum=accum)[0]
        return cost, cost


def wants_augmented_features(model, n_features):
    """True when `model`'s first layer is a one-kernel-per-step consumer of [x | 1 | 0] feature rows: a GraphConv that takes the
    aggregate-first route (layers.py: din + 1 padded to 4 below its width), so that a static ragged batch should assemble its rows
    in that form (data_util.DeviceGraphDataset.static_ragged_batch(augmented_features=True))."""
    first = next((m for m in model.children() if isinstance(m, (layers.GraphConv, layers.GraphDense, layers.GINAggregate))), None)
    if not isinstance(first, layers.GraphConv) or not getattr(model, "ragged", False):
        return False
    dp = (int(n_features) + 1 + 3) // 4 * 4
    return bool(layers.aggregate_first and dp < first.output_dim and not (layers.enabled_bconv or layers.enabled_bspmm or
                                                                          layers.enabled_batched))


class SparseGCN(nn.Module):
    """example_model/sparse.py:45-134 (params of build(): out_dims [256,256,256], dense_dim 256,
    batch_normalize False, max_pool False; both optional layers are available as flags)."""

    def __init__(self, num_classes, adj_channel_num=1, out_dims=(256, 256, 256), dense_dim=256,
                 batch_normalize=False, max_pool=False):
        super().__init__()
        fuse = None if (batch_normalize or max_pool) else "relu"        # relu directly behind the layer: in its epilogue
        self.convs = nn.ModuleList([layers.GraphConv(o, adj_channel_num, activation=fuse) for o in out_dims])
        self.pools = nn.ModuleList([layers.GraphMaxPooling(adj_channel_num) for _ in out_dims]) if max_pool else None
        self.bns = nn.ModuleList([layers.GraphBatchNormalization() for _ in out_dims]) if batch_normalize else None
        self.dense = layers.GraphDense(dense_dim)
        self.bn = layers.GraphBatchNormalization(activation="relu")     # tf.nn.relu(bn(dense)), one pass
        self.out = KerasDense(num_classes)

    def forward(self, batch):
        """batch: kgcn_amd.data_util.BlockDiagonalBatch."""
        net = batch.features.unsqueeze(0)                       # tf.expand_dims(net, 0)
        for i, conv in enumerate(self.convs):
            net = conv(net, batch.adjacency)                    # positional adj, sparse.py:69
            if self.pools is not None:
                net = self.pools[i](net, batch.adjacency)
            if self.bns is not None:
                net = self.bns[i](net)
            if conv.activation is None:
                net = ops.activation(net, "relu")
        net = self.bn(self.dense(net))
        net = net.reshape(net.shape[1], net.shape[2])           # (a view: indexing [0] costs a zero fill + a copy in backward)
        # per-molecule node sum (:83-94) with tf.tanh (:95) in the aggregation's epilogue; its derivative rides in the adjoint
        net = ops.bconv(batch.segments_adjacency(), net, net.shape[1], activation="tanh")
        return self.out(net)                                    # probabilities = softmax(logits)


class DeepChemGCN(nn.Module):
    """example_model/model_deepchem.py:31-81: 4 x [GraphConv(64 / 128 / 128 / 64) -> relu -> GraphMaxPooling ->
    GraphBatchNormalization (valid rows) -> Dropout], GraphDense(64) -> sigmoid, GraphGather, Dense(num_classes).
    dropout_rate: the `dropout_rate` placeholder (0 = the evaluation feed; torch's dropout mask otherwise)."""

    def __init__(self, adj_channel_num=1, num_classes=2, widths=(64, 128, 128, 64)):
        super().__init__()
        self.conv = nn.ModuleList([layers.GraphConv(w, adj_channel_num, activation="relu") for w in widths])   # :44-45 tf.nn.relu(conv)
        self.pool = nn.ModuleList([layers.GraphMaxPooling(adj_channel_num) for _ in widths])
        self.bn = nn.ModuleList([GraphBatchNormalization() for _ in widths])
        self.dense = layers.GraphDense(64, activation="sigmoid")                                              # :75-76
        self.gather = layers.GraphGather()
        self.out = KerasDense(num_classes)

    def forward(self, features, adjs, enabled_node_nums=None, dropout_rate=0.0):
        adjs = layers._pack(adjs, features)
        layer = features
        for conv, pool, bn in zip(self.conv, self.pool, self.bn):
            layer = bn(pool(conv(layer, adj=adjs), adj=adjs), enabled_node_nums=enabled_node_nums)
            if dropout_rate:
                layer = torch.nn.functional.dropout(layer, p=float(dropout_rate), training=True)
        return self.out(self.gather(self.dense(layer)))


class NodeLabelGCN(nn.Module):
    """example_model/model_node_label.py:48-62 (features given): GraphConv(64) -> GraphBatchNormalization -> relu, twice, then
    GraphConv(num_classes): per-NODE logits [B, N, num_classes]."""

    def __init__(self, adj_channel_num=1, num_classes=2):
        super().__init__()
        self.conv = nn.ModuleList([layers.GraphConv(64, adj_channel_num), layers.GraphConv(64, adj_channel_num),
                                   layers.GraphConv(num_classes, adj_channel_num)])
        self.bn = nn.ModuleList([GraphBatchNormalization(activation="relu") for _ in range(2)])       # :52-55 tf.nn.relu(bn(...))

    def forward(self, features, adjs, enabled_node_nums=None):
        adjs = layers._pack(adjs, features)
        layer = features
        for conv, bn in zip(self.conv[:2], self.bn):
            layer = bn(conv(layer, adj=adjs), enabled_node_nums=enabled_node_nums)
        return self.conv[2](layer, adj=adjs)


def node_softmax_ce(logits, node_labels, mask):
    """model_node_label.py:64-70: cost[b] = mask[b] * mean over ALL N node rows of softmax_cross_entropy(node_label[b, n],
    logits[b, n]) (the mask_node_label placeholder is read but not used there); cost_opt = reduce_mean over the padded batch,
    cost_sum = reduce_sum.  -> (cost_opt, cost_sum)"""
    ce = -(node_labels * torch.log_softmax(logits, dim=2)).sum(dim=2)
    cost = mask * ce.mean(dim=1)
    return cost.mean(), cost.sum()


class GATNet(nn.Module):
    """example_model/model_gat.py:30-80."""

    def __init__(self, adj_channel_num=1, num_classes=2):
        super().__init__()
        self.dense = nn.ModuleList([layers.GraphDense(50) for _ in range(3)])
        self.gat = nn.ModuleList([layers.GAT(adj_channel_num) for _ in range(3)])
        self.gather = layers.GraphGather()
        self.out = KerasDense(num_classes)

    def forward(self, features, adjs, enabled_node_nums=None):
        adjs = layers._pack(adjs, features)
        layer = features
        block_out = []
        for i in range(3):
            layer = self.gat[i](self.dense[i](layer), adj=adjs)
            if i > 0:
                block_out.append(layer)
        return self.out(torch.cat([self.gather(o) for o in block_out], dim=1))


class _LinkDecoder(nn.Module):
    """decode_links of example_model/model_vae.py:115-133 for one adjacency channel: GraphDense(64), BN, sigmoid,
    GraphDense(64), sigmoid, GraphDecoderDistMult (whose [B, N, N] product is left to ops.vae_recon)."""

    def __init__(self):
        super().__init__()
        self.dense1 = layers.GraphDense(64)                                   # :124
        self.bn = GraphBatchNormalization(activation="sigmoid")               # :125-128 tf.sigmoid(bn(...)), one pass
        self.dense2 = layers.GraphDense(64, activation="sigmoid")             # :129-130
        self.distmult = layers.GraphDecoderDistMult()                         # :132

    def forward(self, z, n_nodes, enabled_node_nums=None):
        y = self.dense2(self.bn(self.dense1(z), max_node_num=n_nodes, enabled_node_nums=enabled_node_nums))
        if not self.distmult.built:
            self.distmult.build(y.shape, y.device)
        return y, self.distmult.w[0]


class GraphVAE(nn.Module):
    """example_model/model_vae.py (the kgcn-gen graph VAE of example_config/vae.json), call by call:
      encode (:63-97)   GraphConv(64), BN, tanh, GraphConv(64), BN, tanh, GraphDense(64), sigmoid, GraphGather,
                        Dense(64, random_uniform) -> mean, Dense(64) -> std
      sample (:164-181) ops.vae_sample: mean = clip(., -100, 100), std = clip(sqrt(softplus(.)), -5, 5), z = mean + std eps
                        on all N rows, the per-graph KL sum (csrc/vae.hip)
      decode_nodes (:100-112)  GraphDense(F, random_uniform)
      decode_links (:115-133)  per channel GraphDense(64), BN, sigmoid, GraphDense(64), sigmoid, GraphDecoderDistMult
      cost (:203-253)   ops.vae_recon: node-feature and link sigmoid CE, correct_exist; the [B, C, N, N] logits are never formed.

    forward(features, adjs, graph_mask=None, enabled_node_nums=None, eps=None) -> cost_opt (0-d tensor); cost_sum and
    correct_count of the same call are left in .cost_sum / .correct_count, so that loss(out, labels, mask) -> (cost_opt,
    cost_sum) lets train.GraphedTrainStep train it unchanged: the reference's `mask` (1 per real graph, 0 per dummy) reaches the
    model as the fwd_kwarg graph_mask (the step's own `mask` argument is not passed to models).  eps: the reference's `epsilon` placeholder
    [B, N, 64]; None draws the Philox noise of (seed, *step) -- bind_step(optimizer._t_dev) makes it a function of the training
    step, read on the device, so every hipGraph replay draws fresh noise and eager and replayed steps match bit for bit.
    The autoencoder's target is its input: pair adjacency = adjs, pair features = features.

    Reference quirks kept:
      - the KL term is 1 + 2 log(std + 1e-10) - mean^2 - std (-std, not -std^2), summed over the N tiled copies of the latent
        rows (:170-180), and averaged over the PADDED batch: dummy graphs count and the mask is not applied to it (:181);
      - the reconstruction counts padded node rows and columns: N = graph_node_num, label 0 there (:208-228);
      - cost_sum = reduce_mean(cost) (:239), not a sum;
      - the gradient of tf.clip_by_value passes at equality (TF's _ClipByValueGrad);
      - BN in Keras inference mode with its moving statistics (quirk Q6).
    Limits of the fused loss: N <= 128, C <= 8 (ops.vae_recon raises beyond them)."""

    def __init__(self, feature_dim, adj_channel_num=1, seed=0):
        super().__init__()
        C = int(adj_channel_num)
        self.seed = int(seed)
        self.step = None
        self.conv1 = layers.GraphConv(64, C)                                  # :75
        self.bn1 = GraphBatchNormalization(activation="tanh")                 # :76-79 tf.tanh(bn(...)), one pass
        self.conv2 = layers.GraphConv(64, C)                                  # :80
        self.bn2 = GraphBatchNormalization(activation="tanh")                 # :81-84
        self.dense = layers.GraphDense(64, activation="sigmoid")              # :85-86
        self.gather = layers.GraphGather()                                    # :87
        self.mean = KerasDense(64, kernel_initializer="random_uniform")       # :89-91
        self.std = KerasDense(64)                                             # :92
        self.node_decoder = layers.GraphDense(int(feature_dim), kernel_initializer="random_uniform")   # :109-111
        self.link_decoders = nn.ModuleList([_LinkDecoder() for _ in range(C)])                        # :196-199
        self.cost_sum = self.correct_count = None

    def bind_step(self, step):
        """step: a one-element int64 device tensor (TFAdam._t_dev) the noise kernels read at run time; None: step 0."""
        self.step = step
        return self

    def _encode_decode(self, features, adjs, enabled_node_nums, eps):
        adj = layers._pack(adjs, features)
        N = features.shape[1]
        h = self.bn1(self.conv1(features, adj=adj), max_node_num=N, enabled_node_nums=enabled_node_nums)
        h = self.bn2(self.conv2(h, adj=adj), max_node_num=N, enabled_node_nums=enabled_node_nums)
        g = self.gather(self.dense(h))
        # the mean and std Dense layers (:89-92) as one GEMM over [W_mean | W_std]
        self.mean.build(g.shape[1], g.device)
        self.std.build(g.shape[1], g.device)
        wcat, bcat = ops.cat_channels([self.mean.kernel, self.std.kernel], [self.mean.bias, self.std.bias])
        ms = ops.dense(g, wcat, bcat)
        kl, *zs = ops.vae_sample(ms, N, eps, self.seed, self.step, copies=1 + len(self.link_decoders))
        xf = self.node_decoder(zs[0])
        dec = [d(z, N, enabled_node_nums) for d, z in zip(self.link_decoders, zs[1:])]
        return adj, kl, xf, [y for y, _ in dec], [w for _, w in dec]

    def forward(self, features, adjs, graph_mask=None, enabled_node_nums=None, eps=None):
        adj, kl, xf, ys, ws = self._encode_decode(features, adjs, enabled_node_nums, eps)
        cost_opt, cost_sum, correct_count = ops.vae_recon(adj, ys, ws, xf, features, graph_mask, kl)
        # detached: a kept reference must not hold this call's autograd graph (GraphedTrainStep's capture needs none alive)
        self.cost_sum, self.correct_count = cost_sum.detach(), correct_count.detach()
        return cost_opt

    def loss(self, out, labels=None, mask=None):
        """loss_fn for train.train_step / GraphedTrainStep: (cost_opt, cost_sum) of the forward call that produced `out`."""
        return out, self.cost_sum

    @torch.no_grad()
    def reconstruct(self, features, adjs, enabled_node_nums=None, eps=None):
        """The reference's `prediction` (:255-258): (sigmoid(decoded features) [B, N, F], sigmoid(decoded adjacency)
        [B, C, N, N]) -- the dense adjacency is the output here, so it is materialised (ops.gram per channel)."""
        _, _, xf, ys, ws = self._encode_decode(features, adjs, enabled_node_nums, eps)
        adj = torch.stack([ops.gram(y, w) for y, w in zip(ys, ws)], dim=1)
        return ops.activation(xf, "sigmoid"), ops.activation(adj, "sigmoid")


class MultimodalGCN(nn.Module):
    """example_model/model_multimodal.py:53-118 (example_config/multimodal.json, the compound-protein interaction model), call by call:
      graph branch (:60-66)    GraphConv(50, C) sigmoid, GraphDense(50) sigmoid, GraphGather -> [B, 50] (the file's
                               graph_output_layer_dim = 32 is unused)
      sequence branch (:70-93) layers.SequenceEncoder: Embedding(S, E), Conv1D(50, 4, same, relu), MaxPooling1D(4),
                               LSTM(32, go_backwards=True) -> [B, 32]
      shared part (:98-105)    concat([sequence, graph]) -> Dense(52) relu -> Dense(label_dim); loss masked_softmax_ce.
    The activations ride in the epilogues of the producing kernels; the concatenation is one [B, 82] buffer whose columns 0-31
    the LSTM kernel writes and 32-81 the graph read-out (ops.join_columns), so nothing is copied.
    forward(features, adjs, sequences=None, enabled_node_nums=None) -> logits; `sequences` is the int32 [B, L] token batch
    (data_util.sequence_table; GraphedTrainStep passes it as a forward kwarg).  enabled_node_nums is accepted and unused, as in
    the file (every node row, padding included, reaches the read-out).
    sequence_scale / sequence_rep (integrated gradients, visualization.multimodal_integrated_gradients): `sequences` holds
    B / rep token rows, row b of the batch runs the sequence branch on token row b // rep with its embedded input times
    sequence_scale[b] (SequenceEncoder.scaled); the default None keeps the training path above.
    The batch rows never mix (no dropout, no batch normalisation), which is what lets the attribution batch scaled copies."""

    ROW_INDEPENDENT = True

    GRAPH_WIDTH, SEQ_WIDTH, HIDDEN = 50, 32, 52

    def __init__(self, sequence_symbol_num, embedding_dim=4, adj_channel_num=1, label_dim=2, recurrent_activation="hard_sigmoid"):
        super().__init__()
        self.conv = layers.GraphConv(self.GRAPH_WIDTH, adj_channel_num, activation="sigmoid")     # :60-61
        self.dense = layers.GraphDense(self.GRAPH_WIDTH, activation="sigmoid")                    # :62-63
        self.sequence = layers.SequenceEncoder(sequence_symbol_num, embedding_dim, filters=50, kernel_size=4, pool=4,
                                               units=self.SEQ_WIDTH, recurrent_activation=recurrent_activation)   # :73-91
        self.hidden = KerasDense(self.HIDDEN)                                                     # :101-103
        self.out = KerasDense(int(label_dim))                                                     # :104

    def forward(self, features, adjs, sequences=None, enabled_node_nums=None, sequence_scale=None, sequence_rep=1):
        return self.run(features, adjs, sequences, sequence_scale, sequence_rep)[0]

    def run(self, features, adjs, sequences, sequence_scale=None, sequence_rep=1, input_grad=False, sequence_noise=None):
        """forward() -> (logits, pooled, arg-max bytes); the last two are None on the default path, and with sequence_scale they are
        what SequenceEncoder.scaled returns (input_grad: pooled is a leaf that requires grad).  sequence_noise (with
        sequence_scale only) is SequenceEncoder.scaled's noise = (sigma, sample, ids, seed)."""
        if sequences is None:
            raise ValueError("MultimodalGCN needs the sequences= token batch")
        adj = layers._pack(adjs, features)
        B = features.shape[0]
        rep = 1 if sequence_scale is None else int(sequence_rep)
        if sequences.shape[0] * rep != B:
            raise ValueError("%d sequences for %d graphs" % (sequences.shape[0], B) if rep == 1 else
                             "%d sequences x %d copies for %d graphs" % (sequences.shape[0], rep, B))
        joined = features.new_empty((B, self.SEQ_WIDTH + self.GRAPH_WIDTH))
        pooled = arg = None
        if sequence_scale is None:
            if sequence_noise is not None:
                raise ValueError("sequence_noise needs sequence_scale")
            seq = self.sequence(sequences, out=joined, out_col=0)
        else:
            seq, pooled, arg = self.sequence.scaled(sequences, sequence_scale, rep, out=joined, out_col=0, input_grad=input_grad,
                                                    noise=sequence_noise)
        node = self.dense(self.conv(features, adj=adj))
        graph = ops.graph_gather_into(node, joined, self.SEQ_WIDTH)
        layer = ops.join_columns(joined, [seq, graph])                                            # :96 tf.concat
        self.hidden.build(layer.shape[1], layer.device)
        layer = ops.dense(layer, self.hidden.kernel, self.hidden.bias, activation="relu")
        return self.out(layer), pooled, arg

    @staticmethod
    def loss(logits, labels, mask):
        """model_multimodal.py:108-113 -> (cost_opt, cost_sum); correct_count (:115-118) is read off the logits by the caller."""
        return masked_softmax_ce(logits, labels, mask)


class LinkPredictionNet(nn.Module):
    """sample_kg/network_prediction/model_py/{gcn,distmult,ip}.py (config/config_*.json: with_feature false, with_node_embedding
    true, embedding_dim 128), call by call:
      embedding    K.layers.Embedding(N, 128) of nodes = 0 .. N-1: the table itself is the input, U(-0.05, 0.05) (Keras 'uniform')
      gcn (:41-46) GraphConv(128) relu, GraphConv(128) relu on the one graph (relu in the aggregation epilogue)
      distmult     kgcn.layers.DistMult relation vectors, glorot, one per relation id: [num_relations, 128] (the file builds
                   adj_channel_num = 1 rows and gathers ids 2 and 0 from it, out of range; sized by the largest id here)
      loss         ops.linkpred_loss (csrc/linkpred.hip): the four gathers, s1 / s2, the ranking cost and its metrics.
    forward(features, adjs, feed=None) -> cost_opt; cost_sum, correct_count, s1, s2 and the assembled rows of the same call are
    left in .cost_sum / .correct_count / .s1 / .s2 / .rows (detached), so loss(out, labels, mask) -> (cost_opt, cost_sum) lets
    train.GraphedTrainStep train it unchanged (feed= as a forward kwarg; features is unused).  bind_step(optimizer._t_dev)
    makes the label window and the negatives of step t a function of (seed, t), read on the device."""

    VARIANTS = ("gcn", "distmult", "ip")

    def __init__(self, variant, num_nodes, num_relations=1, embedding_dim=128, seed=0, device=None):
        super().__init__()
        if variant not in self.VARIANTS:
            raise ValueError("variant must be one of %s (model_py/gin.py is not supported)" % (self.VARIANTS,))
        self.variant, self.num_nodes, self.seed = variant, int(num_nodes), int(seed)
        self.step = None
        self.embedding = nn.Parameter(layers._init_tensor((self.num_nodes, int(embedding_dim)), "random_uniform", device))
        if variant == "gcn":
            self.conv1 = layers.GraphConv(128, 1, activation="relu")          # gcn.py:41-42
            self.conv2 = layers.GraphConv(128, 1, activation="relu")          # gcn.py:44-45
        self.distmult = None
        if variant == "distmult":
            self.distmult = layers.DistMult(adj_channel_num=int(num_relations))    # distmult.py:42
            self.distmult.build((1, self.num_nodes, int(embedding_dim)), device)
        self.cost_sum = self.correct_count = self.s1 = self.s2 = self.rows = None

    def bind_step(self, step):
        """step: a one-element int64 device tensor (TFAdam._t_dev) the feed kernel reads at run time; None: step 0."""
        self.step = step
        return self

    def node_rows(self, adjs=None):
        """The model's `prediction` [N, D]: the embedding table (distmult, ip) or the two GraphConv layers over it (gcn)."""
        if self.variant != "gcn":
            return self.embedding
        if adjs is None:
            raise ValueError("the gcn variant needs the graph (adjs)")
        x = self.embedding.view(1, self.num_nodes, -1)
        x = self.conv2(self.conv1(x, adj=adjs), adj=adjs)
        return x.view(self.num_nodes, -1)

    def forward(self, features, adjs, feed=None, seed=None, step=None):
        if feed is None:
            raise ValueError("LinkPredictionNet needs the feed= label list (data_util.LinkPredFeed)")
        h = self.node_rows(adjs)
        w = self.distmult.w[0] if self.distmult is not None else None
        cost_opt, cost_sum, correct, s1, s2, rows = ops.linkpred_loss(h, feed, self.variant, w=w,
                                                                      seed=self.seed if seed is None else seed,
                                                                      step=self.step if step is None else step)
        self.cost_sum, self.correct_count, self.s1, self.s2, self.rows = cost_sum.detach(), correct, s1, s2, rows
        return cost_opt

    def loss(self, out, labels=None, mask=None):
        """loss_fn for train.train_step / GraphedTrainStep: (cost_opt, cost_sum) of the forward call that produced `out`."""
        return out, self.cost_sum

    @torch.no_grad()
    def predict(self, adjs=None):
        """(lp_prediction, prediction): H H^T [1, N, N] (gcn, ip) or the DistMult layer's [1, R, N, N] = H diag(w_r) H^T, and the
        node rows H [N, D] (the reference's model.out) -- on the dense GEMM (ops.dense), H^T and H diag(w_r) formed once."""
        h = self.node_rows(adjs).contiguous()
        ht = h.t().contiguous()
        if self.distmult is None:
            return ops.dense(h, ht).unsqueeze(0), h
        w = self.distmult.w[0]
        return torch.stack([ops.dense(h * w[r], ht) for r in range(w.shape[0])]).unsqueeze(0), h

    @torch.no_grad()
    def rank_links(self, adjs, label_list, test_label_list, relation=None, cutoff=10000):
        """run_enrichment.sh on this model (kgcn_amd.predscore.rank_links): all node pairs in score order with their train /
        test / new marks and the enrichment of the test edges, from node_rows(adjs) without the [N, N] prediction.  distmult
        ranks ONE relation's scores, H diag(w[relation]) H^T: `relation` is required there and refused elsewhere."""
        from . import predscore
        if (self.distmult is not None) != (relation is not None):
            raise ValueError("rank_links: relation= is required by 'distmult' and only by it")
        w = None
        if relation is not None:
            if not 0 <= int(relation) < self.distmult.w[0].shape[0]:
                raise ValueError("rank_links: relation %d outside [0, %d)" % (int(relation), self.distmult.w[0].shape[0]))
            w = self.distmult.w[0][int(relation)]
        return predscore.rank_links(self.node_rows(adjs).contiguous(), label_list, test_label_list, w=w, cutoff=cutoff)


class KerasBatchNorm(nn.Module):
    """K.layers.BatchNormalization() on [B, D], called without `training=` (sample_protein/sequence/cnn.py:74, :76): under the
    TF1 learning phase 0 (quirk Q6, the module docstring) it normalises with its moving statistics, which start at mean 0 /
    variance 1 and are never updated, while the trainable gamma (ones) / beta (zeros) receive gradients:
      y = act(gamma x / sqrt(1 + 1e-3) + beta).
    The per-channel affine (and a following relu) is the GraphBatchNormalization kernel in inference mode on a [B, 1, D] view."""

    def __init__(self, eps=1e-3, activation=None):
        super().__init__()
        self.eps, self.activation = eps, activation
        self.gamma = None
        self.beta = None

    def build(self, d, device):
        if self.gamma is None:
            self.gamma = nn.Parameter(torch.ones(d, device=device))
            self.beta = nn.Parameter(torch.zeros(d, device=device))
            self.register_buffer("moving_mean", torch.zeros(d, device=device))
            self.register_buffer("moving_variance", torch.ones(d, device=device))

    def forward(self, x):
        B, D = x.shape
        self.build(D, x.device)
        y = ops.graph_bn(x.reshape(B, 1, D), self.gamma, self.beta, self.moving_mean, self.moving_variance, None, self.eps, False,
                         self.activation)
        return y.reshape(B, D)


class SeqCNN(nn.Module):
    """sample_protein/sequence/cnn.py:36-90 (config_cnn.json: embedding_dim 25, batch_size 1, learning_rate 1e-4), call by call:
      :37      Embedding(sequence_symbol_num, embedding_dim)     embeddings [S, E], U(-0.05, 0.05); gathered inside the first
                                                                 conv kernel (token mode), never written
      :39-42   feed_embedded_layer                               forward(embedded=[B, L, E]): the first layer reads it (dense mode)
      :45-48   Conv1D(505, 4, same, relu), MaxPooling1D(4)       layers.Conv1DPool, one launch each
      :50-53   Conv1D(200, 3, same, relu), MaxPooling1D(3)
      :55-58   Conv1D(100, 2, same, relu), MaxPooling1D(2)
      :60-62   Conv1D(1, 2, same, tanh), tf.squeeze              [B, T3, 1] -> [B, T3].  The reference's squeeze drops the batch
                                                                 axis at B = 1 and repairs it (:64-66); here [B, T3] always
      :74-77   BatchNormalization, Dense(52), BatchNormalization, relu    KerasBatchNorm (learning phase 0), KerasDense
      :79      Dense(label_dim)                                  logits
    forward(features, adjs, sequences=None, embedded=None) -> logits [B, label_dim]; features / adjs are accepted and unused (the
    sample's dataset carries a dummy 2 x 2 graph), `sequences` is the int32 [B, L] token batch (data_util.sequence_table;
    GraphedTrainStep passes it as a forward kwarg).  The gradient with respect to `embedded` comes through autograd (what
    kgcn visualize --ig_label_target differentiates).  Dense(52) fixes the model to one sequence length."""

    ROW_INDEPENDENT = True

    WIDTHS, KERNELS, HIDDEN = (505, 200, 100), (4, 3, 2), 52

    def __init__(self, sequence_symbol_num, embedding_dim=25, label_dim=2, class_weight=None):
        super().__init__()
        ops.conv1d_limits_check(symbols=sequence_symbol_num, in_dim=embedding_dim)
        self.label_dim = int(label_dim)
        self.embeddings = nn.Parameter(torch.empty(int(sequence_symbol_num), int(embedding_dim)).uniform_(-0.05, 0.05))   # :37
        self.convs = nn.ModuleList([layers.Conv1DPool(f, k, k, "relu") for f, k in zip(self.WIDTHS, self.KERNELS)])  # :45-58
        self.conv_out = layers.Conv1DPool(1, self.KERNELS[-1], 1, "tanh")                         # :60-61
        self.bn1 = KerasBatchNorm()                                                               # :74
        self.hidden = KerasDense(self.HIDDEN)                                                     # :75
        self.bn2 = KerasBatchNorm(activation="relu")                                              # :76-77
        self.out = KerasDense(self.label_dim)                                                     # :79
        cw = torch.ones(self.label_dim) if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1)
        if cw.numel() != self.label_dim:
            raise ValueError("class_weight has %d entries for %d classes" % (cw.numel(), self.label_dim))
        self.register_buffer("class_weight", cw)

    def forward(self, features=None, adjs=None, sequences=None, embedded=None, first=None):
        if first is not None:                                                                     # the first layer's output itself
            layer = first
        elif embedded is not None:
            layer = self.convs[0](embedded)                                                       # :39-40
        elif sequences is not None:
            layer = self.convs[0](tokens=sequences, table=self.embeddings)
        else:
            raise ValueError("SeqCNN needs the sequences= token batch (or embedded=)")
        layer = self.convs[2](self.convs[1](layer))
        layer = self.conv_out(layer)
        layer = layer.reshape(layer.shape[0], layer.shape[1])                                     # :62-66
        layer = self.bn2(self.hidden(self.bn1(layer)))
        return self.out(layer)

    def loss(self, logits, labels, mask=None):
        """cnn.py:84-90 -> (cost_opt, cost_sum): cost_b = softmax CE, cost_sum = sum_b mask_b cost_b (unweighted, :90), and
        cost_opt = reduce_mean(cost * labels * class_weight) (:85-87).  That product broadcasts cost [B] against [B, C], which is
        defined at B = 1 only (the config's batch size), where it is cost_0 class_weight[label_0] / C; here, for any B,
          cost_opt = (1 / (B C)) sum_b mask_b cost_b class_weight[label_b]
        (a deviation for B > 1, where the reference expression fails to broadcast or, at B = C, pairs costs with other rows'
        labels).  Both sums are the masked-CE kernel with the per-row weight as its mask operand."""
        labels = labels.to(torch.float32)
        B, C = labels.shape
        mask = torch.ones(B, device=labels.device) if mask is None else mask.to(torch.float32).reshape(-1)
        row_weight = mask * (labels * self.class_weight).sum(dim=1) * (1.0 / C)
        cost_opt, _ = ops.masked_softmax_ce(logits, labels, row_weight)
        _, cost_sum = ops.masked_softmax_ce(logits, labels, mask)
        return cost_opt, cost_sum


class KerasDenseBN(nn.Module):
    """K.layers.Dense(units) -> K.layers.BatchNormalization() -> activation on [B, D] (model_multimodal_vec.py:84-86): kernel
    glorot-uniform, bias zeros, gamma ones, beta zeros, moving mean 0 / variance 1, eps 1e-3; the normalisation runs in learning
    phase 0 (quirk Q6: the moving statistics, never updated).  batch_norm=False: Dense + activation alone.  One op
    (ops.dense_bn), which picks the short-batch kernels of csrc/shortm.hip or dense -> graph_bn.
    forward(x, out=None, out_col=0): the result goes into columns out_col.. of the [B, wide] buffer `out` when given."""

    def __init__(self, units, batch_norm=True, activation=None, eps=1e-3):
        super().__init__()
        ops.act_code(activation)
        self.units, self.batch_norm, self.activation, self.eps = int(units), bool(batch_norm), activation, float(eps)
        self.kernel = self.bias = self.gamma = self.beta = None

    def build(self, din, device):
        if self.kernel is None:
            self.kernel = nn.Parameter(layers._init_tensor((din, self.units), "glorot_uniform", device))
            self.bias = nn.Parameter(torch.zeros(self.units, device=device))
            if self.batch_norm:
                self.gamma = nn.Parameter(torch.ones(self.units, device=device))
                self.beta = nn.Parameter(torch.zeros(self.units, device=device))
                self.register_buffer("moving_mean", torch.zeros(self.units, device=device))
                self.register_buffer("moving_variance", torch.ones(self.units, device=device))

    def forward(self, x, out=None, out_col=0):
        self.build(x.shape[1], x.device)
        if not self.batch_norm:
            return ops.dense_bn(x, self.kernel, self.bias, activation=self.activation, out=out, out_col=out_col)
        return ops.dense_bn(x, self.kernel, self.bias, self.gamma, self.beta, self.moving_mean, self.moving_variance, self.eps,
                            self.activation, out=out, out_col=out_col)


class MultimodalVecGCN(nn.Module):
    """example_model/model_multimodal_vec.py:56-127 (compound graph + per-graph protein vector `profeat`), call by call:
      graph branch (:60-75)   GraphConv(50, C) sigmoid, GraphDense(50) sigmoid, GraphGather -> [B, 50]
      vector branch (:83-94)  Dense(300), BatchNormalization, relu; Dense(100), BN, relu; Dense(64), BN, relu -> [B, 64]
      shared part (:103-110)  concat([vector, graph]) -> Dense(52), BN, relu -> Dense(label_dim); loss masked_softmax_ce (:112-120)
    The concatenation is one [B, 114] buffer: the tower's last layer writes columns 0-63, the graph read-out 64-113
    (ops.join_columns), nothing is copied.  forward(features, adjs, vectors=None, enabled_node_nums=None) -> logits; `vectors`
    is the float32 [B, Dv] batch of data_util.vector_table (GraphedTrainStep passes it as a forward kwarg); enabled_node_nums is
    accepted and unused, as in the file.  vector_first [B, 300]: the already computed output of tower[0], in place of `vectors`
    (visualization.vecmodal_integrated_gradients differentiates to it).  The rows never mix (learning phase 0, no dropout)."""

    ROW_INDEPENDENT = True

    GRAPH_WIDTH, TOWER, HIDDEN = 50, (300, 100, 64), 52

    def __init__(self, adj_channel_num=1, label_dim=2):
        super().__init__()
        self.conv = layers.GraphConv(self.GRAPH_WIDTH, adj_channel_num, activation="sigmoid")     # :60-61
        self.dense = layers.GraphDense(self.GRAPH_WIDTH, activation="sigmoid")                    # :73-74
        self.tower = nn.ModuleList([KerasDenseBN(u, activation="relu") for u in self.TOWER])      # :84-94
        self.hidden = KerasDenseBN(self.HIDDEN, activation="relu")                                # :106-108
        self.out = KerasDenseBN(int(label_dim), batch_norm=False)                                 # :110

    def forward(self, features, adjs, vectors=None, enabled_node_nums=None, vector_first=None):
        if vector_first is not None:                  # the output of tower[0] [B, 300], already computed, in place of `vectors`
            vectors = vector_first
        if vectors is None:
            raise ValueError("MultimodalVecGCN needs the vectors= batch")
        adj = layers._pack(adjs, features)
        B, vw = features.shape[0], self.TOWER[-1]
        if vectors.shape[0] != B:
            raise ValueError("%d vectors for %d graphs" % (vectors.shape[0], B))
        joined = features.new_empty((B, vw + self.GRAPH_WIDTH))
        layer = self.tower[1](self.tower[0](vectors) if vector_first is None else vector_first)
        vec = self.tower[2](layer, out=joined, out_col=0)
        node = self.dense(self.conv(features, adj=adj))
        graph = ops.graph_gather_into(node, joined, vw)                                           # :75
        layer = ops.join_columns(joined, [vec, graph])                                            # :103 tf.concat
        return self.out(self.hidden(layer))

    @staticmethod
    def loss(logits, labels, mask):
        """model_multimodal_vec.py:114-120 -> (cost_opt, cost_sum)."""
        return masked_softmax_ce(logits, labels, mask)


class MultimodalRegressionGCN(nn.Module):
    """example_model/model_multimodal_regression.py:60-101 (graph + per-graph descriptor vector `dragon`, regression), call by call:
      graph branch (:63-81)   GraphDense(32), GraphBatchNormalization, relu (twice); GraphDense(32), GraphBatchNormalization;
                              GraphGather, tanh -> [B, 32].  The adjacency is not read (no GraphConv in the file).
      vector branch (:83-86)  Dense(8), BatchNormalization, relu -> [B, 8]
      head (:88-90)           concat([vector, graph]) -> Dense(label_dim): the predictions
    The node-level body runs through layers.fused_stack when eligible (one launch each way), else layer by layer;
    GraphBatchNormalization honours enabled_node_nums.  The concatenation is one [B, 40] buffer (vector 0-7, graph 8-39).
    forward(features, adjs, vectors=None, enabled_node_nums=None) -> predictions [B, label_dim]; loss: masked squared error.
    vector_first [B, 8]: the already computed output of `vec`, in place of `vectors` (copied into the joined buffer)."""

    ROW_INDEPENDENT = True

    WIDTH, VEC_WIDTH = 32, 8

    def __init__(self, label_dim=1):
        super().__init__()
        self.dense1 = layers.GraphDense(self.WIDTH)                                               # :63
        self.bn1 = GraphBatchNormalization(activation="relu")                                     # :64-67
        self.dense2 = layers.GraphDense(self.WIDTH)                                               # :69
        self.bn2 = GraphBatchNormalization(activation="relu")                                     # :70-73
        self.dense3 = layers.GraphDense(self.WIDTH)                                               # :75
        self.bn3 = GraphBatchNormalization()                                                      # :76-78
        self.gather = layers.GraphGather()                                                        # :80
        self.vec = KerasDenseBN(self.VEC_WIDTH, activation="relu")                                # :84-86
        self.out = KerasDenseBN(int(label_dim), batch_norm=False)                                 # :90

    def forward(self, features, adjs, vectors=None, enabled_node_nums=None, vector_first=None):
        if vector_first is not None:                  # the output of `vec` [B, 8], already computed, in place of `vectors`
            vectors = vector_first
        if vectors is None:
            raise ValueError("MultimodalRegressionGCN needs the vectors= batch")
        B, N = features.shape[0], features.shape[1]
        if vectors.shape[0] != B:
            raise ValueError("%d vectors for %d graphs" % (vectors.shape[0], B))
        joined = features.new_empty((B, self.VEC_WIDTH + self.WIDTH))
        vec = self.vec(vectors, out=joined, out_col=0) if vector_first is None else ops.activation_into(vector_first, None, joined, 0)
        body = [self.dense1, self.bn1, self.dense2, self.bn2, self.dense3, self.bn3]
        pooled = None if adjs is None else layers.fused_stack(body, features, layers._pack(adjs, features),
                                                              enabled_node_nums=enabled_node_nums, gather=True)
        if pooled is None:
            layer = features
            for dense, bn in zip(body[0::2], body[1::2]):
                layer = bn(dense(layer), max_node_num=N, enabled_node_nums=enabled_node_nums)
            pooled = self.gather(layer)
        graph = ops.activation_into(pooled, "tanh", joined, self.VEC_WIDTH)                       # :81 tf.nn.tanh
        layer = ops.join_columns(joined, [vec, graph])                                            # :88 tf.concat
        return self.out(layer)

    @staticmethod
    def loss(logits, labels, mask_label, accum=None):
        """model_multimodal_regression.py:94-101 -> (cost_opt, cost_sum); accum: ops.masked_squared_error's accumulator block."""
        cost_opt, cost_sum = ops.masked_squared_error(logits, labels, mask_label, accum=accum)[:2]
        return cost_opt, cost_sum
