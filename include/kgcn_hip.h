/*
 * kgcn_hip.h -- C ABI of libkgcn_hip.so: the MI355X (gfx950) implementation of kGCN's batched
 * graph-convolution hot path.
 *
 * What this replaces.  The reference loads three TensorFlow custom-op libraries from the
 * working directory -- tf.load_op_library('./bspmm.so') (kgcn/bspmm_call.py:9,19),
 * './bconv.so' (kgcn/bconv_call.py:9,26), './batched.so' (kgcn/batched_call.py:9,19,30) --
 * and calls their ops Bspmm / Bconv / Bspmdt from GraphConv.call and GINAggregate.call
 * (kgcn/layers.py:77,88,102,435,445,458).  Neither sources nor binaries of those libraries are
 * in the reference tree, so there is no ABI to copy: the entry points below are what a binding
 * for this path needs, one per op contract plus the dense contraction, the
 * fused layer and the tiny reductions that close a forward+backward.
 *
 * Conventions
 *  - plain C, no C++/torch types; every pointer marked "device" is a HIP device pointer owned
 *    by the CALLER.  The library never allocates or frees device memory and keeps no global
 *    mutable state besides a thread-local error string; scratch space is passed in and sized
 *    by the *_workspace_bytes queries.
 *  - a workspace of too few bytes is refused with "<entry>: workspace <have> < <need> bytes" before anything is launched.  The
 *    sort-and-rank entry points (graph / hash kernels, pair ranking, CV metrics, link prediction, SVM, label propagation, COO
 *    packing) round the pointer up themselves and take any address.  Every other entry point uses the pointer as given and
 *    accesses it as 4-byte words, except where its layout holds a wider word: kgcn_graph_bn_stats_f32 / kgcn_graph_bn_bwd*_f32
 *    (a 64-bit count) and kgcn_ragged_plan (64-bit pairs) need an 8-byte aligned workspace and refuse another one with
 *    "<entry>: workspace not 8-byte aligned", nothing launched.  Pointers from a device allocator satisfy all of this.
 *  - every launch is asynchronous on the given stream (hipStream_t passed as void*); no
 *    implicit synchronisation.  Entry points are re-entrant.
 *  - return value: 0 = ok, non-zero = error; text via kgcn_last_error().  No exception crosses
 *    the ABI.
 *  - all tensors are IEEE fp32, indices int32; every contraction accumulates in fp32.  Three evaluation routes,
 *    chosen per call from the shapes (kgcn_dense_mfma_products(kind, m, din, dout) reports the route of a dense call:
 *    1, 6 or 3 matrix-pipe products per fp32 product):
 *      (1) v_mfma_f32_32x32x2_f32 -- fp32 operands, exact products (kgcn_dense_* up to 128 output columns, the narrow
 *          50-wide layers, the cross-layer stack kernels);
 *      (2) bf16 x 3 -- an EXACT three-way bf16 split of every fp32 operand (v = p1 + p2 + p3, 8+8+8 significand bits) and
 *          the six products a_i b_j with i + j <= 4; the neglected terms are below 2^-23 |a b|, one fp32 rounding of the
 *          product (the fused GraphConv kernels kgcn_graphconv_*; kgcn_dense_* with more than 128 output columns below
 *          16,384 rows, with 65..96 input columns, and the 256 -> 50 layers);
 *      (3) f16 x 2 -- the wide-layer GEMMs of kgcn_dense_fwd_* / kgcn_dense_dx_dact_* / kgcn_dense_wgrad_* /
 *          kgcn_dense_bwd_* at >= 16,384 rows: each operand is scaled by an exact power of two per ROW (x, gradients) or
 *          per COLUMN (weights; both operands of a weight gradient) so that its largest magnitude lands in [2^14, 2^15),
 *          split into two f16 pieces v' = h + l (22 significand bits) and multiplied as l*H + h*L + h*H.
 *          Error of one dot product of length K:  <= 2^-23 sum_k |x_k w_k|  +  K * 2^-40 * max_k|x_k| * max_k|w_k|
 *          (the second term: elements more than 2^14 below their row's / column's maximum keep fewer than 22 bits --
 *          f16 denormal spacing).  For data within 2^14 of the row / column maximum this is fp32 arithmetic with one
 *          rounding per product; the edge suite (exponent spread, denormals, heavy-tailed rows) is
 *          tests/test_gpu_dense_edges.py, measured errors in profiles/r05_accuracy.json.
 *    Routes (2) and (3) never see reduced-precision INPUTS: the splits are of the caller's fp32 values.
 *
 * Adjacency layout in HBM ("batched CSR", one per adjacency channel).  T graphs, each an
 * [rows x cols] sparse matrix (uniform, = the reference's max_node_num padding,
 * kgcn/data_util.py:30-37, 410).  Row r of graph t owns entries rowptr[t*rows+r] ..
 * rowptr[t*rows+r+1]-1 of `cv`; entry e is the pair cv[2e] = column index LOCAL to the graph
 * (int32 bit pattern), cv[2e+1] = value (fp32 bit pattern).  Entries of a row keep the order
 * they had in the reference's COO (tf.SparseTensor) input; duplicates are simply repeated
 * entries (they accumulate, as in TF); rows without entries produce zeros; graphs without
 * entries (the dummy graphs padding a short batch, kgcn/feed.py:123-126) are legal.
 */
#ifndef KGCN_HIP_H_
#define KGCN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): kgcn_csr_batch grew block_ptr / num_blocks / block_rows_max (round 4), kgcn_dense_dx_dact_gather_f32 gained
 * pooled_ld and kgcn_masked_sigmoid_ce_f32 gained pos_weight_per_task.  A binder built against version 1 must not call a
 * version-2 library: compare kgcn_abi_version() with the KGCN_HIP_ABI_VERSION it was compiled against AND
 * kgcn_csr_batch_size() with its own sizeof(kgcn_csr_batch) before the first call (kgcn_amd/_lib.py and
 * tests/abi_consumer.c do both).
 * Round 6 ADDED entry points only (no signature or layout changed, the version stays 2): kgcn_bconv_fanout_f32,
 * kgcn_copy2d_multi_f32 (+ kgcn_copy2d_job), kgcn_hbm_probe.
 * The graph VAE added entry points only as well (version still 2): kgcn_philox4x64_raw, kgcn_normal_f32,
 * kgcn_vae_sample_fwd_f32 / kgcn_vae_sample_bwd_f32, kgcn_vae_recon_workspace_bytes, kgcn_vae_recon_fwd_f32 /
 * kgcn_vae_recon_bwd_f32.
 * The multimodal sequence encoder added entry points only (version still 2): kgcn_seq_convpool_fwd_f32 /
 * kgcn_seq_convpool_bwd_f32 (+ kgcn_seq_convpool_workspace_bytes), kgcn_seq_lstm_fwd_f32 / kgcn_seq_lstm_bwd_f32
 * (+ kgcn_seq_lstm_stash_floats, kgcn_seq_lstm_workspace_bytes), kgcn_graph_gather_bwd_ld_f32.
 * Knowledge-graph link prediction added entry points only (version still 2): kgcn_linkpred_fwd_f32 / kgcn_linkpred_bwd_f32
 * (+ kgcn_linkpred_workspace_bytes).
 * Integrated gradients of the multimodal model added entry points only (version still 2): kgcn_seq_convpool_scaled_fwd_f32,
 * kgcn_seq_convpool_input_grad_f32.
 * The protein-sequence CNN added entry points only (version still 2): kgcn_conv1d_pool_fwd_f32 / kgcn_conv1d_pool_bwd_f32
 * (+ kgcn_conv1d_pool_workspace_bytes), kgcn_embedding_grad_f32.
 * Integrated gradients of the link-prediction model added an entry point only (version still 2): kgcn_kg_ig_f32.
 * The compact row-padded adjacency (row_pad == KGCN_ROW_PAD_COMPACT) added a layout CODE and entry points only (version
 * still 2): a library without it refuses that code in every entry point (validate_csr accepts row_pad 0 and 4 only), so
 * an old library never misreads it; kgcn_csr_compact4 is the feature query (look it up before building such a batch).
 * The SpMM route report added an entry point only (version still 2): kgcn_spmm_route_query (+ kgcn_spmm_route).
 * The pair ranking added entry points only (version still 2): kgcn_pair_rank_select_f32 / _emit_f32 / _table_i32 (+ _workspace_bytes).
 * The smooth attribution methods added entry points only (version still 2): kgcn_ig_perturb_rows_f32, kgcn_ig_perturb_values_f32,
 * kgcn_seq_convpool_perturbed_fwd_f32.
 * Cross-validation added entry points only (version still 2): kgcn_multitask_softmax2_ce_f32, kgcn_binary_metrics_f32
 * (+ kgcn_binary_metrics_workspace_bytes).
 * The vector-modality models and regression added entry points only (version still 2): kgcn_dense_bn_short_fwd_f32 / _bwd_f32 /
 * _dx_f32 (+ kgcn_dense_bn_short_supported), kgcn_act_cols_fwd_f32 / _bwd_f32, kgcn_masked_sqerr_f32, kgcn_regression_sums_f64.
 * Integrated gradients of the compound-protein interaction network added entry points only (version still 2): kgcn_cpi_ig_f32
 * (+ kgcn_cpi_ig_workspace_bytes).
 * Integrated gradients over the vector modality added entry points and a noise stream only (version still 2):
 * kgcn_ig_copies_expand_f32, kgcn_ig_copies_reduce_f32, KGCN_IG_STREAM_VECTOR.
 * The classical graph kernels added entry points only (version still 2): kgcn_wl_refine_i32, kgcn_wl_rank_i32
 * (+ kgcn_wl_rank_workspace_bytes), kgcn_wl_runs_i32, kgcn_sp_features_i32 (+ kgcn_graph_runs_workspace_bytes), kgcn_gram_plan_i64,
 * kgcn_gram_dense_f64 (+ kgcn_graph_gram_workspace_bytes), kgcn_gram_normalize_f64.
 * The hash graph kernels added entry points only (version still 2): kgcn_attr_scale_f64 (+ kgcn_attr_scale_workspace_bytes),
 * kgcn_lsh_buckets_f64, kgcn_rank_pairs_i64 (+ kgcn_rank_pairs_workspace_bytes), kgcn_wl_refine_copies_i32, kgcn_wl_rank_copies_i32
 * (+ kgcn_wl_rank_copies_workspace_bytes), kgcn_wl_runs_copies_i32, kgcn_sp_features_copies_i32
 * (+ kgcn_graph_runs_copies_workspace_bytes).
 * The batched kernel SVM added entry points only (version still 2): kgcn_svm_smo_f64 (+ kgcn_svm_workspace_bytes),
 * kgcn_svm_decision_f64, kgcn_svm_vote_i32.
 * Active learning added entry points only (version still 2): kgcn_rbf_affinity_f64, kgcn_lp_degrees_f64, kgcn_lp_propagate_f64
 * (+ kgcn_lp_workspace_bytes), kgcn_lp_finish_f64, kgcn_lp_scores_f64, kgcn_lp_select_f64; and, without a
 * stored affinity matrix, kgcn_rbf_apply_f64, kgcn_rbf_degrees_f64, kgcn_lp_propagate_free_f64.
 * Integrated gradients of the protein-sequence CNN added entry points only (version still 2): kgcn_ig_conv1d_expand_f32,
 * kgcn_ig_conv1d_reduce_f32. */
#define KGCN_HIP_ABI_VERSION 2

/* Column index of the padding entries of a row-padded batch (see row_pad): they carry value 0 and
 * gather an all-zero row the fused kernels keep in LDS, so they contribute exactly 0 (never 0*inf). */
#define KGCN_PAD_COL 32

/* row_pad code of the COMPACT row-padded layout (kgcn_csr_compact4): the structure of row_pad = 4 -- same rows, same
 * entries in the same order, padding to multiples of 4 with column KGCN_PAD_COL, same graph_ptr -- in fewer bytes:
 *   cv       [nnz / 4] uint32 column words: entry e's column is byte (e & 3) of word e >> 2 (one 4-entry group = one
 *            word), followed -- unless reserved_ & KGCN_CSR_UNIT_VALUES -- by the value stream: [nnz] fp32 bits starting
 *            at 32-bit word kgcn_compact_values_offset(nnz) of cv (16-byte aligned), 0.0 for padding entries
 *   slots    [T*M] uint16 (the pointer is cast): per graph its M rows by decreasing length (the order of row_pad = 4),
 *            slot = (first group of the row inside the graph, < 128) | (group count << 7, 1..15) | (row << 11)
 *   rowptr   [T*M + 1] and graph_ptr [T + 1] as in row_pad = 4 (in entries)
 * Only the FULL-shape fused kernels read it (kgcn_graphconv_fused_reads_compact); every other entry point refuses it. */
#define KGCN_ROW_PAD_COMPACT 0x104
/* reserved_ flag of a compact batch: every stored (non-padding) value is exactly 1.0f, no value stream is stored and the
 * kernels add the gathered rows instead of multiplying them (fma(1, x, a) == a + x bit for bit). */
#define KGCN_CSR_UNIT_VALUES 1

/* Non-finite inputs, per route (see "Conventions").  bf16 x 3 (fused GraphConv kernels, route 2): p1 + p2 + p3 == x bit for
 * bit for finite x; +-inf splits into (inf, NaN, NaN) and NaN into (NaN, NaN, NaN).  f16 x 2 (wide-layer GEMMs, route 3): a
 * row of x / a column of W (a column of either operand in a weight gradient) that holds +-inf or NaN gets a meaningless
 * scale and non-finite pieces, so EVERY output of that row / column is non-finite -- each of them depends on the non-finite
 * input.  In all routes: every output element that depends on a non-finite input comes out non-finite (NaN where fp32
 * arithmetic would give +-inf is possible), every other element is unaffected -- never a silently finite wrong value
 * (tests/test_gpu_parity.py::test_bf16_split_non_finite_inputs, tests/test_gpu_dense_edges.py).  Padding entries of the
 * row-padded layout gather an all-zero row with value 0, so they contribute exactly 0 (never 0 * inf). */

typedef struct kgcn_csr_batch {
  int32_t num_graphs;        /* T */
  int32_t rows;              /* M: rows per graph (padded, uniform) */
  int32_t cols;              /* K: columns per graph = rows of each rhs block */
  int32_t max_nnz_per_graph; /* max over graphs of stored entries (sizes the LDS staging) */
  int32_t row_pad;           /* 0: plain CSR.  4: every row holds a positive multiple of 4 entries,
                                padded with (col = KGCN_PAD_COL, value = 0) -- the layout the fused
                                GraphConv kernels read (mask-free 4-entry gathers); only those
                                kernels accept it */
  int32_t reserved_;         /* 0, or KGCN_CSR_UNIT_VALUES for a compact batch (row_pad == KGCN_ROW_PAD_COMPACT) */
  int64_t nnz;               /* total stored entries (including padding entries) */
  const int32_t* rowptr;     /* device, [T*M + 1], absolute offsets into cv (in entries) */
  const int32_t* cv;         /* device, [2*nnz], interleaved (local col, fp32 value bits) */
  /* row_pad == 4 only (NULL otherwise): */
  const int32_t* slots;      /* device, [T*M]: per graph its M rows ordered by DEcreasing entry count,
                                slot = (offset of the row's first entry inside the graph) |
                                (entry count << 16) | (row index << 24).  A 4-row aggregation pass
                                reads 4 consecutive slots, so rows longer than 4 entries share the
                                first pass(es) and the others never branch */
  const int32_t* graph_ptr;  /* device, [T + 1]: graph_ptr[t] = rowptr[t*M] */
  /* Block structure of a block-diagonal one-graph container (the ragged-compact batches, kgcn_ragged_compact_csr); NULL /
   * 0 everywhere else.  The rows are cut into num_blocks ROW BLOCKS of whole molecules: block k = rows
   * [block_ptr[k], block_ptr[k+1]) holds the molecules whose first row lies in [k*block_rows, (k+1)*block_rows) -- at
   * most block_rows_max = block_rows + n_nodes - 1 rows, and no adjacency entry leaves its block.  The aggregation
   * kernels stage a block's rhs rows in LDS once and gather there (spmm.hip, spmm_block_kernel); an entry that does
   * leave its block (a container built by hand) is gathered from memory instead, so the result never depends on it. */
  const int32_t* block_ptr;  /* device, [num_blocks + 1], non-decreasing, block_ptr[num_blocks] = rows */
  int32_t num_blocks;
  int32_t block_rows_max;
} kgcn_csr_batch;

/* -- library info ------------------------------------------------------------------------ */
int kgcn_abi_version(void);
/* sizeof(kgcn_csr_batch) as THIS library was compiled: a caller whose own sizeof differs was built against another layout
 * of the descriptor (it grew in ABI version 2) and must not pass it in. */
int64_t kgcn_csr_batch_size(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* kgcn_last_error(void);
/* Name of the code-object architecture the kernels were built for ("gfx950"). */
const char* kgcn_build_arch(void);

/* -- Bspmm: batched sparse x dense ------------------------------------------------------- */
/* Replaces op `Bspmm` (kgcn/bspmm_call.py:16; backward use :45, kgcn/bconv_call.py:58,
 * kgcn/batched_call.py:60) and, because rhs/out are addressed as one strided tensor, also
 * `Bspmdt` (kgcn/batched_call.py:27: rhs is ONE [T*K, D] tensor -> rhs_graph_stride = K*rhs_ld).
 *   out[t] = beta * out[t] + A[t] @ rhs[t],   t = 0..T-1
 * rhs[t] = rhs + t*rhs_graph_stride is [K x d] with leading dimension rhs_ld (floats);
 * out[t] likewise [M x d].  beta is 0 (overwrite) or 1 (accumulate, used for the channel
 * add-n).  adjoint_a of the op is served by passing the batched CSR of A^T (the host packer
 * builds it once per batch); adjoint_b is a host-side transpose of rhs. */
int kgcn_bspmm_f32(const kgcn_csr_batch* a, const float* rhs, int64_t rhs_ld,
                   int64_t rhs_graph_stride, int32_t d, float* out, int64_t out_ld,
                   int64_t out_graph_stride, float beta, void* stream);

/* -- Bconv: fused multi-channel SpMM + channel add-n -------------------------------------- */
/* Replaces op `Bconv` (kgcn/bconv_call.py:18-23):  out[t] = sum_c A_c[t] @ rhs_c[t].
 * a_ch is a HOST array of num_channels descriptors; channel c's dense operand is
 * rhs + c*rhs_channel_stride (so the channels may be column slices of one [T*K, C*d] GEMM
 * output: rhs_channel_stride = d, rhs_ld = C*d). */
int kgcn_bconv_f32(const kgcn_csr_batch* a_ch, int32_t num_channels, const float* rhs,
                   int64_t rhs_ld, int64_t rhs_graph_stride, int64_t rhs_channel_stride,
                   int32_t d, float* out, int64_t out_ld, int64_t out_graph_stride,
                   void* stream);

/* -- gradient w.r.t. the sparse values ---------------------------------------------------- */
/* kgcn/bspmm_call.py:50-55:  dval[e] = sum_k grad[t][row_e,k] * rhs[t][col_e,k]  for every
 * stored entry e (same order as `cv`).  dval: device [nnz]. */
int kgcn_spmm_values_grad_f32(const kgcn_csr_batch* a, const float* grad, int64_t grad_ld,
                              int64_t grad_graph_stride, const float* rhs, int64_t rhs_ld,
                              int64_t rhs_graph_stride, int32_t d, float* dval, void* stream);

/* -- dense contraction (GraphDense, and the X.W part of the unfused GraphConv) ------------- */
/* kgcn/layers.py:255-262 (Keras Dense on reshape(X,[-1,Din])) and :99-100 / :112:
 *   y[m, dout] = x[m, din] @ w + bias        (trans_w = 0: w is [din x dout], ld w_ld)
 *   y[m, dout] = x[m, din] @ w^T + bias      (trans_w = 1: w is [dout x din], ld w_ld)
 * bias may be NULL.  fp32 MFMA. */
int kgcn_dense_fwd_f32(const float* x, int64_t m, int32_t din, int64_t x_ld, const float* w,
                       int64_t w_ld, int32_t trans_w, const float* bias, float* y,
                       int32_t dout, int64_t y_ld, void* stream);

/* Weight/bias gradients of the contraction:  dw[din,dout] = x^T @ dy,  dbias[dout] = colsum(dy)
 * (the reduction over all m = B*N rows: TF MatMul/BiasAdd gradients summed by AddN over the
 * graphs).  Deterministic two-stage reduction through `workspace`.
 * dw (ld = dout) and dbias may each be NULL. */
int64_t kgcn_dense_wgrad_workspace_bytes(int64_t m, int32_t din, int32_t dout);
int kgcn_dense_wgrad_f32(const float* x, int64_t x_ld, const float* dy, int64_t dy_ld, int64_t m,
                         int32_t din, int32_t dout, float* dw, float* dbias, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* -- fused GraphConv layer (single adjacency channel) -------------------------------------- */
/* kgcn/layers.py:64-116, all four branches compute
 *   out[t] = A[t] @ (x[t] @ w + bias)            x[t]: [N x din], out[t]: [N x dout]
 * Forward in ONE kernel (x tile -> LDS, fp32 MFMA, aggregation out of LDS; X.W never touches
 * HBM).  Supported fused shapes are reported by kgcn_graphconv_fused_supported(); other
 * shapes and multi-channel layers use kgcn_dense_* + kgcn_bconv_f32. */
/* a / at of the fused entry points must be row-padded batches (row_pad == 4), or compact ones (KGCN_ROW_PAD_COMPACT)
 * where kgcn_graphconv_fused_reads_compact says the selected kernel reads them; any other combination is refused. */
int kgcn_graphconv_fused_supported(int32_t n_nodes, int32_t din, int32_t dout,
                                   int32_t max_nnz_per_graph);
int kgcn_graphconv_fwd_f32(const kgcn_csr_batch* a, const float* x, const float* w,
                           const float* bias, int32_t din, int32_t dout, float* out,
                           void* stream);
/* Backward in ONE kernel + a small deterministic reduction:
 *   dfw[t] = A[t]^T @ dout[t];  dx[t] = dfw[t] @ w^T;  dw = sum_t x[t]^T dfw[t];
 *   dbias = sum_t colsum(dfw[t])          (SURVEY 3.3 / kgcn/bspmm_call.py:45)
 * at = batched CSR of A^T.  dx may be NULL (first layer). */
int64_t kgcn_graphconv_bwd_workspace_bytes(int32_t num_graphs, int32_t din, int32_t dout);
int kgcn_graphconv_bwd_f32(const kgcn_csr_batch* at, const float* x, const float* w,
                           const float* dout_grad, int32_t din, int32_t dout, float* dx,
                           float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* -- GINAggregate -------------------------------------------------------------------------- */
/* kgcn/layers.py:461-472:  out[t] = sum_c (eps[c] * x[t] + A_c[t] @ x[t]).
 * eps: device [num_channels] or NULL (the accelerated branches :429-460 drop the eps term). */
int kgcn_gin_aggregate_f32(const kgcn_csr_batch* a_ch, int32_t num_channels, const float* x,
                           int32_t d, const float* eps, float* out, void* stream);

/* -- mini-batch assembly on the device ---------------------------------------------------------- */
/* kgcn/feed.py:112-126 without the host: `src` is the container of the WHOLE dataset (resident in HBM),
 * sel[t] (device, int32[num_sel]) the dataset index of batch graph t or -1 for an empty dummy graph.
 * Writes the batch container: dst_rowptr[num_sel*rows + 1], dst_cv[2 * total entries] (capacity in
 * ENTRIES; exact total or worst case num_sel * max_nnz_per_graph), dst_graph_ptr[num_sel + 1]
 * (graph_ptr[num_sel] = total entries) and, for a row-padded source, dst_slots[num_sel*rows] (dummy
 * graphs become rows of 4 padding entries).  sel values must be < src->num_graphs (not checked: device
 * data).  workspace >= kgcn_csr_gather_workspace_bytes(num_sel). */
int64_t kgcn_csr_gather_workspace_bytes(int32_t num_sel);
int kgcn_csr_gather_graphs(const kgcn_csr_batch* src, const int32_t* sel, int32_t num_sel,
                           int32_t* dst_rowptr, int32_t* dst_cv, int64_t dst_cv_capacity,
                           int32_t* dst_slots, int32_t* dst_graph_ptr, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* The whole mini-batch in TWO launches: up to KGCN_ASSEMBLE_MAX_CSR containers of the same dataset (A, A^T, their row-padded
 * copies: each as in kgcn_csr_gather_graphs, dst_graph_ptr[num_sel + 1] included) and up to KGCN_ASSEMBLE_MAX_TABLES per-graph
 * float tables (features [G, N * F], labels, masks ... -- what kgcn/feed.py:112-133 slices per batch on the host):
 * table_out[k][t, :] = table[k][sel[t], :], a row of zeros for sel[t] = -1.  dst_cv_capacity must cover the worst case
 * num_sel * max(max_nnz_per_graph, 4 * rows of a row-padded source): the selection is device data.
 * workspace >= kgcn_batch_assemble_workspace_bytes(num_sel). */
#define KGCN_ASSEMBLE_MAX_CSR 4
#define KGCN_ASSEMBLE_MAX_TABLES 6
typedef struct kgcn_assemble_plan {
  int32_t num_csr, num_tables;
  const kgcn_csr_batch* src[KGCN_ASSEMBLE_MAX_CSR];
  int32_t* dst_rowptr[KGCN_ASSEMBLE_MAX_CSR];
  int32_t* dst_cv[KGCN_ASSEMBLE_MAX_CSR];
  int64_t dst_cv_capacity[KGCN_ASSEMBLE_MAX_CSR];
  int32_t* dst_slots[KGCN_ASSEMBLE_MAX_CSR];
  int32_t* dst_graph_ptr[KGCN_ASSEMBLE_MAX_CSR];
  const float* table[KGCN_ASSEMBLE_MAX_TABLES];
  float* table_out[KGCN_ASSEMBLE_MAX_TABLES];
  int64_t row_floats[KGCN_ASSEMBLE_MAX_TABLES];
} kgcn_assemble_plan;
int64_t kgcn_batch_assemble_workspace_bytes(int32_t num_sel);
int kgcn_batch_assemble(const kgcn_assemble_plan* plan, const int32_t* sel, int32_t num_sel, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* -- GraphMaxPooling ------------------------------------------------------------------------ */
/* kgcn/layers.py:122-150 (one adjacency channel per call; beta = 1 accumulates the channel add-n):
 *   out[t,i,k] = beta*out[t,i,k] + max_j dense(A[t] .* x[t][:,k])[i,j]
 * = the maximum of a_ij * x[t][j,k] over the stored entries of row i, with 0 as a candidate unless
 * the row stores all `cols` entries (absent entries of the densified row are zeros).  Entries of a row must
 * be unique (the reference densifies with tf.sparse_tensor_to_dense, which rejects repeated indices). */
int kgcn_graph_maxpool_fwd_f32(const kgcn_csr_batch* a, const float* x, int32_t d, float* out,
                               float beta, void* stream);
/* Gradient as TF builds it (reduce_max splits the gradient equally among ALL maximal elements of
 * the densified row, implicit zeros included):  dx[t,j,k] = beta*dx + sum_i a_ij * share(i,j,k).
 * at = batched CSR of A^T (same value per entry); workspace >= kgcn_graph_maxpool_bwd_workspace_bytes. */
int64_t kgcn_graph_maxpool_bwd_workspace_bytes(int32_t num_graphs, int32_t rows, int32_t d);
int kgcn_graph_maxpool_bwd_f32(const kgcn_csr_batch* a, const kgcn_csr_batch* at, const float* x,
                               const float* dout_grad, int32_t d, float* dx, float beta,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* -- GAT ------------------------------------------------------------------------------------ */
/* kgcn/layers.py:477-542, one adjacency channel per call (beta = 1 accumulates the channel add-n).  Only
 * the PATTERN of `a` is used (the reference ignores the values, :517-520).  weight_a: device [2*d]
 * (the layer's `weight_a{i}` [2d,1]).  With t_e = x[col_e].wa[0:d] + x[row_e].wa[d:2d], E_e = exp(leaky_relu(
 * t_e, 0.2)), denom[i] = sum over row i of E, alpha_e = E_e / (denom[col_e] + 1e-10) (column-indexed, as the
 * reference gathers it):   out[t,i,:] = beta*out + sigmoid(sum_{e in row i} alpha_e x[t, col_e, :]). */
int64_t kgcn_gat_workspace_bytes(int32_t num_graphs, int32_t n_nodes, int32_t d);
int kgcn_gat_fwd_f32(const kgcn_csr_batch* a, const float* x, int32_t d, const float* weight_a, float* out,
                     float beta, void* workspace, int64_t workspace_bytes, void* stream);
/* dx = beta*dx + d loss / d x,  dweight_a [2*d] overwritten (deterministic two-stage reduction).
 * at = batched CSR of the transposed pattern. */
int kgcn_gat_bwd_f32(const kgcn_csr_batch* a, const kgcn_csr_batch* at, const float* x, int32_t d,
                     const float* weight_a, const float* dout_grad, float* dx, float beta, float* dweight_a,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* -- decoders: per-graph weighted Gram matrix ------------------------------------------------ */
/* GraphDecoderInnerProd (kgcn/layers.py:268-282, w = NULL), GraphDecoderDistMult (:285-305), DistMult.call
 * (:347-354, one relation channel per call):  out[t,i,j] = sum_k w[k] x[t,i,k] x[t,j,k].
 * x [T, N, d], w [d] or NULL, out [T, N, N].  Backward: dx = beta*dx + w * ((g + g^T) x); dw [d] overwritten
 * (NULL to skip; workspace >= kgcn_gram_workspace_bytes(d), deterministic two-stage sum). */
int64_t kgcn_gram_workspace_bytes(int32_t d);
int kgcn_gram_fwd_f32(const float* x, int32_t num_graphs, int32_t n_nodes, int32_t d, const float* w, float* out,
                      void* stream);
int kgcn_gram_bwd_f32(const float* x, int32_t num_graphs, int32_t n_nodes, int32_t d, const float* w,
                      const float* dout_grad, float* dx, float beta, float* dw, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* -- GraphGather ---------------------------------------------------------------------------- */
/* kgcn/layers.py:163-164: out[b, :] = sum_n x[b, n, :] (padding rows included). */
int kgcn_graph_gather_fwd_f32(const float* x, int64_t batch, int32_t n_nodes, int32_t d,
                              float* out, void* stream);
/* the same into a column block of a wider tensor: out[b * out_ld + c] (tf.concat of several read-outs, model_gin.py:61, without
 * the concatenation pass) */
int kgcn_graph_gather_fwd_ld_f32(const float* x, int64_t batch, int32_t n_nodes, int32_t d, float* out, int64_t out_ld,
                                 void* stream);
/* dx[b, n, :] = dout[b, :] */
int kgcn_graph_gather_bwd_f32(const float* dout_grad, int64_t batch, int32_t n_nodes, int32_t d,
                              float* dx, void* stream);

/* dx[b, n, :] = dx_in[b, n, :] + dout[b, :] -- the gradient of a tensor that feeds a GraphGather read-out AND the next layer
 * (example_model/model_gin.py:45-60) in one pass; d % 4 == 0, 16-byte aligned tensors; dx may alias dx_in. */
int kgcn_graph_gather_bwd_add_f32(const float* dout_grad, const float* dx_in, int64_t batch, int32_t n_nodes, int32_t d,
                                  float* dx, void* stream);

/* -- small reductions used by the layer gradients ------------------------------------------- */
/* out[0] = sum_i a[i]*b[i]  (d eps of GINAggregate).  workspace >= kgcn_dot_workspace_bytes(). */
int64_t kgcn_dot_workspace_bytes(int64_t n);
int kgcn_dot_f32(const float* a, const float* b, int64_t n, float* out, void* workspace,
                 int64_t workspace_bytes, void* stream);

/* -- activations fused into the producing kernels -------------------------------------------- */
/* The reference's models wrap the layers in tf.sigmoid / tf.nn.relu / tf.tanh (example_model/model.py:43-53,
 * model_multitask.py:52-60, sparse.py:76, model_gin.py:47-50): one elementwise TF op -- one read and one write of the
 * activation tensor -- per layer and direction.  Here the activation rides in the epilogue of the kernel that produces
 * the tensor, and its derivative (expressed in the layer OUTPUT: sigmoid a(1-a), relu a > 0, tanh 1 - a^2) in the
 * prologue of the adjoint aggregation. */
#define KGCN_ACT_NONE 0
#define KGCN_ACT_SIGMOID 1
#define KGCN_ACT_RELU 2
#define KGCN_ACT_TANH 3
/* kgcn_bconv_f32 followed by act:  out[t] = act( sum_c A_c[t] @ rhs_c[t] ) */
int kgcn_bconv_act_f32(const kgcn_csr_batch* a_ch, int32_t num_channels, const float* rhs, int64_t rhs_ld,
                       int64_t rhs_graph_stride, int64_t rhs_channel_stride, int32_t d, float* out, int64_t out_ld,
                       int64_t out_graph_stride, int32_t act, void* stream);

/* The adjoint of Bconv for ALL channels from one read of the gradient (kgcn/bconv_call.py:45-53: addn_grad fans the incoming
 * gradient out to every channel):   out_c[t] = A_c[t]^T (grad[t] (.) act'(act_out[t]))   for c = 0 .. num_channels - 1,
 * out_c = out + c * out_channel_stride.  at_ch: the TRANSPOSED containers (A_c^T) of one batch shape; act / act_out as in
 * kgcn_bspmm_dact_f32 (act = KGCN_ACT_NONE: act_out may be NULL).  Equivalent to num_channels calls of kgcn_bspmm_dact_f32 with
 * beta = 0 (bit for bit: the same sums in the same order). */
int kgcn_bconv_fanout_f32(const kgcn_csr_batch* at_ch, int32_t num_channels, const float* grad, const float* act_out, int64_t ld,
                          int64_t graph_stride, int32_t d, int32_t act, float* out, int64_t out_ld, int64_t out_graph_stride,
                          int64_t out_channel_stride, void* stream);
/* backward of that layer through one channel (pass the A^T container):
 *   out[t] = beta*out[t] + A[t] @ ( grad[t] (.) act'(act_out[t]) )      grad, act_out: same layout (ld, graph stride) */
int kgcn_bspmm_dact_f32(const kgcn_csr_batch* a, const float* grad, const float* act_out, int64_t ld,
                        int64_t graph_stride, int32_t d, int32_t act, float* out, int64_t out_ld,
                        int64_t out_graph_stride, float beta, void* stream);
/* kgcn_dense_fwd_f32 followed by act:  y = act(x @ w(^T) + bias) */
int kgcn_dense_fwd_act_f32(const float* x, int64_t m, int32_t din, int64_t x_ld, const float* w, int64_t w_ld,
                           int32_t trans_w, const float* bias, float* y, int32_t dout, int64_t y_ld, int32_t act,
                           void* stream);
/* The same contraction with a caller-provided workspace of kgcn_dense_fwd_workspace_bytes(din, dout) bytes (0 for
 * layers that do not use one): for wide layers (dout > 128, din >= 192: the 256-wide layers of example_model/
 * model_multitask.py:51-57 and sparse.py:30) the weight operand is split once per call into a bf16 fragment table in
 * that workspace (csrc/wtable.hip) which the GEMM reads instead of splitting W in every workgroup.
 * workspace == NULL: kgcn_dense_fwd_act_f32. */
int64_t kgcn_dense_fwd_workspace_bytes(int32_t din, int32_t dout);
int kgcn_dense_fwd_ws_f32(const float* x, int64_t m, int32_t din, int64_t x_ld, const float* w, int64_t w_ld,
                          int32_t trans_w, const float* bias, float* y, int32_t dout, int64_t y_ld, int32_t act,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* Fragment tables ahead of time: ONE launch splits every listed operand (a training step: W of each wide layer for the forward,
 * W^T for d input -- 7-9 separate 5 us launches otherwise); job = the operand of a contraction over k with n output columns,
 * i.e. w [k x n] (trans_w = 0) or [n x k] (trans_w = 1), table = kgcn_dense_fwd_workspace_bytes(k, n) bytes.  The *_tab entry
 * points take such a READY table (valid as long as w is unchanged) instead of a workspace; table == NULL: no table. */
#define KGCN_WTABLE_MAX_JOBS 16
typedef struct kgcn_wtable_job {
  const float* w;
  int64_t w_ld;
  int32_t trans_w, k, n;
  int32_t k_w;               /* stacked operand (extra_row != NULL, trans_w = 0): rows 0 .. k_w - 1 come from w */
  void* table;
  const float* extra_row;    /* NULL: plain operand.  Else the operand is [w (k_w rows); extra_row (1 row, n floats); zeros] of k rows:
                                [W; bias; 0] of an aggregate-first GraphConv -- A (X W + 1 b) = (A [X | 1]) [W; b], kgcn/layers.py:112-113 --
                                split without a concatenation pass (ABI version 2) */
} kgcn_wtable_job;
int kgcn_wtable_split_multi(const kgcn_wtable_job* jobs, int32_t num_jobs, void* stream);
int kgcn_dense_fwd_tab_f32(const float* x, int64_t m, int32_t din, int64_t x_ld, const float* w, int64_t w_ld,
                           int32_t trans_w, const float* bias, float* y, int32_t dout, int64_t y_ld, int32_t act,
                           const void* table, int64_t table_bytes, void* stream);
/* Backward of y = act(x @ w + bias) with respect to x (w: [din x dout], ld w_ld):
 *   dpre = grad (.) act'(act_out)   written to dpre (same layout as grad; must not alias it) -- the operand of
 *                                   kgcn_dense_wgrad_f32 for dw / dbias,
 *   dx   = dpre @ w^T               [m x din].
 * For wide layers with a workspace of kgcn_dense_fwd_workspace_bytes(dout, din) bytes both happen in ONE pass of the
 * GEMM (the derivative is applied while the gradient rows are staged); otherwise two launches. */
int kgcn_dense_dx_dact_f32(const float* grad, const float* act_out, int64_t m, int32_t dout, int64_t ld, const float* w,
                           int64_t w_ld, int32_t din, float* dx, int64_t dx_ld, int32_t act, float* dpre,
                           void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_dense_dx_dact_tab_f32(const float* grad, const float* act_out, int64_t m, int32_t dout, int64_t ld, const float* w,
                               int64_t w_ld, int32_t din, float* dx, int64_t dx_ld, int32_t act, float* dpre, const void* table,
                               int64_t table_bytes, void* stream);
/* The same for a layer whose output was read out by GraphGather (kgcn/layers.py:163-164) and possibly handed on as well
 * (example_model/model_gin.py:45-60): the incoming gradient of node row r is  grad[r] + pooled_grad[r / n_nodes]  (grad == NULL: the
 * read-out alone).  The broadcast of d pooled over the node rows is formed while the GEMM stages its rows -- it never exists in
 * HBM (a [rows x dout] tensor written by kgcn_graph_gather_bwd(_add)_f32 and read back otherwise).  Wide layers only:
 * kgcn_dense_dx_dact_gather_supported(m, din, dout); table: kgcn_dense_fwd_workspace_bytes(dout, din) bytes, already split
 * (table_ready != 0, kgcn_wtable_split_multi) or a workspace the call splits into. */
int kgcn_dense_dx_dact_gather_supported(int64_t m, int32_t din, int32_t dout);
/* pooled_ld: row stride of pooled_grad [graphs, dout] in floats (a multiple of 4, >= dout: the gradient of a column block of a
 * wider read-out tensor -- model_gin.py:61 concatenates the read-outs of its blocks -- is used where it lies) */
int kgcn_dense_dx_dact_gather_f32(const float* grad, const float* pooled_grad, int64_t pooled_ld, int32_t n_nodes,
                                  const float* act_out, int64_t m, int32_t dout, int64_t ld, const float* w, int64_t w_ld,
                                  int32_t din, float* dx, int64_t dx_ld, int32_t act, float* dpre, void* table,
                                  int64_t table_bytes, int32_t table_ready, void* stream);
/* ONE-PASS backward of a wide dense layer (round 5, gemmb.hip): the whole backward of y = act(x @ w + bias) -- Keras Dense inside
 * GraphDense (kgcn/layers.py:248,260) and the X.W part of GraphConv (:99-100, :112) at the widths of example_model/model_gin.py:45-54
 * and example_model/model_multitask.py:51-57 -- from ONE sweep over (grad, act_out, x):
 *   dpre = (grad [+ pooled_grad[row / n_nodes]]) (.) act'(act_out)      (act == KGCN_ACT_NONE: dpre = grad, act_out may be NULL)
 *   dx = dpre @ w^T      dw = x^T @ dpre      dbias = colsum(dpre)      (dbias may be NULL)
 * The d pre-activation tensor is never written (kgcn_dense_dx_dact_f32 + kgcn_dense_wgrad_f32 write it and read it back: six
 * passes over [m, 256] tensors instead of four).  grad may be NULL when pooled_grad is given (the layer output was only read out
 * by GraphGather); pooled_grad as in kgcn_dense_dx_dact_gather_f32, with n_nodes >= 8 (smaller graphs: the two-call route).
 * ld: row stride of grad and act_out.
 * kgcn_dense_bwd_supported(m, din, dout): dout == 256, 128 < din <= 256 (a multiple of 4), m >= 16,384.  table / table_ready: the
 * fragment tables of w^T as for kgcn_dense_dx_dact_gather_f32 (kgcn_dense_fwd_workspace_bytes(dout, din) bytes); workspace >=
 * kgcn_dense_wgrad_workspace_bytes(m, din, dout) (128 partials, fixed-order second stage, deferrable: kgcn_reduce_defer).
 * Arithmetic: route 3 of "Conventions" (f16 x 2) with a row scale on dpre and a counter-scaled, per-column online scale on x. */
int kgcn_dense_bwd_supported(int64_t m, int32_t din, int32_t dout);
int kgcn_dense_bwd_f32(const float* grad, const float* pooled_grad, int64_t pooled_ld, int32_t n_nodes, const float* act_out,
                       int32_t act, int64_t ld, const float* x, int64_t x_ld, int64_t m, int32_t din, int32_t dout,
                       const float* w, int64_t w_ld, float* dx, int64_t dx_ld, float* dw, float* dbias, void* table,
                       int64_t table_bytes, int32_t table_ready, void* workspace, int64_t workspace_bytes, void* stream);
/* ... and its form for a layer whose d-input product is only needed for an inner product (kgcn_dense_dx_dact_dot_f32's case: the
 * activated wide GraphDense behind a GINAggregate whose input needs no gradient, example_model/model_gin.py:45-50):
 *   dot_out[0] = < dpre @ w^T , dotx >     dw = x^T @ dpre     dbias = colsum(dpre)        dpre = grad (.) act'(act_out)
 * from one sweep over (grad, act_out, x, dotx); nothing of size [m, .] is written.  Shapes, table and workspace as for
 * kgcn_dense_bwd_f32. */
int kgcn_dense_bwd_dot_f32(const float* grad, const float* act_out, int32_t act, int64_t ld, const float* x, int64_t x_ld, int64_t m,
                           int32_t din, int32_t dout, const float* w, int64_t w_ld, const float* dotx, int64_t dotx_ld, float* dw,
                           float* dbias, float* dot_out, void* table, int64_t table_bytes, int32_t table_ready, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* The same dX contraction where the product is only needed for an inner product (d epsilon of a GINAggregate, kgcn/layers.py:469
 * <d out, x>, in front of an activated wide layer whose input needs no gradient -- the first block of example_model/model_gin.py):
 *   dot_out[0] = < (grad (.) act'(act_out)) @ w^T , dotx >       dotx [m, din] (row stride dotx_ld, 16-byte aligned rows)
 * d pre-activation is written to dpre as in kgcn_dense_dx_dact_f32; the [m, din] product never exists in HBM.
 * kgcn_dense_dx_dact_dot_supported(m, din, dout); workspace >= kgcn_dense_dx_dact_dot_workspace_bytes(m, din) (one partial per
 * workgroup, fixed-order second stage); table as for kgcn_dense_dx_dact_gather_f32. */
int kgcn_dense_dx_dact_dot_supported(int64_t m, int32_t din, int32_t dout);
int64_t kgcn_dense_dx_dact_dot_workspace_bytes(int64_t m, int32_t din);
int kgcn_dense_dx_dact_dot_f32(const float* grad, const float* act_out, int64_t m, int32_t dout, int64_t ld, const float* w,
                               int64_t w_ld, int32_t din, const float* dotx, int64_t dotx_ld, int32_t act, float* dpre,
                               void* table, int64_t table_bytes, int32_t table_ready, float* dot_out, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* stand-alone forms: y = act(x) over n floats; dpre = grad (.) act'(act_out) (dpre may alias grad) */
int kgcn_act_fwd_f32(const float* x, int64_t n, int32_t act, float* y, void* stream);
int kgcn_act_bwd_f32(const float* act_out, const float* grad, int64_t n, int32_t act, float* dpre, void* stream);

/* -- GraphBatchNormalization (kgcn/layers.py:170-220) --------------------------------------- */
/* Keras BatchNormalization over the VALID node rows of a padded batch x [T, N, D]: rows n < enabled[t] of graph t
 * (enabled == NULL: every row; the reference gathers those rows, normalises the stacked [rows, D] matrix per feature and
 * pads the result back with zeros, :196-210 / :211-216).
 *   kgcn_graph_bn_stats_f32   mean[c], var[c] (population variance, two passes like tf.nn.moments) over the valid rows --
 *                             the batch statistics of training mode
 *   kgcn_graph_bn_apply_f32   y = gamma (x - mean) / sqrt(var + eps) + beta on valid rows, 0 on padding rows; with the
 *                             moving statistics this is inference mode (the TF1 default phase)
 *   kgcn_graph_bn_bwd_f32     dgamma = sum g xhat, dbeta = sum g, and dx (may be NULL):
 *                             training != 0: gamma rstd (g - dbeta/n - xhat dgamma/n);  training == 0: gamma rstd g
 * mean / var / gamma / beta / dgamma / dbeta: device [D].  workspace: kgcn_graph_bn_workspace_bytes(D) bytes; reductions
 * are deterministic (per-workgroup partials, fixed-order second stage). */
int64_t kgcn_graph_bn_workspace_bytes(int32_t d);
int kgcn_graph_bn_stats_f32(const float* x, int64_t graphs, int32_t n_nodes, int32_t d, const int32_t* enabled,
                            float* mean, float* var, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_graph_bn_apply_f32(const float* x, int64_t graphs, int32_t n_nodes, int32_t d, const int32_t* enabled,
                            const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                            float* y, void* stream);
int kgcn_graph_bn_bwd_f32(const float* x, const float* grad, int64_t graphs, int32_t n_nodes, int32_t d,
                          const int32_t* enabled, const float* mean, const float* var, const float* gamma, float eps,
                          int32_t training, float* dx, float* dgamma, float* dbeta, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* act(bn(x)) in one pass (the padding rows become act(0), as tf.sigmoid(bn(...)) makes them) and its backward: the incoming
 * gradient is multiplied by act'(act_out) while it is read (act_out = the output of kgcn_graph_bn_apply_act_f32). */
int kgcn_graph_bn_apply_act_f32(const float* x, int64_t graphs, int32_t n_nodes, int32_t d, const int32_t* enabled,
                                const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                                int32_t act, float* y, void* stream);
int kgcn_graph_bn_bwd_dact_f32(const float* x, const float* grad, const float* act_out, int32_t act, int64_t graphs,
                               int32_t n_nodes, int32_t d, const int32_t* enabled, const float* mean, const float* var,
                               const float* gamma, float eps, int32_t training, float* dx, float* dgamma, float* dbeta,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* -- COO -> batched CSR on the device (the feed side: kgcn/feed.py:112-126 assembles the same triples in Python) ------ */
/* (graph, row, col, val)[nnz]: device arrays in ANY order (val NULL = all ones) -> rowptr_out [T*R + 1], cv_out [nnz]
 * (int2: column, fp32 value bits) with R = rows and the entries of a row in feed order (stable sort: duplicates stay and
 * are summed in feed order, like the host packer), or, transposed != 0, the container of A^T: R = cols, entries of a
 * transposed row in ascending original row.  perm_out (may be NULL): [nnz] input position of every stored entry.
 * stats_out: device int32[2] = {max stored entries per graph, number of out-of-range triples (must be 0)}.
 * workspace >= kgcn_coo_pack_workspace_bytes(nnz, T, rows, cols). */
int64_t kgcn_coo_pack_workspace_bytes(int64_t nnz, int32_t num_graphs, int32_t rows, int32_t cols);
int kgcn_coo_pack_f32(const int32_t* graph, const int32_t* row, const int32_t* col, const float* val, int64_t nnz,
                      int32_t num_graphs, int32_t rows, int32_t cols, int32_t transposed, int32_t* rowptr_out,
                      void* cv_out, int32_t* perm_out, int32_t* stats_out, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* plain container (row_pad = 0, square, rows <= KGCN_PAD_COL) -> the row-padded layout of the fused GraphConv kernels:
 * rowptr4_out [T*M + 1], cv4_out [cv4_capacity entries; nnz + 4*T*M always suffices], slots_out [T*M],
 * graph_ptr_out [T + 1].  stats_out: device int32[3] = {max padded entries per graph, total padded entries,
 * number of violations (row longer than 252 entries, graph longer than 65535, capacity exceeded; must be 0)}.
 * workspace >= kgcn_csr_pad4_workspace_bytes(T, M). */
int64_t kgcn_csr_pad4_workspace_bytes(int32_t num_graphs, int32_t rows);
int kgcn_csr_pad4(const kgcn_csr_batch* a, int32_t* rowptr4_out, void* cv4_out, int64_t cv4_capacity,
                  int32_t* slots_out, int32_t* graph_ptr_out, int32_t* stats_out, void* workspace,
                  int64_t workspace_bytes, void* stream);
/* row-padded container (row_pad = 4) -> the compact layout (KGCN_ROW_PAD_COMPACT, see there) of the same batch:
 * cv_out [kgcn_compact_cv_words(nnz, with_values) uint32], slots_out [T*M] uint16 (rowptr / graph_ptr are shared with
 * the source).  with_values = 0 writes no value stream.  stats_out: device int32[2] = {stored entries whose value is not
 * exactly 1.0f (padding excluded; 0 means KGCN_CSR_UNIT_VALUES applies), number of rows the 16-bit slot cannot hold (a
 * graph of more than 127 groups or a row of more than 15; must be 0 to use the result)}. */
int64_t kgcn_compact_values_offset(int64_t nnz);
int64_t kgcn_compact_cv_words(int64_t nnz, int32_t with_values);
int kgcn_csr_compact4(const kgcn_csr_batch* a4, void* cv_out, int with_values, void* slots_out, int32_t* stats_out,
                      void* stream);
/* 1 if the fused GraphConv launcher, for these arguments, selects a kernel that reads the compact layout (the FULL
 * forward; the pairs backward with dx), else 0.  backward: 0 forward, 1 backward; max_nnz of the row-padded batch. */
int kgcn_graphconv_fused_reads_compact(int32_t backward, int32_t num_graphs, int32_t n_nodes, int32_t din, int32_t dout,
                                       int32_t max_nnz_per_graph, int32_t with_dx);
/* 1 if kgcn_graphconv_fwd_f32, for these arguments, runs the FULL forward as reader | aggregator wave pairs
 * (graphconv_fwd_full_kernel), 0 if one wave per graph (small batches, slices too large for the pairs' LDS, other shapes).
 * Both compute the same bits.  max_nnz of the row-padded batch. */
int kgcn_graphconv_fwd_pairs_route(int32_t num_graphs, int32_t n_nodes, int32_t din, int32_t dout, int32_t max_nnz_per_graph);

/* -- ragged-compact batches: the layer stack on the VALID node rows only ------------------------------------------------ */
/* The reference pads every graph to max_node_num rows (kgcn/data_util.py:30-37, feed.py:127-133); its ragged layers
 * gather the first enabled_node_nums[b] rows of every graph, compute on the stacked [sum n_b, D] matrix and pad back
 * (GraphDense kgcn/layers.py:243-254, GraphBatchNormalization :196-210).  These entry points build that stacked layout
 * ONCE per batch so that every layer runs on it:
 *   rows [graph_ptr[t], graph_ptr[t+1])  the n_t valid rows of batch graph t
 *   rows [R, capacity_rows)              padding representatives: zero features, no adjacency entries; they go through
 *                                        the layers like the padded rows of the reference's layout, so any one of them
 *                                        holds the value ALL padded rows of the padded formulation have (GraphConv -> 0,
 *                                        act(0), un-ragged GraphDense -> one constant row, ragged BN -> 0)
 *   adjacency                            one block-diagonal [capacity_rows x capacity_rows] CSR (num_graphs = 1),
 *                                        accepted by every kgcn_bspmm / kgcn_bconv entry point
 * capacity_rows >= R + 1 is chosen by the caller (a fixed capacity lets a captured hipGraph replay batches of varying R).
 *
 * kgcn_ragged_plan: n_t = clamp(sizes[g], 0, rows) and e_t = stored entries in rows [0, n_t) of graph g = sel[t]
 * (sel NULL: g = t; sel[t] < 0: an empty dummy graph); graph_ptr / entry_ptr [num_sel + 1] = their exclusive scans
 * (graph_ptr[num_sel] = R).  src: square batched CSR of the source graphs (the batch itself or the whole dataset).
 * workspace >= kgcn_ragged_workspace_bytes(num_sel). */
int64_t kgcn_ragged_workspace_bytes(int32_t num_sel);
int kgcn_ragged_plan(const kgcn_csr_batch* src, const int32_t* sizes, const int32_t* sel, int32_t num_sel,
                     int32_t* graph_ptr, int32_t* entry_ptr, void* workspace, int64_t workspace_bytes, void* stream);
/* dst_rowptr [capacity_rows + 1], dst_cv [dst_cv_capacity entries] <- the block-diagonal container of the selected graphs
 * (also for A^T: pass the transposed source container with the SAME plan).  status (may be NULL): device int32, += the
 * number of stored entries that do not fit the compact layout (rows or columns >= n_t, plan mismatch, capacity exceeded);
 * must read 0. */
int kgcn_ragged_compact_csr(const kgcn_csr_batch* src, const int32_t* sel, int32_t num_sel, const int32_t* graph_ptr,
                            const int32_t* entry_ptr, int32_t capacity_rows, int32_t* dst_rowptr, int32_t* dst_cv,
                            int64_t dst_cv_capacity, int32_t* status, void* stream);
/* The same for a channel's A and A^T (one plan, two destination containers) in ONE launch. */
int kgcn_ragged_compact_csr_pair(const kgcn_csr_batch* src, const kgcn_csr_batch* src_t, const int32_t* sel, int32_t num_sel,
                                 const int32_t* graph_ptr, const int32_t* entry_ptr, int32_t capacity_rows, int32_t* dst_rowptr,
                                 int32_t* dst_cv, int64_t dst_cv_capacity, int32_t* dst_t_rowptr, int32_t* dst_t_cv,
                                 int64_t dst_t_cv_capacity, int32_t* status, void* stream);
/* The row blocks of a ragged-compact batch (kgcn_csr_batch.block_ptr): block_ptr [kgcn_ragged_num_blocks(capacity_rows) + 1]
 * from the plan's graph_ptr [num_sel + 1]; blocks past the valid rows cover the padding rows in steps of
 * KGCN_RAGGED_BLOCK_ROWS.  Every block holds at most KGCN_RAGGED_BLOCK_ROWS + n_nodes - 1 rows. */
#define KGCN_RAGGED_BLOCK_ROWS 32
int32_t kgcn_ragged_block_rows(void);                 /* KGCN_RAGGED_BLOCK_ROWS of the library that was loaded */
int32_t kgcn_ragged_num_blocks(int32_t capacity_rows);
int kgcn_ragged_blocks(const int32_t* graph_ptr, int32_t num_sel, int32_t capacity_rows, int32_t* block_ptr, void* stream);
/* dst [capacity_rows, d] <- the valid rows of src [num_source_graphs, n_nodes, d] (feed.py:127-133 layout), zeros on the
 * rows >= R. */
int kgcn_ragged_compact_rows_f32(const float* src, const int32_t* sel, int32_t num_sel, int32_t n_nodes, int32_t d,
                                 const int32_t* graph_ptr, int32_t capacity_rows, float* dst, void* stream);
/* The same rows as [x | 1 | 0 ...]: dst [capacity_rows, dst_ld], dst_ld >= d + 1; column d of EVERY row <- 1, columns d + 1 .. <- 0
 * (= kgcn_ragged_compact_rows_f32 followed by kgcn_augment_ones_f32 in one pass: the operand of the aggregate-first GraphConv,
 * A (X W + 1 b) = (A [X | 1]) [W ; b], kgcn/layers.py:99-113).  n_nodes * dst_ld < 2^22. */
int kgcn_ragged_compact_rows_aug_f32(const float* src, const int32_t* sel, int32_t num_sel, int32_t n_nodes, int32_t d,
                                     const int32_t* graph_ptr, int32_t capacity_rows, float* dst, int32_t dst_ld, void* stream);
/* back to the padded layout: dst [num_graphs, n_nodes, d]; padded rows <- row fill_row of src (the padding representative)
 * or zeros (fill_row < 0). */
int kgcn_ragged_expand_rows_f32(const float* src, int32_t num_graphs, int32_t n_nodes, int32_t d,
                                const int32_t* graph_ptr, int32_t fill_row, float* dst, void* stream);
/* GraphGather (kgcn/layers.py:163-164, padding rows included: quirk Q4) on the compact layout:
 *   out[b, :] = sum_{r in graph b} x[r, :] + (n_nodes - n_b) * x[pad_row, :]
 * backward: dx[r] = dout[b(r)] on valid rows, dx[pad_row] = sum_b (n_nodes - n_b) dout[b] (deterministic two-stage sum;
 * workspace >= kgcn_ragged_gather_bwd_workspace_bytes(d)), 0 on the other rows >= R. */
int kgcn_ragged_gather_fwd_f32(const float* x, const int32_t* graph_ptr, int64_t batch, int32_t n_nodes, int32_t d,
                               int32_t pad_row, float* out, void* stream);
int64_t kgcn_ragged_gather_bwd_workspace_bytes(int32_t d);
int kgcn_ragged_gather_bwd_f32(const float* dout_grad, const int32_t* graph_ptr, int64_t batch, int32_t n_nodes, int32_t d,
                               int32_t pad_row, int32_t capacity_rows, float* dx, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* -- loss definitions and optimiser update of the model files ---------------------------------------------- */
/* example_model/model_multitask.py:66-79:  cost[b] = mask[b] * sum_t mask_label[b,t] * ce(logits[b,t], labels[b,t]) with
 * tf.nn.sigmoid_cross_entropy_with_logits (weighted == 0) or tf.nn.weighted_cross_entropy_with_logits(pos_weight):
 * pos_weight_per_task [tasks] (device; the reference's info.pos_weight is one weight per label column,
 * kgcn/data_util.py:563-568) or, when it is NULL, the scalar pos_weight for every task;
 * sums[0] = reduce_sum(cost) (cost_sum), sums[1] = reduce_mean(cost) over the PADDED batch (cost_opt, quirk Q5);
 * dlogits [batch, tasks] = d sums[0] / d logits.  mask_label may be NULL (all ones), cost [batch] may be NULL.
 * workspace >= kgcn_loss_workspace_bytes(batch); deterministic (block partials added in a fixed order). */
int64_t kgcn_loss_workspace_bytes(int64_t batch);
int kgcn_masked_sigmoid_ce_f32(const float* logits, const float* labels, const float* mask, const float* mask_label,
                               int64_t batch, int32_t tasks, int32_t weighted, float pos_weight,
                               const float* pos_weight_per_task, float* cost, float* dlogits, float* sums, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* example_model/model.py:56-61:  cost[b] = mask[b] * softmax_cross_entropy(labels[b], logits[b]); same outputs. */
int kgcn_masked_softmax_ce_f32(const float* logits, const float* labels, const float* mask, int64_t batch, int32_t classes,
                               float* cost, float* dlogits, float* sums, void* workspace, int64_t workspace_bytes,
                               void* stream);
/* example_model/sparse.py:112-113: tf.nn.sparse_softmax_cross_entropy_with_logits -- label_idx [batch] int64 class indices
 * instead of dense labels; mask may be NULL (all ones); outputs as above (sums[0] = the reduce_sum the model minimises). */
int kgcn_sparse_softmax_ce_f32(const float* logits, const int64_t* label_idx, const float* mask, int64_t batch,
                               int32_t classes, float* cost, float* dlogits, float* sums, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* Backward of those heads: out = dlogits * (g_sum + g_opt / batch), g_opt / g_sum = the upstream gradients of sums[1] (cost_opt)
 * and sums[0] (cost_sum) as DEVICE scalars, either may be NULL (no gradient through that output). */
int kgcn_loss_grad_f32(const float* dlogits, const float* g_opt, const float* g_sum, int64_t batch, int64_t n, float* out,
                       void* stream);
/* tf.train.AdamOptimizer(lr) (kgcn/core.py:124) over one flat buffer of n floats, with t = *step_counter + 1:
 *   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) (fp64);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *   params -= lr_t m / (sqrt(v) + eps)
 * then *step_counter += 1 (device int64: a captured hipGraph advances it on every replay). */
int kgcn_adam_tf_f32(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, int64_t* step_counter, void* stream);
/* The same update without a packed gradient buffer: segment q covers `numel` floats at `offset` of params / m / v and reads its
 * gradient from `grad` (the tensor the backward pass produced for that parameter); floats outside the segments are untouched.
 * More than KGCN_ADAM_MAX_SEGMENTS segments take several launches; ALL segments are checked before the first one, so a refused
 * list leaves params, m, v and the counter as they were. */
#define KGCN_ADAM_MAX_SEGMENTS 32
typedef struct kgcn_adam_segment {
  const float* grad;
  int64_t offset, numel;
} kgcn_adam_segment;
int kgcn_adam_tf_multi_f32(float* params, float* m, float* v, int64_t n, const kgcn_adam_segment* segments, int32_t num_segments,
                           float lr, float beta1, float beta2, float eps, int64_t* step_counter, void* stream);

/* -- aggregate-FIRST GraphConv: A (X W + 1 b) = (A [X | 1]) [W ; b] --------------------------------------------------- */
/* kgcn/layers.py:112-113 computes fw = X W + b and then A fw: a [rows, dout] aggregation.  When din + 1 < dout the other
 * association is cheaper (an aggregation of din + 1 columns, the same contraction, and in the backward no dout-wide adjoint
 * aggregation at all: dW', db = (A [X | 1])^T d pre-activation).  The bias term rowsum(A) (x) b -- NOT b: rows of A sum to
 * anything, empty rows to 0 -- is carried by a column of ones:
 *   out[r, 0:din] = x[r, 0:din], out[r, din] = 1, out[r, din+1 : out_ld] = 0          (out_ld >= din + 1)
 * backward: dx[r, 0:din] = dout[r, 0:din]. */
int kgcn_augment_ones_f32(const float* x, int64_t m, int32_t din, int64_t x_ld, float* out, int64_t out_ld, void* stream);
int kgcn_augment_ones_bwd_f32(const float* dout_grad, int64_t m, int32_t din, int64_t g_ld, float* dx, int64_t dx_ld,
                              void* stream);

/* -- cross-layer kernels for small graphs: the node-level body of example_model/model.py:42-54 in ONE launch ------------ */
/* For N <= 32 nodes per graph and layer widths <= 64 a graph's activations and all weights fit LDS: one forward and one
 * backward launch run   [GraphConv -> act] x k -> [BatchNormalization (moving statistics) -> act] -> [GraphDense -> act]
 * -> GraphGather   for every graph, instead of one launch and one HBM round trip per layer (at the reference's batch sizes
 * -- 30 graphs in example_config/synth.json -- a step is bound by launch latency).  Two routes with the same results up to
 * the summation order: one graph per workgroup trip on plain fp32 FMAs (a few hundred graphs: the latency of one graph), and
 * 64-row tiles of floor(64 / N) whole graphs on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate) for thousands.
 *   kind 0  H <- act(A (H W + b))   one adjacency channel (kgcn/layers.py:105-116);  w [din, dout], b [dout] or NULL
 *   kind 1  H <- act(H W + b)       GraphDense (:255-262)
 *   kind 2  H <- act(gamma (H - mean) / sqrt(var + eps) + beta) on rows < enabled[t], act(0) on the others
 *                                   GraphBatchNormalization with its moving statistics (:196-216); w = gamma, b = beta
 * layer_out: HOST array of num_layers device pointers, layer l's output [T, N, dout_l] (written by the forward, read by
 * the backward).  pooled (forward) non-NULL: GraphGather over all N rows (:163-164) -> [T, dout_last].
 * backward: dlast = d pooled [T, dout_last] (gather != 0) or d (last layer output) [T, N, dout_last]; dx [T, N, din_0] or
 * NULL; dparams: flat, per layer dW [din, dout] | db [dout] (kind 2: dgamma [d] | dbeta [d]), kgcn_gcn_stack_param_floats()
 * floats in total; deterministic (one partial per workgroup, fixed-order second stage);
 * workspace >= kgcn_gcn_stack_bwd_workspace_bytes(). */
#define KGCN_STACK_MAX_LAYERS 8
typedef struct kgcn_stack_layer {
  int32_t kind, act, din, dout;
  const float* w;
  const float* b;
  const float* mean; /* kind 2 only */
  const float* var;  /* kind 2 only */
  float eps;         /* kind 2 only */
  int32_t route;     /* read from layers[0] only: 0 automatic, 1 one graph per workgroup trip (plain fp32 FMAs), 2 64-row tiles of
                        whole graphs on the f32 MFMA (<= 4 weight matrices); the others: 0 */
} kgcn_stack_layer;
int kgcn_gcn_stack_supported(int32_t n_nodes, int32_t max_nnz_per_graph, const kgcn_stack_layer* layers, int32_t num_layers);
int64_t kgcn_gcn_stack_param_floats(const kgcn_stack_layer* layers, int32_t num_layers);
int kgcn_gcn_stack_fwd_f32(const kgcn_csr_batch* a, const float* x, const int32_t* enabled, const kgcn_stack_layer* layers,
                           int32_t num_layers, float* const* layer_out, float* pooled, void* stream);
int64_t kgcn_gcn_stack_bwd_workspace_bytes(int32_t num_graphs, const kgcn_stack_layer* layers, int32_t num_layers);
int kgcn_gcn_stack_bwd_f32(const kgcn_csr_batch* at, const float* x, const int32_t* enabled, const kgcn_stack_layer* layers,
                           int32_t num_layers, float* const* layer_out, const float* dlast, int32_t gather, float* dx,
                           float* dparams, void* workspace, int64_t workspace_bytes, void* stream);

/* Deferred second stages of PARAMETER gradients.  Every weight-gradient entry point (kgcn_dense_wgrad*_f32, kgcn_graphconv_bwd_f32)
 * ends by adding its per-workgroup partials in a fixed order -- a 5-7 us launch each, 7-9 per training step of the model files.
 * kgcn_reduce_defer(1) (PROCESS-wide -- frameworks run backward nodes on worker threads --; returns the previous setting) makes those calls QUEUE that second stage instead: dw /
 * dbias are then NOT valid, and the workspaces must stay untouched, until kgcn_reduce_flush(stream) has added all queued
 * partials in ONE launch (same order of additions: bit-identical results).  kgcn_reduce_pending(): queued second stages.
 * Deferring entry points: kgcn_dense_wgrad*_f32, kgcn_dense_bwd*_f32, kgcn_graphconv_bwd_f32 and -- with training == 0 only
 * (learning phase 0: d gamma / d beta are not read inside the call) -- kgcn_graph_bn_bwd_f32 / kgcn_graph_bn_bwd_dact_f32, whose
 * dgamma / dbeta buffers must likewise stay allocated until the flush.
 * The reference has no counterpart (TF sums gradients inside its executor, core.py:124); used by kgcn_amd.train. */
int kgcn_reduce_defer(int32_t on);
int kgcn_reduce_pending(void);
int kgcn_reduce_flush(void* stream);

/* Measurement aid (bench.py / tools/abi_roofline.py price a dense call against the pipe it really runs on): the number of
 * matrix-pipe products per fp32 product of the kernel the library routes this call to, operands assumed 16-byte aligned with
 * the W table present -- 3: f16 two-piece kernels (gemmh.hip, 2.5 PF / 3), 6: bf16 three-piece kernels (gemm3 / gemmn /
 * wgradn / wgradx, 2.5 PF / 6), 1: v_mfma_f32_32x32x2_f32 kernels (157.3 TF), 0: no matrix pipe (read-out layers).
 * kind 0: y = act(x W + b) / dx = dy W^T (din = contraction width), 1: dx with the activation derivative, 2: weight gradient. */
int kgcn_dense_mfma_products(int32_t kind, int64_t m, int32_t din, int32_t dout);

/* Which kernel a batched SpMM call takes (csrc/spmm.hip decides it in one host function, spmm_route; this reports its answer).
 * Host only: no launch, no device pointer followed (the descriptors' rowptr / cv may be anything; block_ptr only counts as
 * present or NULL), so it answers without a GPU.  a_ch: num_channels (1..8) descriptors of one launch; strides as the entry
 * point takes them -- channel_stride is the rhs channel stride of an aggregation (kgcn_bconv*_f32; 0 for single-channel calls)
 * and the out channel stride of a fan-out; align_bytes: the common alignment of the operand pointers, 16, 8 or 4. */
enum {
  KGCN_SPMM_NONE = 0,          /* nothing to launch (empty batch); fan-out: one single-channel launch per channel instead */
  KGCN_SPMM_TILE = 1,          /* spmm_tile_kernel<LPR, VEC, NW, false> */
  KGCN_SPMM_TILE_DOT = 2,      /* spmm_tile_kernel<LPR, 4, NW, true>: <grad, x> of GINAggregate's backward rides along */
  KGCN_SPMM_SLICES = 3,        /* spmm_slices_kernel<NS> */
  KGCN_SPMM_BLOCK = 4,         /* spmm_block_kernel<VEC, LPR, DACT> */
  KGCN_SPMM_ROWS = 5,          /* spmm_rows_kernel<VEC, LPR, DACT, ROWS> */
  KGCN_SPMM_GATHER = 6,        /* spmm_gather_kernel<VEC> */
  KGCN_SPMM_BCONV_LOOP = 7,    /* bconv_loop_kernel<VEC, NVL, NP> */
  KGCN_SPMM_BCONV_FANOUT = 8   /* bconv_fanout_kernel<VEC, NVL> */
};
/* flags of the call */
#define KGCN_SPMM_DACT 1         /* the operand is multiplied by act'(act_out) (kgcn_bspmm_dact_f32, fan-out with act != 0) */
#define KGCN_SPMM_SELF_SCALE 2   /* eps * x is added (kgcn_gin_aggregate_f32 and its backward with eps) */
#define KGCN_SPMM_DOT 4          /* first channel of kgcn_gin_aggregate_bwd_f32 with deps */
#define KGCN_SPMM_FANOUT 8       /* kgcn_bconv_fanout_f32 */
typedef struct kgcn_spmm_route {
  int32_t kernel;              /* KGCN_SPMM_* */
  int32_t template_args[4];    /* of the instantiation, in declaration order (bool as 0 / 1); unused entries 0 */
  int32_t ds, slices;          /* columns per workgroup and column slices (d = ds * slices) */
  int32_t workgroup;           /* threads per workgroup */
  int64_t grid;                /* workgroups */
  int64_t lds_bytes;           /* dynamic LDS of the launch */
} kgcn_spmm_route;
int kgcn_spmm_route_query(const kgcn_csr_batch* a_ch, int32_t num_channels, int32_t d, int64_t rhs_ld, int64_t rhs_graph_stride,
                          int64_t channel_stride, int64_t out_ld, int64_t out_graph_stride, int32_t align_bytes, int32_t flags,
                          kgcn_spmm_route* route);

/* Several strided 2-D fp32 copies in ONE launch: dst[r * dst_ld + c] = src[r * src_ld + c] for r < rows, c < cols of every job.
 * Used for the operand of a multi-channel GraphConv's single GEMM, [W_0 | W_1 | ...] and [b_0 | b_1 | ...] (kgcn/layers.py:68-78
 * builds one MatMul per channel; one GEMM over the concatenated kernels produces the same FW[b][ch] blocks side by side), and for
 * the split of that operand's gradient into one contiguous tensor per parameter.  Jobs without rows or columns are legal (their
 * pointers may be NULL); more than KGCN_COPY2D_MAX_JOBS jobs take several launches, and ALL jobs are checked (rows, cols >= 0,
 * both leading dimensions >= cols) before the first one: a refused list has copied nothing. */
#define KGCN_COPY2D_MAX_JOBS 16
typedef struct kgcn_copy2d_job {
  const float* src;
  float* dst;
  int64_t rows, cols, src_ld, dst_ld;
} kgcn_copy2d_job;
int kgcn_copy2d_multi_f32(const kgcn_copy2d_job* jobs, int32_t num_jobs, void* stream);

/* Measurement aid (bench.py: `roofline.hbm_probe`, SURVEY 8(d) "report both nominal and achievable"): one grid-stride float4
 * stream over `bytes` bytes per operand in the read : write mix of the kernel being priced, so that a bench line carries what
 * THIS box's HBM delivers right after the timed region.  mix 0: b = a (1 : 1, the batched SpMM's mix); 1: b = a + a2 (2 : 1, the
 * fused backward's mix); 2: read a only (b receives at most 16 bytes); 3: write b only.  No reference counterpart. */
int kgcn_hbm_probe(int32_t mix, const void* a, const void* a2, void* b, int64_t bytes, void* stream);

/* dW, dbias of act(x W + b) when the layer INPUT needs no gradient (first layer of a model): d pre-activation = dy * act'(act_out)
 * is formed while the weight-gradient GEMM stages the gradient rows, so it never exists in HBM.  Wide layers only
 * (kgcn_dense_wgrad_dact_supported(din, dout) != 0); otherwise run kgcn_act_bwd_f32 + kgcn_dense_wgrad_f32.  dy and act_out
 * share the leading dimension dy_ld; workspace as for kgcn_dense_wgrad_f32. */
int kgcn_dense_wgrad_dact_supported(int32_t din, int32_t dout);
int kgcn_dense_wgrad_dact_f32(const float* x, int64_t x_ld, const float* dy, const float* act_out, int64_t dy_ld, int32_t act,
                              int64_t m, int32_t din, int32_t dout, float* dw, float* dbias, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* Backward of GINAggregate (kgcn/layers.py:461-472) in one call: dx = sum_c (eps_c g + A_c^T g) -- at_ch = the TRANSPOSED
 * channel containers -- and d eps = <g, x> (one scalar: the same for every channel, :469), accumulated while the gradient
 * tiles are staged for the aggregation (no pass of its own over g and x); deterministic (one partial per graph, fixed-order
 * sum).  dx or deps may be NULL.  workspace >= kgcn_gin_aggregate_bwd_workspace_bytes(T, N, d). */
int64_t kgcn_gin_aggregate_bwd_workspace_bytes(int32_t num_graphs, int32_t n_nodes, int32_t d);
int kgcn_gin_aggregate_bwd_f32(const kgcn_csr_batch* at_ch, int32_t num_channels, const float* grad, int32_t d,
                               const float* eps, const float* x, float* dx, float* deps, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* -- graph VAE (example_model/model_vae.py) ------------------------------------------------------------------------------
 * Noise: Philox4x64-10 (the Random123 generator numpy ships as np.random.Philox) with key (seed, 0) and counter
 * (j, step, 0, 0) gives the four 64-bit words of block j; block j holds noise elements 4j .. 4j+3: words (0, 1) and (2, 3) each
 * give two N(0, 1) values by Box-Muller in f32 -- u1 = ((w0 >> 40) + 1) 2^-24, u2 = (w1 >> 40) 2^-24,
 * r = sqrt(-2 log u1), (r cos 2 pi u2, r sin 2 pi u2).  `step` is a DEVICE pointer (NULL = 0), read by the kernel: a replayed
 * hipGraph draws new noise when the value behind it changes. */
#define KGCN_VAE_MAX_NODES 128
#define KGCN_VAE_MAX_CHANNELS 8
#define KGCN_VAE_MAX_DIM 64
/* out[4j + q] = word q of block j, j < num_blocks (device, uint64) */
int kgcn_philox4x64_raw(uint64_t seed, const int64_t* step, int64_t num_blocks, uint64_t* out, void* stream);
/* out[e] = noise element e, e < n */
int kgcn_normal_f32(uint64_t seed, const int64_t* step, int64_t n, float* out, void* stream);
/* Reparameterisation (model_vae.py:89-96, 169-181) of the [B, d] pre-activations of the mean and std Dense layers (rows `ld`
 * floats apart, also for dm_pre / ds_pre: both may be column blocks of one [B, 2d] tensor):
 * mean = clip(m, -100, 100), std = clip(sqrt(softplus(s)), -5, 5), z [B, N, d] = mean_b + std_b * eps[b, n, :] with eps the
 * caller's [B, N, d] tensor or, when eps is NULL, noise elements b N d + n d + k of (seed, *step);
 * kl [B] (may be NULL) = N * sum_k (1 + 2 log(std + 1e-10) - mean^2 - std) -- the KL loss is -1/2 mean_b kl[b].  d <= 64.
 * The backward regenerates the same eps; dz[0 .. num_dz-1] (num_dz <= KGCN_VAE_MAX_CHANNELS + 1) are gradients of z from its
 * consumers, added in order; dkl [B] (NULL = 0) is the gradient arriving at kl; tf.clip_by_value's gradient passes at
 * equality. */
int kgcn_vae_sample_fwd_f32(const float* m_pre, const float* s_pre, int32_t num_graphs, int32_t n_nodes, int32_t d, int32_t ld,
                            const float* eps, uint64_t seed, const int64_t* step, float* z, float* kl, void* stream);
int kgcn_vae_sample_bwd_f32(const float* m_pre, const float* s_pre, int32_t num_graphs, int32_t n_nodes, int32_t d, int32_t ld,
                            const float* eps, uint64_t seed, const int64_t* step, const float* const* dz, int32_t num_dz,
                            const float* dkl, float* dm_pre, float* ds_pre, void* stream);
/* Reconstruction cost (model_vae.py:203-253) without the [B, C, N, N] logits: adj_ch[c] (host array of C descriptors, any
 * row_pad) are the target adjacencies, label(i, j) = value of entry (i, j) (a repeated column: the last entry of the row);
 * y[c] the [B, N, d] decoder outputs and w[c] the [d] DistMult kernels of channel c (host arrays of device pointers);
 * feat_logits / feat_target [B, N, f].  Per graph b:
 *   per_graph[b]      = mean over N, f of sigmoid CE(feat_logits, feat_target)
 *   per_graph[B + b]  = mean over C, N, N of sigmoid CE(L_c, label_c), L_c = (y_c * w_c) y_c^T
 *   per_graph[2B + b] = mean over N, N of [max_c L_c > 0] == [max_c label_c > 0.5]
 * sums[0] = cost_opt = mean_b mask_b (feature + link) - 1/2 mean_b kl[b], sums[1] = cost_sum = mean_b mask_b (feature + link),
 * sums[2] = correct_count = sum_b mask_b per_graph[2B + b]; mask / kl NULL = ones / zeros; means over the padded batch.
 * Backward: g_opt / g_sum device scalars (NULL = 0) arriving at cost_opt / cost_sum; writes dy[c] [B, N, d], dfeat [B, N, f],
 * dkl [B] (may be NULL) = -1/2 g_opt / B, and dw[c] [d] (dw or dw[c] may be NULL) through per-workgroup partials in
 * `workspace` (>= kgcn_vae_recon_workspace_bytes(B, C, d)) and a fixed-order second stage (deferrable: kgcn_reduce_defer).
 * Limits: N <= 128, C <= 8, d <= 64; outside them the call fails.  Results are bitwise reproducible. */
int64_t kgcn_vae_recon_workspace_bytes(int32_t num_graphs, int32_t num_channels, int32_t d);
int kgcn_vae_recon_fwd_f32(const kgcn_csr_batch* adj_ch, int32_t num_channels, const float* const* y, const float* const* w,
                           int32_t d, const float* feat_logits, const float* feat_target, int32_t f, const float* mask,
                           const float* kl, float* per_graph, float* sums, void* stream);
int kgcn_vae_recon_bwd_f32(const kgcn_csr_batch* adj_ch, int32_t num_channels, const float* const* y, const float* const* w,
                           int32_t d, const float* feat_logits, const float* feat_target, int32_t f, const float* mask,
                           const float* g_opt, const float* g_sum, float* const* dy, float* const* dw, float* dfeat,
                           float* dkl, void* workspace, int64_t workspace_bytes, void* stream);

/* -- protein-sequence encoder of the multimodal model (example_model/model_multimodal.py:70-93) ---------------------------
 * Embedding(S, E) -> Conv1D(F, k, padding="same", relu) -> MaxPooling1D(p) -> LSTM(H, go_backwards=True).
 * Conv-pool: tokens [B, L] int32 in [0, S) (checked by the caller on the host, not here), table [S, E], w [k, E, F], bias [F]
 * -> out [B, L / p, F] = max over each pool window of relu(conv), TF SAME padding at stride 1 ((k-1)/2 zero positions on the left,
 * the rest on the right), positions >= (L / p) p dropped.  argmax (NULL under no_grad) [B, L / p, F] bytes: the lowest index in
 * the window among equal maxima, 0xFF when the maximum is not > 0 (relu passes no gradient).  Backward: d out -> d table [S, E],
 * d w, d bias through per-workgroup partials in `workspace` (>= kgcn_seq_convpool_workspace_bytes) and fixed-order second stages
 * (deferrable: kgcn_reduce_defer).  Limits: E <= 32, F <= 64, k <= 8, p <= 8, S <= 1024, L <= 8192.
 * LSTM: Keras v1 cell, gate order i, f, c, o, kernel wx [D, 4H], recurrent kernel wh [H, 4H], bias [4H]; recurrent activation
 * KGCN_SEQ_ACT_HARD_SIGMOID (clip(0.2 z + 0.5, 0, 1), gradient passing at the boundaries) or KGCN_SEQ_ACT_SIGMOID, tanh elsewhere,
 * zero initial state, x [B, T, D] processed from step T-1 down to 0 with no masking; h_out[b * h_ld + u] = h after step 0.
 * stash (NULL under no_grad): kgcn_seq_lstm_stash_floats(B, T, H) floats, per (b, t) the 4H gate pre-activations, h and c
 * (6H floats, 768 bytes a sequence step at H = 32).  The backward reads dh[b * dh_ld + u] (NULL = 0), OVERWRITES the
 * pre-activations of the stash with their gradients, writes dx [B, T, D] (may be NULL) and -- all three or none -- d wx, d wh,
 * d bias through partials in `workspace` (>= kgcn_seq_lstm_workspace_bytes) and fixed-order second stages (deferrable).  An
 * incomplete set of the three, or a workspace too small for them, is refused before the first launch: neither dx nor the stash
 * is touched by a refused call.
 * Limits: D <= 64, H <= 64, T <= 8192.  No float atomics: results are bitwise reproducible. */
#define KGCN_SEQ_MAX_EMBED 32
#define KGCN_SEQ_MAX_FILTERS 64
#define KGCN_SEQ_MAX_KERNEL 8
#define KGCN_SEQ_MAX_POOL 8
#define KGCN_SEQ_MAX_UNITS 64
#define KGCN_SEQ_MAX_LSTM_INPUT 64
#define KGCN_SEQ_MAX_SYMBOLS 1024
#define KGCN_SEQ_MAX_LENGTH 8192
#define KGCN_SEQ_ACT_HARD_SIGMOID 0
#define KGCN_SEQ_ACT_SIGMOID 1
int64_t kgcn_seq_convpool_workspace_bytes(int32_t batch, int32_t length, int32_t symbols, int32_t embed_dim, int32_t kernel_size,
                                          int32_t filters, int32_t pool);
int kgcn_seq_convpool_fwd_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* table, int32_t symbols,
                              int32_t embed_dim, const float* w, const float* bias, int32_t kernel_size, int32_t filters,
                              int32_t pool, float* out, uint8_t* argmax, void* stream);
int kgcn_seq_convpool_bwd_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* table, int32_t symbols,
                              int32_t embed_dim, const float* w, int32_t kernel_size, int32_t filters, int32_t pool,
                              const float* dout, const uint8_t* argmax, float* dtable, float* dw, float* dbias, void* workspace,
                              int64_t workspace_bytes, void* stream);
int64_t kgcn_seq_lstm_stash_floats(int32_t batch, int32_t steps, int32_t units);
int64_t kgcn_seq_lstm_workspace_bytes(int32_t batch, int32_t steps, int32_t in_dim, int32_t units);
int kgcn_seq_lstm_fwd_f32(const float* x, int32_t batch, int32_t steps, int32_t in_dim, const float* wx, const float* wh,
                          const float* bias, int32_t units, int32_t recurrent_act, float* h_out, int64_t h_ld, float* stash,
                          void* stream);
int kgcn_seq_lstm_bwd_f32(const float* x, int32_t batch, int32_t steps, int32_t in_dim, const float* wx, const float* wh,
                          const float* bias, int32_t units, int32_t recurrent_act, const float* dh, int64_t dh_ld, float* stash,
                          float* dx, float* dwx, float* dwh, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);
/* Integrated gradients over the embedded sequence (kgcn/visualization.py:187-231, the model built with feed_embedded_layer).
 * `batch` rows are rep copies of each of the batch / rep token rows (batch a multiple of rep).  Scaled forward: row b reads token
 * row b / rep and its embedding rows times scale[b] (the scaled [B, L, E] input is never written), otherwise exactly
 * kgcn_seq_convpool_fwd_f32 (out and argmax [batch, L / p, F]).  Input gradient: d out [batch, L / p, F] routed through argmax ->
 * dx [batch / rep, L, E] = sum over the copies r of compound c, in copy order, of row_weight[c rep + r] (NULL = 1; rows of weight 0
 * are skipped) times the gradient with respect to that row's scaled embedded input,
 *   sum_j sum_f dconv[m + (k-1)/2 - j, f] w[j, e, f]   (positions outside [0, (L / p) p) carry no conv gradient),
 * times table[tokens[c, m], e] when times_table is non-zero.  No weight gradient, no float atomics (bitwise reproducible).
 * Limits as the conv-pool above; a shape beyond them fails before any launch. */
int kgcn_seq_convpool_scaled_fwd_f32(const int32_t* tokens, int32_t batch, int32_t rep, const float* scale, int32_t length,
                                     const float* table, int32_t symbols, int32_t embed_dim, const float* w, const float* bias,
                                     int32_t kernel_size, int32_t filters, int32_t pool, float* out, uint8_t* argmax, void* stream);
int kgcn_seq_convpool_input_grad_f32(const int32_t* tokens, int32_t batch, int32_t rep, int32_t length, const float* table,
                                     int32_t symbols, int32_t embed_dim, const float* w, int32_t kernel_size, int32_t filters,
                                     int32_t pool, const float* dout, const uint8_t* argmax, const float* row_weight,
                                     int32_t times_table, float* dx, void* stream);
/* Noise of the smooth attribution methods (kgcn/visualization.py:235-259 smooth_grad / smooth_ig; kgcn/feed.py:88-89
 * add_perturbation draws it on the host).  One N(0, 1) value z per (seed, stream s, compound g, sample k, row r, column w) of a
 * 2-D array [R, W]: normal number w & 3 of the Philox4x64-10 block with counter (r ceil(W / 4) + (w >> 2), k, g, s) and key
 * (seed, 0), by the Box-Muller of the VAE noise above (24-bit uniforms; words 0, 1 give normals 0, 1 and words 2, 3 give normals
 * 2, 3).  g is the compound's index in the dataset and k the sample number (both read as unsigned 32-bit values), never the
 * position of the copy in a launch.  Streams: KGCN_IG_STREAM_FEATURES the node features [N, F], padding rows included;
 * KGCN_IG_STREAM_ADJACENCY + ch the stored values of adjacency channel ch of graph g as [1, nnz_g] in the CSR order of the batch;
 * KGCN_IG_STREAM_SEQUENCE the embedded sequence [L, E]; KGCN_IG_STREAM_VECTOR the per-graph vector of the vector-modality models
 * as [1, Dv] (adjacency channels occupy 1 .. 0xff, so 0x200 meets none of them).  The perturbed value is fma(sigma, z, x * scale) in fp32; a copy with
 * sigma == 0 is x * scale, the clean path's product, and draws nothing.
 * Rows: out [batch, rows, width], copy b = x[b / rep] (x [batch / rep, rows, width]) with scale[b], sigma[b], sample[b] and
 * ids[b / rep] (16-byte accesses when width % 4 == 0 and x, out are 16-byte aligned).  Values: out[e] for the entries e of a plain batched CSR (rowptr
 * [num_graphs rows + 1], nnz entries, values [nnz]), graph b owning rowptr[b rows] .. rowptr[(b + 1) rows] with scale[b],
 * sigma[b], sample[b], ids[b] (all PER GRAPH); graphs without entries and repeated (row, col) entries need nothing special (the
 * noise is per stored entry); max_nnz_per_graph only sizes the grid.  Perturbed conv-pool: kgcn_seq_convpool_scaled_fwd_f32 with
 * the window element at position l, column e = table[tok] * scale[b] + sigma[b] * z (stream KGCN_IG_STREAM_SEQUENCE, row l,
 * column e, g = ids[b / rep], k = sample[b]); positions outside [0, L) stay 0.  kgcn_seq_convpool_input_grad_f32 serves it
 * unchanged (it needs the arg-max bytes and the clean table only). */
#define KGCN_IG_STREAM_FEATURES 0u
#define KGCN_IG_STREAM_ADJACENCY 1u
#define KGCN_IG_STREAM_SEQUENCE 0x100u
enum { KGCN_IG_STREAM_VECTOR = 0x200 };
int kgcn_ig_perturb_rows_f32(const float* x, int64_t batch, int32_t rep, int32_t rows, int32_t width, const float* scale,
                             const float* sigma, const int32_t* sample, const int32_t* ids, uint32_t noise_stream, uint64_t seed,
                             float* out, void* stream);
int kgcn_ig_perturb_values_f32(const int32_t* rowptr, int32_t num_graphs, int32_t rows, int64_t nnz, int32_t max_nnz_per_graph,
                               const float* values, const float* scale, const float* sigma, const int32_t* sample,
                               const int32_t* ids, uint32_t noise_stream, uint64_t seed, float* out, void* stream);
int kgcn_seq_convpool_perturbed_fwd_f32(const int32_t* tokens, int32_t batch, int32_t rep, const float* scale, const float* sigma,
                                        const int32_t* sample, const int32_t* ids, uint64_t seed, int32_t length, const float* table,
                                        int32_t symbols, int32_t embed_dim, const float* w, const float* bias, int32_t kernel_size,
                                        int32_t filters, int32_t pool, float* out, uint8_t* argmax, void* stream);
/* dx[b, n, :] = dout[b * dout_ld + :d]: the gradient of a GraphGather read-out written into a column block of a wider buffer
 * (kgcn_graph_gather_fwd_ld_f32), read where it lies */
int kgcn_graph_gather_bwd_ld_f32(const float* dout_grad, int64_t dout_ld, int64_t batch, int32_t n_nodes, int32_t d, float* dx,
                                 void* stream);

/* -- knowledge-graph link prediction (sample_kg/network_prediction/model_py/{gcn,distmult,ip}.py) ---------------------------
 * h [N, D] node rows, labels [M, 6] int32 (i, r, j, i', r', j'), perm [M] (NULL = identity), negatives [K] (the sorted node set
 * of columns 0 and 2 of the fed list, kgcn/feed.py:8-16).  All node and relation ids must lie in [0, N) / [0, R): checked by the
 * caller on the host, not here.
 * Forward (one label batch of L rows): window j = *step mod floor(M / L) (step NULL = 0; read on the device), row i =
 * labels[perm[j L + i]] with col 3 := col 0 and col 5 := negatives[u], u uniform in [0, K) without bias from Philox4x64-10,
 * key (seed, 0), counter (i, *step, round, 0), words in order, Lemire's multiply-shift with rejection of the low halves below
 * 2^64 mod K.  Writes rows [L, 6], s1 [L] = sum_d h[c0] h[c2] w[c1], s2 [L] = sum_d h[c3] h[c5] w[c4] (w = 1 unless DISTMULT),
 * sums [5] = cost_opt, cost_sum, correct_count, S1, S2:
 *   KGCN_LP_GCN       cost_i = -log(sigmoid(s1 - s2) + 1e-10), cost_opt = mean, correct = sum [s1 > s2]
 *   KGCN_LP_DISTMULT  cost_i = -log(1 / (1 + exp(s2 - s1 + 0.1)) + 1e-10)
 *   KGCN_LP_IP        one cost on S1 = sum_i s1_i, S2 = sum_i s2_i (cost_opt = cost_sum = cost, correct = [S1 > S2]); S1, S2 kept
 * Where exp(s2 - s1 + 0.1) overflows, the gradient is 0 (TF: NaN).  Backward: g_opt / g_sum (device scalars, NULL = 0) ->
 * dh [N, D] (every row written) and, for DISTMULT, dw [R, D] through per-workgroup partials in `workspace`
 * (>= kgcn_linkpred_workspace_bytes) and a fixed-order second stage (deferrable: kgcn_reduce_defer).  No float atomics:
 * results are bitwise reproducible.  Limits: D <= 256, L <= 2^22, R D <= 16384. */
#define KGCN_LP_GCN 0
#define KGCN_LP_DISTMULT 1
#define KGCN_LP_IP 2
#define KGCN_LP_MAX_DIM 256
#define KGCN_LP_MAX_BATCH (1 << 22)
#define KGCN_LP_MAX_REL_FLOATS 16384
int64_t kgcn_linkpred_workspace_bytes(int64_t nodes, int32_t dim, int32_t relations, int32_t mode, int32_t batch);
int kgcn_linkpred_fwd_f32(const float* h, int64_t nodes, int32_t dim, const float* w, int32_t relations, int32_t mode,
                          const int32_t* labels, const int32_t* perm, int64_t num_labels, int32_t batch, const int32_t* negatives,
                          int32_t num_negatives, uint64_t seed, const int64_t* step, int32_t* rows, float* s1, float* s2,
                          float* sums, void* stream);
int kgcn_linkpred_bwd_f32(const float* h, int64_t nodes, int32_t dim, const float* w, int32_t relations, int32_t mode,
                          const int32_t* rows, const float* s1, const float* s2, const float* sums, int32_t batch,
                          const float* g_opt, const float* g_sum, float* dh, float* dw, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* -- general Conv1D -> MaxPooling1D on the matrix pipe (sample_protein/sequence/cnn.py:36-79; csrc/conv1d.hip) ---------------
 * out [B, L / pool, F] = max over each pool window of act(conv(rows, w [k, Cin, F]) + bias [F]), Keras padding="same" at stride 1
 * ((k-1)/2 zero positions on the left, the rest on the right, per sequence), pool = 1: no pooling.  The rows are x [B, L, Cin]
 * (tokens and table NULL) or table[tokens[b, l]] (x NULL; tokens [B, L] int32, table [S, Cin]; a token outside [0, S) reads a zero
 * row).  act: KGCN_ACT_NONE / KGCN_ACT_RELU / KGCN_ACT_TANH.  Conv positions >= (L / pool) pool lie outside every window.  argmax
 * (NULL under no_grad) [B, L / pool, F] bytes: the lowest index in the window among equal maxima.
 * Backward: dout, argmax and the forward's out [B, L / pool, F] -> dx [B, L, Cin] (may be NULL; every row written), dw, dbias (both or
 * neither) through fixed-order partials in `workspace` (>= kgcn_conv1d_pool_workspace_bytes) and fixed-order second stages (deferrable:
 * kgcn_reduce_defer).  kgcn_embedding_grad_f32: dtable [S, E] = sum by symbol of dembedded [B, L, E] in a fixed order (rows of
 * unused symbols are zeros).  No float atomics: results are bitwise reproducible.
 * Limits: Cin, F, E <= 1024, k <= 8, pool <= 8, L <= 8192, S <= 1024; a shape beyond them fails before any launch. */
#define KGCN_CONV1D_MAX_CHANNELS 1024
#define KGCN_CONV1D_MAX_KERNEL 8
#define KGCN_CONV1D_MAX_POOL 8
#define KGCN_CONV1D_MAX_LENGTH 8192
#define KGCN_CONV1D_MAX_SYMBOLS 1024
int64_t kgcn_conv1d_pool_workspace_bytes(int32_t batch, int32_t length, int32_t in_dim, int32_t kernel_size, int32_t filters,
                                         int32_t pool);
int kgcn_conv1d_pool_fwd_f32(const float* x, const int32_t* tokens, const float* table, int32_t symbols, int32_t batch,
                             int32_t length, int32_t in_dim, const float* w, const float* bias, int32_t kernel_size,
                             int32_t filters, int32_t pool, int32_t act, float* out, uint8_t* argmax, void* stream);
int kgcn_conv1d_pool_bwd_f32(const float* x, const int32_t* tokens, const float* table, int32_t symbols, int32_t batch,
                             int32_t length, int32_t in_dim, const float* w, int32_t kernel_size, int32_t filters, int32_t pool,
                             int32_t act, const float* dout, const uint8_t* argmax, const float* out, float* dx, float* dw,
                             float* dbias, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_embedding_grad_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* dembedded, int32_t symbols,
                            int32_t embed_dim, float* dtable, void* stream);

/* -- integrated gradients of the link-prediction model (kgcn visualize, kgcn/visualization.py:289-439, on model_py/gcn.py;
 * csrc/kgig.hip) -----------------------------------------------------------------------------------------------------------
 * The network is relu(A (relu(A (E W1 + b1)) W2 + b2)) over ONE graph A [N, N] given as a plain CSR (indptr [N + 1], indices
 * [nnz], values [nnz]; A need not be symmetric or have unit values).  The embedded layer is scaled by scales[k], k = 0 .. K-1.
 * The caller computes once, for all targets: p = E W1 [N, C], g1 = A p [N, C], rowsum = A 1 [N], and the stash
 * h2 [K, N, C] = relu(A (relu(Z1_k) W2 + b2)) with Z1_k = scales[k] * g1 + rowsum (x) b1 formed as fp32 product, product, sum
 * (the kernel recomputes the layer-1 relu mask with exactly these roundings).  targets [T, 4] int32 = (a, b, a', b'):
 *   KGCN_KGIG_SCORE  the attributed quantity is s = h[a] . h[b] (a', b' are not read); score [T, K] = s per step
 *   KGCN_KGIG_LOSS   it is -log(sigmoid(s1 - s2) + 1e-10), s1 = h[a] . h[b], s2 = h[a'] . h[b']; score [T, K] = s1 - s2 per step
 * Outputs: node_ig [T, N], node_ig[t, j] = sum_d E[j, d] * (sum_k weights[k] d quantity / d (scales[k] E)[j, d]) -- the
 * attribution summed over the embedding axis, all the dump reads -- and, when u is not NULL, u [T, N, C] += sum_k weights[k]
 * dZ1_k (the caller zeroes it; rows outside the seeds' neighbourhoods stay zero), from which the full attribution is
 * E (.) ((A^T u) W1^T).  One persistent workgroup per target, `groups` of them (0: KGCN_KGIG_GROUPS) in a grid-stride loop.
 * No float atomics: bitwise reproducible.  NOT checked here (device memory), the caller checks on the host: indptr is
 * monotone from 0 to nnz, every row's columns are strictly increasing (sorted, no duplicates) and lie in [0, N), target ids
 * lie in [0, N).  A bad id never reads or writes out of bounds (the entry / target is skipped), but the result is undefined.
 * Limits: C == 128; N <= KGCN_KGIG_MAX_NODES (the target's node_ig row lives in LDS beside W2 and the 128-row product block);
 * 1 <= K <= KGCN_KGIG_MAX_STEPS. */
#define KGCN_KGIG_SCORE 0
#define KGCN_KGIG_LOSS 1
#define KGCN_KGIG_WIDTH 128
#define KGCN_KGIG_MAX_NODES 7168
#define KGCN_KGIG_MAX_STEPS 4096
#define KGCN_KGIG_GROUPS 256
int kgcn_kg_ig_f32(const int32_t* indptr, const int32_t* indices, const float* values, int64_t nnz, int32_t nodes, int32_t width,
                   const float* g1, const float* rowsum, const float* b1, const float* w2, const float* h2, const float* p,
                   const float* scales, const float* weights, int32_t steps, const int32_t* targets, int32_t num_targets,
                   int32_t mode, int32_t groups, float* node_ig, float* score, float* u, void* stream);

/* -- ranking of all node pairs of the link-prediction model (run_enrichment.sh: script/predscore.py; csrc/pairrank.hip) -------
 * The score of pair (i, j), i < j, is s_ij = sum_k (h[i,k] w[k]) h[j,k] over h [nodes, dim] (w NULL: gcn / ip; one relation's
 * DistMult vector otherwise), fp32 on the f32 MFMA, k ascending; the [N, N] matrix is never formed.  The list is in the order of
 * predscore.py:153: score, then row, then col, all descending; -0.0 ranks as +0.0 and NaN below every number.
 *   select  counts [3] (device int64) = T, count(key > T), count(key == T): T the uint32 key of the cutoff-th largest score
 *           (cutoff 0, or more than N (N - 1) / 2: of the smallest).  Asynchronous; workspace >= workspace_bytes(.., 0, 0).
 *   emit    score / row / col [min(cutoff or all, all)]: the head of the sorted list.  counts is select's output for the same
 *           operands, capacity >= counts[1] + counts[2] (the caller reads them: one synchronisation) and <=
 *           KGCN_PAIRRANK_MAX_CANDIDATES; workspace >= workspace_bytes(.., capacity, 0).  Nothing is written past the capacity:
 *           the call reads the candidate counter back (it synchronises the stream) and fails when the buffer was too small.
 *   table   on a sorted list of `entries` rows: train_edge / test_edge / new_edge [entries] uint8 by membership of
 *           row << 16 | col in target_codes (train + test) and test_codes (both sorted ascending, duplicate-free, device uint32),
 *           score_ranking [entries] int64 = 1 + the entries with a larger score (ties share the smallest rank), and for the
 *           num_top <= KGCN_PAIRRANK_MAX_TOP HOST thresholds top_ratio[p]: hits[p] = test entries among the first top_ratio[p]
 *           entries that are no train edge, covered[p] = whether the list holds that many such entries (device int64 each).
 *           workspace >= workspace_bytes(.., 0, entries).
 * No float atomics: bitwise reproducible.  Not for hipGraph capture (emit synchronises). */
#define KGCN_PAIRRANK_MAX_NODES 65536
#define KGCN_PAIRRANK_MAX_CANDIDATES (1 << 28)
#define KGCN_PAIRRANK_MAX_TOP 16
int64_t kgcn_pair_rank_workspace_bytes(int32_t nodes, int32_t dim, int64_t capacity, int64_t entries);
int kgcn_pair_rank_select_f32(const float* h, int32_t nodes, int32_t dim, const float* w, int64_t cutoff, int64_t* counts,
                              void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_pair_rank_emit_f32(const float* h, int32_t nodes, int32_t dim, const float* w, int64_t cutoff, const int64_t* counts,
                            int64_t capacity, float* score, int32_t* row, int32_t* col, void* workspace, int64_t workspace_bytes,
                            void* stream);
int kgcn_pair_rank_table_i32(const float* score, const int32_t* row, const int32_t* col, int64_t entries,
                             const uint32_t* target_codes, int64_t num_target, const uint32_t* test_codes, int64_t num_test,
                             const int64_t* top_ratio, int32_t num_top, uint8_t* train_edge, uint8_t* test_edge, uint8_t* new_edge,
                             int64_t* score_ranking, int64_t* hits, int64_t* covered, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* -- classical graph kernels of graph_kernel/gk.py (csrc/graphkern.hip, kgcn_amd/graph_kernel.py) ------------------------------
 * Weisfeiler-Lehman subtree and shortest-path features of a batch of graphs and the Gram matrix over them, integer-exact and
 * bitwise reproducible.  a: a plain (row_pad == 0) square batch of T graphs x M padded rows; num_nodes [T]: rows >=
 * num_nodes[t] do not exist; stored values are ignored and every stored entry is one edge occurrence (a repeated entry is a
 * multi-edge); labels / colors [T*M]: dense ranks >= 0 (what rows that do not exist hold is not read as a colour of theirs).
 * Every call is asynchronous on `stream`; workspaces are the caller's, sized by the *_workspace_bytes queries.
 *
 * Feature runs: (run_col, run_graph, run_count), one run per (feature column, graph) with a non-zero count.  kgcn_wl_runs_i32
 * and kgcn_sp_features_i32 are called twice: with run_col == NULL they count the runs of every graph and write run_ptr [T + 1]
 * (run_ptr[0] = 0, then the inclusive scan: run_ptr[T] is the total; needs the workspace of kgcn_graph_runs_workspace_bytes),
 * with the three buffers (capacity entries each) they write graph t's runs from run_ptr[t] on in ascending column order and
 * never past the capacity.
 *
 *   kgcn_wl_refine_i32   one refinement step, first half: sorted_nbr [nnz] receives every row's neighbour colours in ascending
 *                        order (at the row's own rowptr range; any degree), key_hi / key_lo [T*M] a 128-bit mix of the row's
 *                        signature (own colour, degree, multiset of neighbour colours), both words and-ed with hash_mask (all
 *                        ones in production; a narrow mask forces collisions for tests).  Rows that do not exist: all ones.
 *   kgcn_wl_rank_i32     second half: rows ordered by key (two stable 64-bit radix passes), a new colour wherever the key
 *                        changes, dense colours by a scan -> new_colors [T*M] (-1 for rows that do not exist).  info[0] = the
 *                        number of colours; info[1] = pairs of neighbours in that order with EQUAL keys whose true signatures
 *                        (existence, own colour, degree, sorted list) differ: the partition is exact iff it is 0.
 *   kgcn_wl_runs_i32     the colour histogram of every graph as runs, column = column_offset + colour (rows <= 4,096).
 *   kgcn_sp_features_i32 unweighted all-pairs shortest paths (breadth-first search in LDS, one workgroup a graph) and the runs of
 *                        the keys label_k << 20 | label_j << 8 | distance over ALL ordered pairs (k, j), k = j and unreachable
 *                        pairs (distance 255) included.  Refuses M > 128 and num_labels > 4,096 (labels must be < num_labels).
 *   kgcn_gram_plan_i64   sorts the runs by column; a column that occurs in one graph goes to an exact int64 diagonal sum of
 *                        count^2 (integer atomics), the others get dense indices.  stats [3] = columns, one-graph columns, dense
 *                        columns.  Leaves its plan in the workspace.
 *   kgcn_gram_dense_f64  gram [G, G] from the plan in the SAME workspace (same runs, graphs, chunk_cols; dense_cols = stats[2]):
 *                        the dense columns are laid out chunk_cols (a multiple of 16) at a time as [G_pad, chunk_cols] int32 counts
 *                        and multiplied on v_mfma_f64_16x16x4_f64 into the upper-triangle tiles, mirrored on store; then the
 *                        diagonal sums are added.  Sums of non-negative integers: exact below 2^53, in any order.  G <= 46,340.
 *   kgcn_gram_normalize_f64  out_ij = gram_ij / sqrt(gram_ii * gram_jj), 0 where either diagonal entry is 0 (out != gram). */
int kgcn_wl_refine_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, uint64_t hash_mask,
                       int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream);
int64_t kgcn_wl_rank_workspace_bytes(int64_t rows);
int kgcn_wl_rank_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, const int32_t* sorted_nbr,
                     const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors, int64_t* info, void* workspace,
                     int64_t workspace_bytes, void* stream);
int64_t kgcn_graph_runs_workspace_bytes(int32_t graphs);
int kgcn_wl_runs_i32(const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, uint64_t column_offset,
                     int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count, int64_t capacity, void* workspace,
                     int64_t workspace_bytes, void* stream);
int kgcn_sp_features_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int32_t num_labels,
                         int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count, int64_t capacity,
                         void* workspace, int64_t workspace_bytes, void* stream);
int64_t kgcn_graph_gram_workspace_bytes(int64_t runs, int32_t graphs, int32_t chunk_cols);
int kgcn_gram_plan_i64(const uint64_t* run_col, const int32_t* run_graph, const int32_t* run_count, int64_t runs, int32_t graphs,
                       int32_t chunk_cols, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_gram_dense_f64(const int32_t* run_graph, const int32_t* run_count, int64_t runs, int32_t graphs, int64_t dense_cols,
                        int32_t chunk_cols, double* gram, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_gram_normalize_f64(const double* gram, int32_t graphs, double* out, void* stream);

/* -- hash graph kernels for continuous node attributes (csrc/hashkern.hip, kgcn_amd/graph_kernel.py hash_graph_kernel) ----------
 * graph_kernel/graphkernel/hash_graph_kernel.py of the reference: the attribute rows of all existing nodes, x [rows, d] fp64 in
 * graph order, are scaled, projected on R random directions and cut into buckets; the classical kernels above then run on R
 * colourings of the same graphs at once.  fp64 and integers, no float atomics: bitwise reproducible.  Asynchronous on `stream`.
 *
 *   kgcn_attr_scale_f64  scaled [rows, d], mean [d], std_dev [d] (population): per column the rows are added one after another in
 *                        ascending order inside chunks of 256 rows, then the chunk sums in ascending chunk order, every sum from
 *                        +0.0; mean = sum / rows; the same two stages over (x - mean) * (x - mean); std_dev = sqrt(sum / rows);
 *                        scaled = (x - mean) / (std_dev == 0 ? 1 : std_dev).  No operation is fused.  1 <= d <= KGCN_LSH_MAX_DIM.
 *   kgcn_lsh_buckets_f64 bucket [draws, rows] = floor((x . v_r + b_r) / w): v [draws, d], b [draws] on the device, bin_width one
 *                        HOST value w > 0; acc = 0, acc = acc + x_k * v_rk for k ascending, unfused.  errors [1] (device) counts
 *                        the values that are not finite or not below 2^62 in magnitude (their bucket is written as 0): the caller
 *                        refuses a non-zero count, nothing wraps.  Every attribute row is read once for all draws.
 *   kgcn_rank_pairs_i64  ranks [n] = the dense rank of (hi, lo) among the distinct pairs in ascending signed order (numpy's
 *                        unique(..., return_inverse) of the pairs), by two stable 64-bit radix passes as kgcn_wl_rank_i32.  mark
 *                        NULL or [n]: a row with mark < 0 does not exist, takes no part and gets -1.  info[0] = the number of
 *                        classes, info[1] = existing rows with hi = 2^63 - 1, which cannot be told from missing rows: refuse.
 *
 * R colourings ("copies") of the same T graphs over ONE stored batch: colors / labels / new_colors / key_hi / key_lo are
 * [copies, T*M], row c * T*M + p reading rowptr / cv of row p; sorted_nbr is [copies, nnz].  One launch sequence and one info
 * serve all copies.  kgcn_wl_rank_copies_i32 ranks all copies together: where the initial colours of different copies are
 * disjoint (the ranks of (copy, bucket)) every signature holds its copy's own colour, so the copies never share a colour and each
 * copy's partition is the one its own refinement gives.  The runs are written in slot order, slot = c * T + t (all graphs of copy
 * 0, then copy 1, ...): run_ptr is [copies * T + 1], run_graph holds t, and
 *   kgcn_wl_runs_copies_i32      column = column_offset + c * column_stride + colour
 *                                (the driver: offset = iteration << 32, stride = (iterations + 1) << 32);
 *   kgcn_sp_features_copies_i32  column = c << 32 | key; the breadth-first searches of a graph run once and their distance bytes stay
 *                                in LDS while the keys of every copy are built, sorted and run-length encoded.  M <= 128 and
 *                                labels < num_labels <= 4,096 in every copy.
 * copies >= 1, copies * T * M < 2^31 - 1 (refused beyond: positions and colours are int32).  Workspaces: those of the plain kernels
 * for copies * T*M rows and copies * T slots, kgcn_wl_rank_copies_workspace_bytes(T*M, copies) and
 * kgcn_graph_runs_copies_workspace_bytes(T, copies). */
enum { KGCN_LSH_MAX_DIM = 4096 };   /* attributes a row: a staged row of d | 1 doubles leaves a workgroup at least one in 64 KB */
int64_t kgcn_attr_scale_workspace_bytes(int64_t rows, int32_t d);
int kgcn_attr_scale_f64(const double* x, int64_t rows, int32_t d, double* scaled, double* mean, double* std_dev, void* workspace,
                        int64_t workspace_bytes, void* stream);
int kgcn_lsh_buckets_f64(const double* scaled, int64_t rows, int32_t d, const double* v, const double* b, int32_t draws,
                         const double* bin_width, int64_t* bucket, int64_t* errors, void* stream);
int64_t kgcn_rank_pairs_workspace_bytes(int64_t n);
int kgcn_rank_pairs_i64(const int64_t* hi, const int64_t* lo, const int32_t* mark, int64_t n, int32_t* ranks, int64_t* info,
                        void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_wl_refine_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int32_t copies,
                              uint64_t hash_mask, int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream);
int64_t kgcn_wl_rank_copies_workspace_bytes(int64_t rows, int32_t copies);
int kgcn_wl_rank_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int32_t copies,
                            const int32_t* sorted_nbr, const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors,
                            int64_t* info, void* workspace, int64_t workspace_bytes, void* stream);
int64_t kgcn_graph_runs_copies_workspace_bytes(int32_t graphs, int32_t copies);
int kgcn_wl_runs_copies_i32(const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, int32_t copies,
                            uint64_t column_offset, uint64_t column_stride, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph,
                            int32_t* run_count, int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_sp_features_copies_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int32_t copies,
                                int32_t num_labels, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count,
                                int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream);

/* -- batched C-SVC over a precomputed kernel (csrc/svm.hip; kgcn_amd/graph_kernel.py svm_fit / svm_decision / svm_predict / svm_cv)
 * The nested KFold / SVC(kernel="precomputed") loop of graph_kernel/gk.py:243-292 as one batch of independent dual problems
 *   min 1/2 a^T Q a - e^T a,  0 <= a_t <= C,  y^T a = 0,   Q_st = y_s y_t K[idx_s, idx_t]
 * over ONE shared matrix K [graphs, graphs] fp64 (row-major, read in place through the index sets; no sub-matrix is formed),
 * solved by libsvm's SMO (svm.cpp Solver::Solve, select_working_set: second-order working-set selection, TAU = 1e-12;
 * calculate_rho) in fp64, without shrinking and without a kernel cache, one workgroup a problem.  fp64 and integers, no float
 * atomics, nothing fused: bitwise reproducible, and independent of the workgroup size, the wave order and the slicing below.
 *
 * Index sets: `sets` of them, set s = set_idx[set_ptr[s] .. set_ptr[s+1]) rows of K (set_ptr [sets + 1] ascending from 0 to
 * set_total), set_sign [set_total] the label +1 / -1 of each entry (the sign lives with the set, not with the row: a one-vs-one pair
 * relabels rows; evaluation sets have none), max_rows >= the longest set.  All arrays on the device.  A problem p is (set
 * prob_set[p], C = prob_C[p] > 0); problems that differ only in C share a set.
 *
 *   kgcn_svm_smo_f64   one SLICE of at most iters_per_launch iterations of every unfinished problem (a kernel's running time is
 *       bounded; the caller relaunches while the word below is not 0).  first != 0 starts from alpha = 0, G = -1; otherwise from
 *       the alpha [problems, max_rows] and the G in the workspace the previous slice left, so slicing changes no bit.  An iteration:
 *       i = argmax of -y_t G_t over I_up; row i of K gathered into registers; j = argmin of -b^2 / a over I_low with b = Gmax +
 *       y_t G_t > 0, a = (QD_i + QD_t) - 2 K_it (TAU where a <= 0); row j gathered; the clipped two-variable update exactly as
 *       libsvm orders it, both label cases; G_t = G_t + ((Q_it d_i) + (Q_jt d_j)).  Reductions carry (value, index) and among equal
 *       values the LAST index wins, as libsvm's `>=` / `<=` scans do.  Stops when m(alpha) - M(alpha) < *tol (status
 *       KGCN_SVM_CONVERGED) or after max_iter iterations in all (KGCN_SVM_MAX_ITER; max_iter <= 0: libsvm's max(10^7, 100 n)).
 *       Then rho: with free vectors acc = +0.0, acc = acc + y_t G_t over the free t ascending, rho = acc / count; with none the
 *       midpoint of the bounds.  Outputs: alpha, rho [problems], n_iter [problems], status [problems] (KGCN_SVM_*); a problem
 *       whose descriptor is out of range (set, length, row index, sign, C) touches no memory and gets KGCN_SVM_REFUSED.  The
 *       first 4 bytes of the 256-byte aligned workspace hold the number of problems still KGCN_SVM_RUNNING after the slice.
 *       Refused before any launch: max_rows > KGCN_SVM_MAX_ROWS (G, alpha, QD, the indices and signs of a problem live in LDS).
 *   kgcn_svm_decision_f64   job q = (problem job_prob[q], evaluation set job_eval[q]) writes dec[job_out[q] + r] for every row
 *       r of the set: acc = +0.0, acc = acc + (alpha_t y_t) K[row_r, idx_t] for t = 0, 1, ... over ALL training rows, dec =
 *       acc - rho.  job_out [jobs + 1] ascending, job_out[q + 1] - job_out[q] = the set's length, job_out[jobs] = dec_total.
 *       Positive: the +1 class (scikit-learn's two-class decision_function is the negative).
 *   kgcn_svm_vote_i32   vote v takes the classes (classes - 1) / 2 consecutive jobs vote_first_job[v] ... (libsvm's pair order (0, 1),
 *       (0, 2), ..., (1, 2), ...; +1 is the pair's first class; all on evaluation set vote_eval[v]) and writes pred[vote_out[v] + r]
 *       = the class index with the most votes, dec > 0 voting for the first class of a pair and anything else for the second, the
 *       lowest index among equals (svm_predict_values).  correct[v] = the rows whose prediction equals labels[row] (class
 *       indices of the rows of K; integer atomics).  2 <= classes <= KGCN_SVM_MAX_CLASSES.
 * decision and vote: errors [1] (device) counts jobs / rows whose descriptors are out of range (nothing is read or written for
 * them): the caller refuses a non-zero count.  Asynchronous on `stream`. */
enum { KGCN_SVM_MAX_ROWS = 4096, KGCN_SVM_MAX_CLASSES = 64, KGCN_SVM_DEFAULT_SLICE = 2048 };
enum { KGCN_SVM_RUNNING = 0, KGCN_SVM_CONVERGED = 1, KGCN_SVM_MAX_ITER = 2, KGCN_SVM_REFUSED = 3 };
int64_t kgcn_svm_workspace_bytes(int32_t problems, int32_t max_rows);
int kgcn_svm_smo_f64(const double* K, int32_t graphs, const int64_t* set_ptr, const int32_t* set_idx, const int8_t* set_sign,
                     int32_t sets, int64_t set_total, int32_t max_rows, const int32_t* prob_set, const double* prob_C,
                     int32_t problems, const double* tol, int64_t max_iter, int32_t iters_per_launch, int32_t first, double* alpha,
                     double* rho, int64_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_svm_decision_f64(const double* K, int32_t graphs, const int64_t* set_ptr, const int32_t* set_idx, const int8_t* set_sign,
                          int32_t sets, int64_t set_total, int32_t max_rows, const int32_t* prob_set, int32_t problems,
                          const double* alpha, const double* rho, const int64_t* eval_ptr, const int32_t* eval_idx, int32_t evals,
                          int64_t eval_total, int32_t eval_max_rows, const int32_t* job_prob, const int32_t* job_eval,
                          const int64_t* job_out, int32_t jobs, double* dec, int64_t dec_total, int64_t* errors, void* stream);
int kgcn_svm_vote_i32(const double* dec, int64_t dec_total, const int64_t* job_out, int32_t jobs, const int64_t* eval_ptr,
                      const int32_t* eval_idx, int32_t evals, int64_t eval_total, int32_t eval_max_rows,
                      const int32_t* vote_first_job, const int32_t* vote_eval, const int64_t* vote_out, int32_t votes,
                      int32_t classes, const int32_t* labels, int32_t graphs, int32_t* pred, int64_t pred_total, int64_t* correct,
                      int64_t* errors, void* stream);

/* -- active learning: label propagation and query scoring (csrc/labelprop.hip; kgcn_amd/active_learning.py) -----------------------
 * active_learning/models.py of the reference fits scikit-learn's LabelPropagation / LabelSpreading once per task and scores the
 * unlabelled rows.  Here ONE affinity matrix W [n, n] fp64 (row-major) serves every task and every query over the same points; the
 * variants' scalings are applied to W F instead of being stored as a second matrix.  fp64 and integers, no float atomics, nothing
 * fused: a pure function of the input.  "The lane tree": of 64 values v_0 .. v_63, v_l = v_l + v_(l ^ off) for off = 32, 16, 8, 4,
 * 2, 1 in turn.  All arrays on the device unless said otherwise; doubles are passed by address (host memory).  Asynchronous.
 *
 *   kgcn_rbf_affinity_f64   x [n, d] -> W_ij = exp(-gamma max(0, (|x_i|^2 + |x_j|^2) - 2 x_i.x_j)), W_ii = exp(-0) = 1
 *       (sklearn.metrics.pairwise.rbf_kernel).  norms [n] receives |x_i|^2 = acc + x_ik x_ik for k ascending from +0.0.  The dot
 *       products are formed on v_mfma_f64_16x16x4_f64 (its internal order and the device exp are not restated: W is compared by
 *       tolerance).  Entries with i <= j are computed and stored at (i, j) and (j, i): W is symmetric bit for bit.  Refused before
 *       any launch: n * n * 8 > max_bytes, n > KGCN_LP_MAX_ROWS.
 *   kgcn_lp_degrees_f64     s_i = sum_j W_ij (LabelPropagation's normaliser), d_i = the same with the term j = i replaced by +0.0 (the
 *       degree of scipy's normed Laplacian).  Lane l adds j = l, l + 64, ... ascending from +0.0; then the lane tree.
 *   kgcn_lp_propagate_f64   the label block F [n, cols] holds the class columns of task t at task_col[t] .. task_col[t + 1] (task_col
 *       [tasks + 1] ascending from 0 to cols, every task at least one column); labels [n, tasks] = the class index inside the task or
 *       -1.  first_step == 0 starts: F = one-hot labels, status = KGCN_LP_RUNNING, n_iter = 0.  Then `steps` steps, numbered from
 *       first_step.  A step, for the tasks still running:
 *         raw_ic = sum_j w_ij G_jc: lane l adds the rounded products for j = l, l + 64, ... ascending from +0.0, then the lane tree;
 *         propagation (scale = s): G = F, w = W; v_c = raw_ic / s_i; norm = the v_c of the task added in column order from +0.0
 *           (0 counts as 1); F'_ic = v_c / norm on rows with label -1 in the task, the one-hot label on the others;
 *         spreading (scale = d): G_jc = F_jc / q_j with q_j = sqrt(d_j) (1 where d_j = 0), w = W without its diagonal;
 *           F'_ic = alpha (raw_ic / q_i) + (1 - alpha) onehot_ic;
 *         delta (row, task) = |F'_ic - F_ic| added in column order from +0.0; the partial of a block of KGCN_LP_BLOCK_ROWS rows = its
 *           rows' deltas added in row order from +0.0; the task's sum = the partials added in block order from +0.0.
 *       After step number k - 1 (and, with k = 0, after the start, where the sum is over |F|) a running task with k >= max_iter gets
 *       KGCN_LP_MAX_ITER and n_iter = max_iter, otherwise one whose sum < *tol gets KGCN_LP_CONVERGED and n_iter = k
 *       (BaseLabelPropagation.fit).  A task that is not running is frozen: its columns keep their bits.  The first 4 bytes of the
 *       256-byte aligned workspace hold the number of tasks still running: the one word a caller reads back, after as many steps
 *       as it likes; how the steps are cut into calls changes no bit and no n_iter.  *alpha is read for spreading only.
 *   kgcn_lp_finish_f64      dist [n, cols] = F / (the task's columns added in order from +0.0; 0 counts as 1) after steps_done steps in
 *       all (the caller's count of the steps it asked for).
 *   kgcn_lp_scores_f64      scores [5, m] of the rows cand [m] of dist (a row outside 0..n-1: NaN), p = the row's block of task t:
 *         KGCN_LP_SCORE_E         sum over tasks, in task order from +0.0, of sum_c entr(p_c / sum_c p_c) (scipy.stats.entropy; both sums in
 *                                 column order from +0.0; entr(0) = 0; an all-zero block gives NaN)
 *         KGCN_LP_SCORE_LC_MEAN   1 - max_c mean_c, mean_c = (p_c added over the tasks in order from +0.0) / tasks (query_next_data_points)
 *         KGCN_LP_SCORE_MS_MEAN   the largest minus the second largest mean_c; both _MEAN scores are NaN unless all tasks have the same
 *                                 number of classes, MS_MEAN also with one class
 *         KGCN_LP_SCORE_LC_TASKS  (max_c p_c added over the tasks from +0.0) / tasks (ActiveLearner.query)
 *         KGCN_LP_SCORE_MS_TASKS  the tasks' margins added in order from +0.0: largest minus second largest p_c, the only column of a
 *                                 one-class task
 *   kgcn_lp_select_f64      out [k] = positions into cand, -1 where fewer than k take part.  THE TIE RULE: candidates are ordered as a
 *       stable ascending sort orders them, NaN last (by score, then by position; all NaN equal).  largest != 0: out = the last k of
 *       that order, in that order (out[k - 1] is the very last: the E / LC top-k of query_next_data_points, the E pick of
 *       ActiveLearner.query); largest == 0: its first k (MS top-k; with k = 1 the first among equal minima, np.argmin).  numpy's
 *       default argsort is not stable: where scores tie the reference's own order is unspecified.  active NULL or [n]: a candidate
 *       whose row has active == 0 takes no part.  truth != NULL (k = 1 only) teaches the picked row on the device: labels[row, :] =
 *       truth[row, :] ([n, tasks] both), active[row] = 0, log[0] = the picked position (log may be NULL).  1 <= k <= KGCN_LP_MAX_PICKS.
 *
 * The same without a stored W (entry points only, version still 2): each 64 x 64 tile of w is rebuilt where it is consumed, in
 * O(n (d + cols)) memory.  Every w_ij is formed as kgcn_rbf_affinity_f64 forms it (the same norms, 16 attributes staged and 4 fed
 * to the MFMA at a time, NaN kept, distance 0 where the two points are the same row of the same set), column tiles start at
 * multiples of 64 and are walked upwards, a column past the set adds no term: the results below are the stored route's bit for bit.
 *   kgcn_rbf_apply_f64      out [m, cols] = sum_j w(q_i, r_j) G_jc for queries xq [m, d], references xr [n, d] (1 <= n <=
 *       KGCN_LP_MAX_ROWS; m >= 1 is not bounded by it) and G [n, cols], 1 <= cols <= KGCN_LP_MAX_COLS: lane l adds the rounded
 *       products for j = l, l + 64, ... ascending from +0.0, then the lane tree.  same_set != 0: xq == xr and m == n, the diagonal
 *       distance is 0, and zero_diagonal != 0 counts w_ii as +0.0 (refused without same_set).  norms_q [m] and norms_r [n] receive
 *       the squared norms (norms_q is not touched, and may be NULL, with same_set).
 *   kgcn_rbf_degrees_f64    s_out, d_out [n] of kgcn_lp_degrees_f64 from x [n, d], in its order; norms [n] receives the squared norms.
 *   kgcn_lp_propagate_free_f64   kgcn_lp_propagate_f64 with (x [n, d], d, gamma) in place of W: the same protocol (first_step / steps,
 *       the workspace of kgcn_lp_workspace_bytes, status / n_iter / the running word), the same steps, partials (one per block of
 *       KGCN_LP_BLOCK_ROWS rows, in block order) and decisions.  norms [n] is written by the call with first_step == 0 and read by
 *       the later ones.  scale = s or d of kgcn_rbf_degrees_f64.
 *   All three refuse before any launch: a NULL operand, d < 1, n outside 1..KGCN_LP_MAX_ROWS, a gamma that is not positive and
 *   finite, cols out of range, a short workspace. */
enum { KGCN_LP_MAX_ROWS = 131072, KGCN_LP_MAX_TASKS = 32, KGCN_LP_MAX_COLS = 64, KGCN_LP_BLOCK_ROWS = 32, KGCN_LP_MAX_PICKS = 8,
       KGCN_LP_DEFAULT_CHECK = 8 };
enum { KGCN_LP_PROPAGATION = 0, KGCN_LP_SPREADING = 1 };
enum { KGCN_LP_RUNNING = 0, KGCN_LP_CONVERGED = 1, KGCN_LP_MAX_ITER = 2 };
enum { KGCN_LP_SCORE_E = 0, KGCN_LP_SCORE_LC_MEAN = 1, KGCN_LP_SCORE_MS_MEAN = 2, KGCN_LP_SCORE_LC_TASKS = 3, KGCN_LP_SCORE_MS_TASKS = 4 };
int kgcn_rbf_affinity_f64(const double* x, int64_t n, int32_t d, const double* gamma, int64_t max_bytes, double* W, double* norms,
                          void* stream);
int kgcn_lp_degrees_f64(const double* W, int64_t n, double* s_out, double* d_out, void* stream);
int64_t kgcn_lp_workspace_bytes(int64_t n, int32_t tasks, int32_t cols);
int kgcn_lp_propagate_f64(const double* W, const double* scale, int64_t n, const int32_t* labels, const int32_t* task_col,
                          int32_t tasks, int32_t cols, int32_t variant, const double* alpha, const double* tol, int32_t max_iter,
                          int32_t first_step, int32_t steps, int32_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes,
                          void* stream);
int kgcn_lp_finish_f64(int64_t n, const int32_t* task_col, int32_t tasks, int32_t cols, int32_t steps_done, double* dist,
                       const void* workspace, int64_t workspace_bytes, void* stream);
int kgcn_lp_scores_f64(const double* dist, int64_t n, const int32_t* task_col, int32_t tasks, int32_t cols, const int32_t* cand,
                       int64_t m, double* scores, void* stream);
int kgcn_lp_select_f64(const double* score, const int32_t* cand, int64_t m, int64_t n, int32_t* active, int32_t k, int32_t largest,
                       int32_t* out, int32_t* labels, const int32_t* truth, int32_t tasks, int32_t* log, void* stream);
int kgcn_rbf_apply_f64(const double* xq, int64_t m, const double* xr, int64_t n, int32_t d, const double* gamma, const double* G,
                       int32_t cols, int32_t same_set, int32_t zero_diagonal, double* out, double* norms_q, double* norms_r,
                       void* stream);
int kgcn_rbf_degrees_f64(const double* x, int64_t n, int32_t d, const double* gamma, double* s_out, double* d_out, double* norms,
                         void* stream);
int kgcn_lp_propagate_free_f64(const double* x, int32_t d, const double* gamma, double* norms, const double* scale, int64_t n,
                               const int32_t* labels, const int32_t* task_col, int32_t tasks, int32_t cols, int32_t variant,
                               const double* alpha, const double* tol, int32_t max_iter, int32_t first_step, int32_t steps,
                               int32_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* -- k-fold cross-validation of the compound-protein interaction networks (gcn.py train_cv; csrc/cvloss.hip, csrc/cvmetrics.hip)
 * Loss head of sample_chem/compound-protein_interaction/multitask.py:53-86 (singletask.py: tasks = 1): logits [batch, 2, tasks],
 * labels and mask_label [batch, tasks] (a row counts where mask_label != 0, is positive where labels != 0).
 *   stats      [3 tasks + 1] = each_cost | each_correct_count | each_count | cost: the summed two-class sparse softmax cross entropy
 *              softplus(z_other - z_label) per task, the rows whose argmax (a tie is class 0) is the label, the rows counted, and
 *              cost = sum over tasks (a sum, not a mean).  Counts are floats holding integers.
 *   prediction [batch, tasks] = softmax(logits, axis 1)[:, 1, :] = sigmoid(z1 - z0), for every row whatever its mask
 *   dlogits    [batch, 2, tasks] = d cost / d logits (0 for rows not counted)
 *   accum      NULL, or a [3 tasks + 1] block that the call adds stats to in place as its last step (fixed order, one addition
 *              per entry per call): a captured step accumulates an epoch on the device.
 * Fixed summation order, no float atomics; asynchronous and capturable. */
#define KGCN_SOFTMAX2_MAX_BATCH (1 << 24)
#define KGCN_SOFTMAX2_MAX_TASKS 65535
int kgcn_multitask_softmax2_ce_f32(const float* logits, const float* labels, const float* mask_label, int64_t batch, int32_t tasks,
                                   float* dlogits, float* prediction, float* stats, float* accum, void* stream);

/* Binary-classification metrics of compute_metrics (gcn.py:170-256) for all tasks in one call: score [n, tasks] with row stride
 * score_ld, label and mask [n, tasks] contiguous (mask NULL: every row counts, as the reference; a row counts where mask != 0,
 * is positive where label != 0).  Per task, counts [tasks, 8] int64, all exact:
 *   n_used, P, TP, FP (at score > threshold, strict), n_nonfinite, auc_num2, n_groups, 0
 * with auc_num2 = sum over the distinct scores g in descending order of (fp_g - fp_g-1) (tp_g + tp_g-1), so that
 * ROC-AUC = auc_num2 / (2 P (n_used - P)), and ap [tasks] fp64 = sum_g ((tp_g - tp_g-1) / P) (tp_g / (tp_g + fp_g)) (0 when P = 0),
 * added in a fixed order.  -0.0 ties with +0.0.  A task with n_nonfinite != 0 has no meaningful curve sums (the caller refuses it).
 * One radix sort of n * tasks 64-bit keys (rocPRIM) + one workgroup per task; no atomics: bitwise reproducible.  Asynchronous. */
#define KGCN_BINARY_METRICS_MAX_ELEMENTS (1ll << 31)
#define KGCN_BINARY_METRICS_MAX_TASKS (1 << 20)
int64_t kgcn_binary_metrics_workspace_bytes(int64_t n, int32_t tasks);
int kgcn_binary_metrics_f32(const float* score, int64_t score_ld, const float* label, const float* mask, int64_t n, int32_t tasks,
                            float threshold, int64_t* counts, double* ap, void* workspace, int64_t workspace_bytes, void* stream);

/* -- vector-modality models and regression (example_model/model_multimodal_vec.py, model_multimodal_regression.py;
 * csrc/shortm.hip, csrc/regress.hip)
 * Dense + BatchNormalization in learning phase 0 + activation for short batches, x [rows, k] with row stride x_ld:
 *   pre = x w + bias,  y = act(s (pre - mean) + beta),  s = gamma / sqrt(var + eps);   gamma NULL (then beta, mean, var NULL too):
 *   y = act(pre).  bias may be NULL.  y has row stride y_ld (a column block of a wider buffer).
 * One workgroup owns 16 output columns and every row: the forward is one launch; the backward is one launch that writes
 * dw [k, n], dbias, dgamma, dbeta [n] complete (each may be NULL) and dpre [rows, n] = d loss / d pre (NULL when no dX follows)
 * from x, the forward's y, dy (row stride dy_ld) and -- with gamma -- the pre-activations `pre` [rows, n] the forward stashed
 * (its `pre` argument; NULL there when no backward follows).  kgcn_dense_bn_short_dx_f32: dx [rows, k] (row stride dx_ld) =
 * dpre w^T.  Plain fp32 FMAs, fixed summation order, no float atomics, no alignment requirement.  kgcn_dense_bn_short_supported
 * answers the shape question on the host (1 / 0); every call outside it is refused before any launch. */
#define KGCN_DENSE_BN_SHORT_MAX_ROWS 256
#define KGCN_DENSE_BN_SHORT_MAX_K 8192
#define KGCN_DENSE_BN_SHORT_MAX_N 1024
int kgcn_dense_bn_short_supported(int64_t rows, int64_t k, int64_t n);
int kgcn_dense_bn_short_fwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t k, const float* w, const float* bias, int32_t n,
                                const float* gamma, const float* beta, const float* mean, const float* var, float eps, int32_t act,
                                float* y, int64_t y_ld, float* pre, void* stream);
int kgcn_dense_bn_short_bwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t k, int32_t n, const float* y, int64_t y_ld,
                                const float* dy, int64_t dy_ld, const float* pre, const float* gamma, const float* mean,
                                const float* var, float eps, int32_t act, float* dw, float* dbias, float* dgamma, float* dbeta,
                                float* dpre, void* stream);
int kgcn_dense_bn_short_dx_f32(const float* dpre, int64_t rows, int32_t n, const float* w, int32_t k, float* dx, int64_t dx_ld,
                               void* stream);
/* y[b, 0:n] = act(x[b, 0:n]) between column blocks with row strides x_ld / y_ld, and its backward dx = g act'(y). */
int kgcn_act_cols_fwd_f32(const float* x, int64_t x_ld, int64_t rows, int32_t n, int32_t act, float* y, int64_t y_ld, void* stream);
int kgcn_act_cols_bwd_f32(const float* y, int64_t y_ld, const float* g, int64_t g_ld, int64_t rows, int32_t n, int32_t act, float* dx,
                          int64_t dx_ld, void* stream);

/* Masked squared error of model_multimodal_regression.py:94-101: pred, labels, mask_label [batch, tasks] contiguous.
 *   stats [2 tasks + 2] = error_sum [tasks] | count [tasks] | cost_sum | cost_opt with error_sum[t] = sum_b mask_label (labels -
 *         pred)^2, count[t] = sum_b mask_label, cost_sum = sum_t error_sum[t], cost_opt = cost_sum / (batch tasks)
 *   dpred [batch, tasks] = d cost_sum / d pred (exactly 0 where mask_label == 0)
 *   accum NULL, or a [2 tasks + 1] block error_sum | count | cost_sum that the call adds its values to in place.
 * Fixed summation order, no float atomics; asynchronous and capturable. */
#define KGCN_SQERR_MAX_BATCH (1 << 24)
#define KGCN_SQERR_MAX_TASKS 65535
int kgcn_masked_sqerr_f32(const float* pred, const float* labels, const float* mask_label, int64_t batch, int32_t tasks, float* dpred,
                          float* stats, float* accum, void* stream);
/* The sums behind r2 / mse / gmfe (gcn.py:204-208) per task over n evaluated rows: pred and label [n, tasks] with row strides
 * pred_ld / label_ld, mask NULL or [n, tasks] contiguous (a row counts where mask != 0).  sums [tasks, 6] fp64 =
 *   n | sum y | sum (y - mean y)^2 | sum (y - p)^2 | sum log(y / p) over the rows with 0 < y / p < inf | the count of the other rows
 * two passes in fp64, fixed order, no atomics.  Asynchronous. */
#define KGCN_REGRESSION_SUMS_MAX_ROWS (1ll << 31)
int kgcn_regression_sums_f64(const float* pred, int64_t pred_ld, const float* label, int64_t label_ld, const float* mask, int64_t n,
                             int32_t tasks, double* sums, void* stream);

/* Integrated gradients of the compound-protein interaction multitask network (multitask.py:35-51: GraphConv(Wd), sigmoid, sum
 * over the node rows, Dense(2 T); kgcn/visualization.py:187-286): the sweep over the `steps` scaled copies of `compounds`
 * compounds for all `tasks` tasks (csrc/cpiig.hip; an entry point only, version still 2).
 * The caller forms once per compound P = sum_ch A_ch X W_ch and Q = sum_ch rowsum(A_ch) (x) b_ch, both [compounds, nodes, width]
 * contiguous, and per task u_t = V[:, T + t] - V[:, t] ([tasks, width]) and e_t = c[T + t] - c[t] ([tasks]) of the Dense layer.
 * Copy k has the pre-activation Z_k = alpha[k] P + gamma[k] Q, H_k = sigmoid(Z_k), and
 *   p [compounds, steps, tasks]         p[c, k, t] = sigmoid(sum_{n, j} H_k[n, j] u_t[j] + e_t): task t's prediction of copy k
 *   GA [compounds, tasks, nodes, width] GA[c, t] = sum_k wA[k] p (1 - p)[c, k, t] u_t[j] H_k (1 - H_k): the weighted sum over the
 *                                       copies of d prediction / d Z_k; GB the same with wB (wB and GB both NULL: not formed).
 * The sigmoid is evaluated from exp(-|z|): no overflow, no NaN, no cancellation in H (1 - H) or p (1 - p) at any |z|.  All sums
 * run in a fixed order without atomics and no workgroup spans two compounds: bitwise reproducible, and a compound's rows do
 * not depend on which other compounds the call holds.  A lane of the accumulate pass carries KGCN_CPIIG_TASKS_PER_PASS tasks;
 * more tasks take further passes over the copies.  workspace: kgcn_cpi_ig_workspace_bytes(compounds, width, tasks, steps) bytes.
 * Limits: nodes, width, tasks >= 1, steps >= 2 (the start and the end copy); the three grids must stay below 2^31 workgroups.
 * Asynchronous. */
#define KGCN_CPIIG_TASKS_PER_PASS 8
int64_t kgcn_cpi_ig_workspace_bytes(int32_t compounds, int32_t width, int32_t tasks, int32_t steps);
int kgcn_cpi_ig_f32(const float* P, const float* Q, int32_t compounds, int32_t nodes, int32_t width, const float* u, const float* e,
                    int32_t tasks, const float* alpha, const float* gamma, const float* wA, const float* wB, int32_t steps, float* p,
                    float* GA, float* GB, void* workspace, int64_t workspace_bytes, void* stream);

/* Integrated gradients over the per-graph vector of the vector-modality models (model_multimodal_vec.py:83-94,
 * model_multimodal_regression.py:83-86; kgcn/visualization.py:187-260): the sweeps over the `copies` scaled copies of `compounds`
 * compounds through the vector branch's first layer, Dense(Dv -> width) + BatchNormalization (learning phase 0) + activation
 * (csrc/vecig.hip; entry points only, version still 2).
 * expand: P [compounds, width] contiguous is v W of every compound, formed once by the caller; copy k of compound c is row
 *   c copies + k of Y (row stride y_ld >= width: Y may be a column block of a wider buffer, the other columns are not touched):
 *     Y[c copies + k, j] = act(bn(fma(alpha[k], P[c, j], bias[j])))     bn(x) = (x - mean[j]) * (1 / sqrt(var[j] + eps)) * gamma[j] + beta[j]
 *   in fp32, the operation order of kgcn_graph_bn_apply_act_f32, so that a copy with alpha == 1 equals that pass applied to
 *   P + bias bit for bit.  (With scale = gamma / sqrt(var + eps) and shift = beta - scale mean this is act(scale (alpha P + bias) +
 *   shift); the entry point takes the layer's own four vectors because the folded form rounds differently.)  bias may be NULL
 *   (zeros); gamma, beta, mean, var are all NULL (no normalisation) or all given.
 * reduce: dY and Y [compounds copies, width] with row strides dy_ld, y_ld >= width, w [copies], scale [width] or NULL (ones):
 *     S[c, j] = scale[j] sum_k w[k] dY[c copies + k, j] act'(Y[c copies + k, j])        S [compounds, width] contiguous
 *   -- the weighted sum over the copies of d score / d pre-activation.  The sum runs over k = 0, 1, ... in that order in fp32 in
 *   one register (acc = fma(w[k], dY act'(Y), acc)) without atomics; a copy with w[k] == 0 is skipped: whatever its rows hold, NaN
 *   included, never reaches the sum (the rows themselves must exist).
 * Both: act is a KGCN_ACT_* code; a compound's rows do not depend on the other compounds of the call (chunking changes no bit);
 * 16-byte accesses when the base pointers are 16-byte aligned and width and the row strides are multiples of 4, single floats
 * otherwise; each output element is written once, Y and dY are read once.  compounds == 0 is a no-op.
 * Limits: 1 <= width <= KGCN_IG_COPIES_MAX_WIDTH, 1 <= copies <= KGCN_IG_COPIES_MAX_COPIES, compounds >= 0 with compounds copies <=
 * KGCN_IG_COPIES_MAX_ROWS and a grid below 2^31 workgroups (pass fewer compounds); anything else is refused before any launch.
 * Asynchronous. */
enum { KGCN_IG_COPIES_MAX_WIDTH = 1 << 20, KGCN_IG_COPIES_MAX_COPIES = 65535, KGCN_IG_COPIES_MAX_ROWS = 0x7fffffff };
int kgcn_ig_copies_expand_f32(const float* P, int64_t compounds, int32_t copies, int32_t width, const float* alpha, const float* bias,
                              const float* gamma, const float* beta, const float* mean, const float* var, float eps, int32_t act,
                              float* Y, int64_t y_ld, void* stream);
int kgcn_ig_copies_reduce_f32(const float* dY, int64_t dy_ld, const float* Y, int64_t y_ld, int64_t compounds, int32_t copies,
                              int32_t width, const float* w, const float* scale, int32_t act, float* S, void* stream);

/* Integrated gradients of the protein-sequence CNN (kgcn visualize on sample_protein/sequence/cnn.py; kgcn/visualization.py:187-260):
 * the sweeps over the `copies` scaled copies of `proteins` proteins through the model's first layer, Conv1D(filters, k, same, relu)
 * -> MaxPooling1D(pool) (csrc/convig.hip; entry points only, version still 2; named kgcn_ig_conv1d_* beside kgcn_ig_copies_*, the
 * kgcn_conv1d_* prefix being the layer's own set of entry points).  Copy k feeds alpha[k] e, alpha[k] >= 0, so its
 * pre-activation is alpha[k] P + bias with P = conv(e) without the bias, and p -> relu(fl(fl(alpha p) + b)) is non-decreasing:
 * the window maximum commutes with it, also after fp32 rounding.  The caller forms Pm [proteins, positions, filters] = the
 * window maxima of P and their arg-max ONCE per protein with kgcn_conv1d_pool_fwd_f32 (zero bias, KGCN_ACT_NONE).
 * expand: out [proteins copies, positions, filters], copy k of protein c in row c copies + k:
 *     v = fl(fl(alpha[k] * Pm[c, t, f]) + bias[f]);  out[c copies + k, t, f] = v > 0 ? v : +0
 *   -- two roundings, the product is NOT fused into the sum.  kgcn_conv1d_pool_fwd_f32 adds its bias AFTER the accumulation
 *   (act(acc + bias), csrc/conv1d.hip), so at alpha[k] == 1 the row is bit for bit the first layer that kernel computes from e.
 * reduce: dout (the gradient arriving at `out`) and out as above, w [copies] -> r [proteins, positions, filters] contiguous:
 *     acc = +0;  for k = 0, 1, ..: if w[k] != 0 and out[c copies + k, t, f] > 0: acc = fl(acc + fl(w[k] * dout[c copies + k, t, f]))
 *   in that order, unfused, without atomics.  A copy with w[k] == 0 is neither read nor added (its rows must exist; NaN there
 *   never reaches the sum).  One kgcn_conv1d_pool_bwd_f32 (KGCN_ACT_NONE, dout = r, the arg-max and out of the Pm pass, dx only)
 *   then gives sum_k w[k] d score_k / d (alpha[k] e), because conv is linear.
 * Deviation from the per-copy route: where two candidates of a window of P differ but their scaled, biased values round to the same
 * positive fp32 number, the per-copy kernel routes the gradient to the lowest index among the equal values and this route to the
 * arg-max of P -- the one exact arithmetic picks.  (Where both are cut to 0 by the relu no gradient flows on either route.)
 * Both: a protein's rows do not depend on the other proteins of the call (chunking changes no bit); bitwise reproducible; the
 * accesses are 16 bytes wide along (t, f) and 4-byte aligned, the last n mod 4 floats of a row (n = positions filters) go float by
 * float, nothing past a row is touched.  proteins == 0 is a no-op.  Scales are checked by the caller (kgcn_amd.ops refuses a
 * negative or non-finite one before any launch).
 * Limits: positions <= KGCN_CONV1D_MAX_LENGTH, filters <= KGCN_CONV1D_MAX_CHANNELS, 1 <= copies <= KGCN_CONV1D_IG_MAX_COPIES,
 * proteins copies < 2^31 and a grid below 2^31 workgroups (pass fewer proteins); anything else is refused before any launch.
 * Asynchronous. */
enum { KGCN_CONV1D_IG_MAX_COPIES = 1024 };
int kgcn_ig_conv1d_expand_f32(const float* Pm, int64_t proteins, int32_t copies, int32_t positions, int32_t filters,
                              const float* alpha, const float* bias, float* out, void* stream);
int kgcn_ig_conv1d_reduce_f32(const float* dout, const float* out, int64_t proteins, int32_t copies, int32_t positions,
                              int32_t filters, const float* w, float* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KGCN_HIP_H_ */
