// General Conv1D(F, k, padding="same", activation) -> MaxPooling1D(pool) on the fp32 matrix pipe: the layer stack of
// sample_protein/sequence/cnn.py:36-79 (Embedding -> three conv-pool layers -> Conv1D(1, 2, tanh)).
//
//   forward   implicit GEMM, v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns kRows = 64 conv positions of ONE sequence and
//             kCols = 64 filters; wave (rb, cb) owns the 32 x 32 block (rows rb, columns cb).  The reduction runs over
//             (Cin chunk of 32, tap): per chunk the kRows + k - 1 input rows are staged in LDS ONCE ([row][33]: conflict-free
//             for the A operand, lane l reads row l & 31, column 2 s + (l >> 5)) and the k taps read them at row offsets
//             0 .. k-1; the chunk of W [k][32][64] lies beside them (odd reduction rows with their two 32-column halves
//             swapped, so the two lane halves of the B operand hit disjoint banks).  A tile starts at a multiple of
//             (64 / pool) pool positions, so it holds whole pool windows: bias, activation and the window maximum are formed
//             in the epilogue from an LDS copy of the 64 x 64 block and only the pooled [B, L / pool, F] tensor is written
//             (plus one arg-max byte per output when a gradient will be needed: the lowest index among equal maxima).
//             The input rows are x [B, L, Cin] or, in token mode, table[tokens[b, l]] (the embedded tensor is never written).
//   backward  G = d pooled routed through the arg-max bytes times the activation's derivative (a function of the output) is never
//             written either: it is formed while it is staged.
//             dX [B, L, Cin] is the same implicit GEMM over G with the taps reversed and W transposed (a small kernel writes
//             that copy of W into the workspace): dX[m] = sum_dk' G[m - (k - 1 - padL) + dk'] Wt[dk'], no bias, no pooling.
//             dW[dk] = sum_(b, l) x[b, l - padL + dk]^T G[b, l]: workgroup (64 channels, 64 filters, tap dk, part), 64 positions
//             per LDS stage, the parts are fixed contiguous ranges of (sequence, position chunk) walked in order; dbias is the
//             column sum of the same staged G (the dk = 0, first-channel-tile workgroups).  The partials go through
//             reduce_or_defer: fixed order, no float atomics, bitwise reproducible, deferrable (kgcn_reduce_defer).
//   embedding gradient  d table[s] = sum over the positions holding symbol s of d embedded, one workgroup per (symbol, 32 columns),
//             8 position classes mod 8 summed in order, then added in class order.
// Precision: plain fp32 MFMA (an exact k-ordered fmaf chain), as dense.hip; the split-bf16 product of gemmh.hip would need the
// staged window split per tap or held three times in LDS, and the model's widest reduction (3 x 505) is small.
#include "workspace.h"

namespace kgcn {

namespace {
constexpr int kRows = 64;      // conv positions per workgroup tile
constexpr int kCols = 64;      // output columns per workgroup tile
constexpr int kChunk = 32;     // reduction columns per LDS stage
constexpr int kLdx = kChunk + 1;
constexpr int kLde = kCols + 1;
constexpr int kMaxParts = 64;  // weight-gradient partials

enum { kSrcDense = 0, kSrcTokens = 1, kSrcGrad = 2 };

struct ConvArgs {
  const float* x;        // dense rows [B, L, K]
  const int32_t* tok;    // token mode: rows are table[tok[b, l]]
  const float* table;
  const float* dout;     // routed-gradient rows: d pooled, arg-max bytes and pooled output [B, T, K]
  const uint8_t* arg;
  const float* y;
  const float* w;        // [k][K][N]
  const float* bias;     // [N] or NULL
  int B, L, S, K, N, k, pool, pad;
  int act;               // the LAYER's activation (derivative of the routed gradient)
  int eact;              // activation of this product's epilogue
  int T;                 // pooled positions of the layer, L / pool of the LAYER (the routed gradient lives on [0, T pool))
  int gpool;             // pool of the layer (routing); `pool` is this product's epilogue pool
  int To;                // output rows per sequence of this product
  int rows_per_tile, tiles_per_seq;
};

// element (position l, column c) of the operand rows of sequence b; 0 outside the sequence
template <int kSrc>
__device__ __forceinline__ float src_value(const ConvArgs& a, int b, int l, int c) {
  if (kSrc == kSrcGrad) {
    if (l < 0 || l >= a.T * a.gpool) return 0.f;
    const int t = l / a.gpool, j = l - t * a.gpool;
    const long o = ((long)b * a.T + t) * a.K + c;
    return a.arg[o] == j ? a.dout[o] * act_dout(a.y[o], a.act) : 0.f;
  }
  if (l < 0 || l >= a.L) return 0.f;
  if (kSrc == kSrcTokens) {
    const int s = a.tok[(long)b * a.L + l];
    return (s >= 0 && s < a.S) ? a.table[(long)s * a.K + c] : 0.f;
  }
  return a.x[((long)b * a.L + l) * a.K + c];
}

template <int kSrc>
__global__ __launch_bounds__(256) void conv1d_gemm_kernel(ConvArgs a, float* __restrict__ out, uint8_t* __restrict__ argmax) {
  extern __shared__ float lds[];
  const int nrows = kRows + a.k - 1;
  float* xs = lds;                       // [nrows][kLdx]
  float* ws = xs + nrows * kLdx;         // [k][kChunk][kCols], odd rows with their halves swapped
  float* ep = lds;                       // [kRows][kLde], after the reduction
  const int b = blockIdx.x / a.tiles_per_seq, tile = blockIdx.x - b * a.tiles_per_seq;
  const int l0 = tile * a.rows_per_tile, n0 = blockIdx.y * kCols;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
  const int rb = wv & 1, cb = wv >> 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int c0 = 0; c0 < a.K; c0 += kChunk) {
    __syncthreads();                     // the previous chunk is no longer read
    for (int i = threadIdx.x; i < nrows * kChunk; i += 256) {
      const int r = i >> 5, cc = i & 31;
      xs[r * kLdx + cc] = c0 + cc < a.K ? src_value<kSrc>(a, b, l0 - a.pad + r, c0 + cc) : 0.f;
    }
    for (int i = threadIdx.x; i < a.k * kChunk * kCols; i += 256) {
      const int n = i & 63, kk = (i >> 6) & 31, dk = i >> 11;
      const float v = (c0 + kk < a.K && n0 + n < a.N) ? a.w[((long)dk * a.K + c0 + kk) * a.N + n0 + n] : 0.f;
      ws[(dk * kChunk + kk) * kCols + (n ^ ((kk & 1) << 5))] = v;
    }
    __syncthreads();
    for (int dk = 0; dk < a.k; ++dk) {
      const float* xa = xs + (rb * 32 + li + dk) * kLdx + hi;
      const float* wb = ws + (dk * kChunk + hi) * kCols + ((cb * 32 + li) ^ (hi << 5));
#pragma unroll
      for (int s = 0; s < kChunk / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], wb[2 * s * kCols], acc, 0, 0, 0);
    }
  }
  __syncthreads();                       // xs / ws are dead: the block goes to LDS for the window maximum
  {
    const int col = cb * 32 + li;
    const float bf = (a.bias && n0 + col < a.N) ? a.bias[n0 + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ep[row * kLde + col] = act_fwd(acc[r] + bf, a.eact);
    }
  }
  __syncthreads();
  const int nwin = a.rows_per_tile / a.pool, t0 = l0 / a.pool;
  for (int i = threadIdx.x; i < nwin * kCols; i += 256) {
    const int wdw = i >> 6, f = i & 63, t = t0 + wdw;
    if (t >= a.To || n0 + f >= a.N) continue;
    const float* e = ep + wdw * a.pool * kLde + f;
    float m = e[0];
    int am = 0;
    for (int j = 1; j < a.pool; ++j) {
      const float v = e[j * kLde];
      if (v > m) { m = v; am = j; }
    }
    const long o = ((long)b * a.To + t) * a.N + n0 + f;
    out[o] = m;
    if (argmax) argmax[o] = (uint8_t)am;
  }
}

// wt[dk][f][c] = w[k - 1 - dk][c][f]
__global__ __launch_bounds__(256) void conv1d_flip_kernel(const float* __restrict__ w, int k, int Cin, int F, float* __restrict__ wt) {
  __shared__ float t[32][33];
  const int dk = blockIdx.z, c0 = blockIdx.y * 32, f0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    t[r][tx] = (c0 + r < Cin && f0 + tx < F) ? w[((long)(k - 1 - dk) * Cin + c0 + r) * F + f0 + tx] : 0.f;
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (f0 + r < F && c0 + tx < Cin) wt[((long)dk * F + f0 + r) * Cin + c0 + tx] = t[tx][r];
}

struct WgradArgs {
  ConvArgs c;            // K = F (the routed gradient's width); x / tok / table rows are Cin wide
  int Cin, ctiles, cps;  // cps: position chunks per sequence
  long total, per;       // (sequence, chunk) pairs, pairs per part
};

// rows of x for the weight gradient: dense or token mode (kSrcGrad rows use c.K = F, these use Cin)
template <int kSrc>
__device__ __forceinline__ float x_value(const WgradArgs& g, int b, int l, int c) {
  const ConvArgs& a = g.c;
  if (l < 0 || l >= a.L) return 0.f;
  if (kSrc == kSrcTokens) {
    const int s = a.tok[(long)b * a.L + l];
    return (s >= 0 && s < a.S) ? a.table[(long)s * g.Cin + c] : 0.f;
  }
  return a.x[((long)b * a.L + l) * g.Cin + c];
}

template <int kSrc>
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(WgradArgs g, float* __restrict__ part_w, float* __restrict__ part_b) {
  __shared__ float xs[kRows * kCols];    // [position][channel], odd rows with their halves swapped
  __shared__ float gs[kRows * kCols];    // [position][filter], likewise
  const ConvArgs& a = g.c;
  const int F = a.K, Cin = g.Cin;
  const int ct = blockIdx.x % g.ctiles, ft = blockIdx.x / g.ctiles, part = blockIdx.y, dk = blockIdx.z;
  const int c0 = ct * kCols, f0 = ft * kCols;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
  const int cb = wv & 1, fb = wv >> 1;
  const bool live = c0 + cb * 32 < Cin && f0 + fb * 32 < F;     // wave-uniform
  const bool bias_wg = dk == 0 && ct == 0 && threadIdx.x < kCols;
  const int TP = a.T * a.gpool;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float accb = 0.f;
  const long q0 = part * g.per, q1 = q0 + g.per < g.total ? q0 + g.per : g.total;
  for (long q = q0; q < q1; ++q) {
    const int b = (int)(q / g.cps), l0 = (int)(q - (long)b * g.cps) * kRows;
    __syncthreads();
    for (int i = threadIdx.x; i < kRows * kCols; i += 256) {
      const int r = i >> 6, c = i & 63, l = l0 + r;
      const int sw = r * kCols + (c ^ ((r & 1) << 5));
      xs[sw] = (l < TP && c0 + c < Cin) ? x_value<kSrc>(g, b, l - a.pad + dk, c0 + c) : 0.f;
      gs[sw] = f0 + c < F ? src_value<kSrcGrad>(a, b, l, f0 + c) : 0.f;
    }
    __syncthreads();
    if (live) {
      const float* xa = xs + hi * kCols + ((cb * 32 + li) ^ (hi << 5));
      const float* ga = gs + hi * kCols + ((fb * 32 + li) ^ (hi << 5));
#pragma unroll 8
      for (int s = 0; s < kRows / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s * kCols], ga[2 * s * kCols], acc, 0, 0, 0);
    }
    if (bias_wg) {
      for (int r = 0; r < kRows; ++r) accb += gs[r * kCols + ((int)threadIdx.x ^ ((r & 1) << 5))];
    }
  }
  if (live) {
    const int f = f0 + fb * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (c < Cin && f < F) part_w[((long)part * a.k + dk) * Cin * F + (long)c * F + f] = acc[r];
    }
  }
  if (bias_wg && f0 + (int)threadIdx.x < F) part_b[(long)part * F + f0 + threadIdx.x] = accb;
}

// d table[s, e] = sum over positions i (in order within each class i mod 8, classes added in order) with tok[i] == s of d[i, e]
__global__ __launch_bounds__(256) void embedding_grad_kernel(const int32_t* __restrict__ tok, long n, const float* __restrict__ d,
                                                             int E, float* __restrict__ dtable) {
  __shared__ float part[8][32];
  const int s = blockIdx.x, e = blockIdx.y * 32 + (threadIdx.x & 31), grp = threadIdx.x >> 5;
  float acc = 0.f;
  if (e < E)
    for (long i = grp; i < n; i += 8)
      if (tok[i] == s) acc += d[i * E + e];
  part[grp][threadIdx.x & 31] = acc;
  __syncthreads();
  if (grp == 0 && e < E) {
    float v = part[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < 8; ++q) v += part[q][threadIdx.x];
    dtable[(long)s * E + e] = v;
  }
}

int conv_check(int32_t B, int32_t L, int32_t Cin, int32_t k, int32_t F, int32_t pool, int32_t act, const char* who) {
  if (B < 0) return fail("%s: batch %d", who, B);
  if (L < 1 || L > KGCN_CONV1D_MAX_LENGTH) return fail("%s: length %d outside 1..%d", who, L, KGCN_CONV1D_MAX_LENGTH);
  if (Cin < 1 || Cin > KGCN_CONV1D_MAX_CHANNELS) return fail("%s: input width %d outside 1..%d", who, Cin, KGCN_CONV1D_MAX_CHANNELS);
  if (F < 1 || F > KGCN_CONV1D_MAX_CHANNELS) return fail("%s: %d filters outside 1..%d", who, F, KGCN_CONV1D_MAX_CHANNELS);
  if (k < 1 || k > KGCN_CONV1D_MAX_KERNEL) return fail("%s: kernel size %d outside 1..%d", who, k, KGCN_CONV1D_MAX_KERNEL);
  if (pool < 1 || pool > KGCN_CONV1D_MAX_POOL) return fail("%s: pool size %d outside 1..%d", who, pool, KGCN_CONV1D_MAX_POOL);
  if (act != KGCN_ACT_NONE && act != KGCN_ACT_RELU && act != KGCN_ACT_TANH) return fail("%s: activation code %d", who, act);
  if ((int64_t)B * L * (Cin > F ? Cin : F) >= (int64_t)INT32_MAX * 16) return fail("%s: batch x length x width too large", who);
  if ((int64_t)B * ((L + kRows - 1) / kRows + 1) >= (int64_t)INT32_MAX) return fail("%s: too many position tiles", who);
  return 0;
}

// rows come from x, or from (tokens, table) when x is NULL
int source_check(const float* x, const int32_t* tokens, const float* table, int32_t S, const char* who) {
  if (x) {
    if (tokens || table) return fail("%s: both a dense input and a token input", who);
    return 0;
  }
  if (!tokens || !table) return fail("%s: NULL input", who);
  if (S < 1 || S > KGCN_CONV1D_MAX_SYMBOLS) return fail("%s: %d symbols outside 1..%d", who, S, KGCN_CONV1D_MAX_SYMBOLS);
  return 0;
}

size_t gemm_lds(int k) {
  const size_t stage = ((size_t)(kRows + k - 1) * kLdx + (size_t)k * kChunk * kCols) * 4, epi = (size_t)kRows * kLde * 4;
  return stage > epi ? stage : epi;
}

template <int kSrc>
int launch_gemm(const ConvArgs& a, float* out, uint8_t* argmax, hipStream_t s, const char* what) {
  const size_t lds = gemm_lds(a.k);
  if (int rc = allow_full_lds<conv1d_gemm_kernel<kSrc>>(lds, what)) return rc;
  hipLaunchKernelGGL(conv1d_gemm_kernel<kSrc>, dim3((unsigned)(a.B * a.tiles_per_seq), (unsigned)((a.N + kCols - 1) / kCols)),
                     dim3(256), lds, s, a, out, argmax);
  return check_launch(what);
}

int wgrad_parts(int32_t B, int32_t L, int32_t Cin, int32_t k, int32_t F, int32_t pool) {
  const long tiles = (long)((Cin + kCols - 1) / kCols) * ((F + kCols - 1) / kCols) * k;
  const long total = (long)(B > 0 ? B : 0) * ((L / pool * pool + kRows - 1) / kRows);
  long parts = (1024 + tiles - 1) / tiles;
  if (parts > kMaxParts) parts = kMaxParts;
  if (parts > total) parts = total;
  return parts < 1 ? 1 : (int)parts;
}

// the flipped weights wt [k, F, Cin] | `parts` partials of d w [k, Cin, F] | `parts` partials of d bias [F]
struct BwdWorkspace { int parts; long nw; float *wt, *part_w, *part_b; size_t bytes; };
BwdWorkspace bwd_layout(void* base, int32_t batch, int32_t length, int32_t in_dim, int32_t kernel_size, int32_t filters, int32_t pool) {
  Taker t(base, 4);
  BwdWorkspace w;
  w.parts = wgrad_parts(batch, length, in_dim, kernel_size, filters, pool);
  w.nw = (long)kernel_size * in_dim * filters;
  w.wt = t.take<float>((size_t)w.nw);
  w.part_w = t.take<float>((size_t)w.parts * w.nw);
  w.part_b = t.take<float>((size_t)w.parts * filters);
  w.bytes = t.off;
  return w;
}
}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_conv1d_pool_workspace_bytes(int32_t batch, int32_t length, int32_t in_dim, int32_t kernel_size,
                                                    int32_t filters, int32_t pool) {
  if (conv_check(batch, length, in_dim, kernel_size, filters, pool, KGCN_ACT_NONE, "kgcn_conv1d_pool_workspace_bytes")) return -1;
  return (int64_t)bwd_layout(nullptr, batch, length, in_dim, kernel_size, filters, pool).bytes;
}

extern "C" int kgcn_conv1d_pool_fwd_f32(const float* x, const int32_t* tokens, const float* table, int32_t symbols, int32_t batch,
                                        int32_t length, int32_t in_dim, const float* w, const float* bias, int32_t kernel_size,
                                        int32_t filters, int32_t pool, int32_t act, float* out, uint8_t* argmax, void* stream) {
  const char* who = "kgcn_conv1d_pool_fwd_f32";
  if (int rc = conv_check(batch, length, in_dim, kernel_size, filters, pool, act, who)) return rc;
  const int T = length / pool;
  if (batch == 0 || T == 0) return 0;
  if (int rc = source_check(x, tokens, table, symbols, who)) return rc;
  if (!w || !bias || !out) return fail("%s: NULL operand", who);
  ConvArgs a = {};
  a.x = x; a.tok = tokens; a.table = table; a.w = w; a.bias = bias;
  a.B = batch; a.L = length; a.S = symbols; a.K = in_dim; a.N = filters; a.k = kernel_size; a.pool = pool; a.gpool = pool;
  a.act = act; a.eact = act; a.pad = (kernel_size - 1) / 2; a.T = T; a.To = T;
  a.rows_per_tile = kRows / pool * pool;
  a.tiles_per_seq = (T * pool + a.rows_per_tile - 1) / a.rows_per_tile;
  return x ? launch_gemm<kSrcDense>(a, out, argmax, as_stream(stream), "conv1d_gemm_kernel<dense>")
           : launch_gemm<kSrcTokens>(a, out, argmax, as_stream(stream), "conv1d_gemm_kernel<tokens>");
}

extern "C" int kgcn_conv1d_pool_bwd_f32(const float* x, const int32_t* tokens, const float* table, int32_t symbols, int32_t batch,
                                        int32_t length, int32_t in_dim, const float* w, int32_t kernel_size, int32_t filters,
                                        int32_t pool, int32_t act, const float* dout, const uint8_t* argmax, const float* out,
                                        float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const char* who = "kgcn_conv1d_pool_bwd_f32";
  if (int rc = conv_check(batch, length, in_dim, kernel_size, filters, pool, act, who)) return rc;
  if (!dw != !dbias) return fail("%s: d w and d bias are formed together", who);
  if (!dw && !dx) return 0;
  const int T = length / pool;
  const bool any = batch > 0 && T > 0;
  if (batch > 0)
    if (int rc = source_check(x, tokens, table, symbols, who)) return rc;
  if (any && (!dout || !argmax || !out || !w)) return fail("%s: NULL operand", who);
  const BwdWorkspace ws = bwd_layout(workspace, batch, length, in_dim, kernel_size, filters, pool);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)ws.bytes)) return rc;
  hipStream_t s = as_stream(stream);
  const int parts = ws.parts;
  float *wt = ws.wt, *part_w = ws.part_w, *part_b = ws.part_b;
  ConvArgs a = {};
  a.x = x; a.tok = tokens; a.table = table; a.dout = dout; a.arg = argmax; a.y = out;
  a.B = batch; a.L = length; a.S = symbols; a.K = filters; a.k = kernel_size; a.gpool = pool; a.act = act; a.T = T;
  if (!any) {                                        // no pooled output: zero gradients
    if (int rc = zero_async(who, part_w, (size_t)parts * (ws.nw + filters) * 4, s)) return rc;   // part_w | part_b
    if (dx && batch > 0)
      if (int rc = zero_async(who, dx, (size_t)batch * length * in_dim * 4, s)) return rc;
  } else {
    if (dx) {
      hipLaunchKernelGGL(conv1d_flip_kernel, dim3((filters + 31) / 32, (in_dim + 31) / 32, kernel_size), dim3(256), 0, s, w,
                         kernel_size, in_dim, filters, wt);
      if (int rc = check_launch("conv1d_flip_kernel")) return rc;
      ConvArgs d = a;
      d.w = wt; d.bias = nullptr; d.eact = KGCN_ACT_NONE; d.N = in_dim; d.pool = 1; d.pad = kernel_size - 1 - (kernel_size - 1) / 2; d.To = length;
      d.rows_per_tile = kRows; d.tiles_per_seq = (length + kRows - 1) / kRows;
      if (int rc = launch_gemm<kSrcGrad>(d, dx, nullptr, s, "conv1d_gemm_kernel<grad>")) return rc;
    }
    if (!dw) return 0;
    WgradArgs g = {};
    g.c = a; g.c.pad = (kernel_size - 1) / 2;
    g.Cin = in_dim; g.ctiles = (in_dim + kCols - 1) / kCols; g.cps = (T * pool + kRows - 1) / kRows;
    g.total = (long)batch * g.cps; g.per = (g.total + parts - 1) / parts;
    const dim3 grid((unsigned)(g.ctiles * ((filters + kCols - 1) / kCols)), (unsigned)parts, (unsigned)kernel_size);
    if (x) hipLaunchKernelGGL(conv1d_wgrad_kernel<kSrcDense>, grid, dim3(256), 0, s, g, part_w, part_b);
    else hipLaunchKernelGGL(conv1d_wgrad_kernel<kSrcTokens>, grid, dim3(256), 0, s, g, part_w, part_b);
    if (int rc = check_launch("conv1d_wgrad_kernel")) return rc;
  }
  if (!dw) return 0;
  if (int rc = reduce_or_defer(part_w, parts, ws.nw, dw, s)) return rc;
  return reduce_or_defer(part_b, parts, filters, dbias, s);
}

extern "C" int kgcn_embedding_grad_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* dembedded,
                                       int32_t symbols, int32_t embed_dim, float* dtable, void* stream) {
  const char* who = "kgcn_embedding_grad_f32";
  if (batch < 0 || length < 0 || length > KGCN_CONV1D_MAX_LENGTH) return fail("%s: bad batch %d x length %d", who, batch, length);
  if (symbols < 1 || symbols > KGCN_CONV1D_MAX_SYMBOLS) return fail("%s: %d symbols outside 1..%d", who, symbols, KGCN_CONV1D_MAX_SYMBOLS);
  if (embed_dim < 1 || embed_dim > KGCN_CONV1D_MAX_CHANNELS)
    return fail("%s: embedding width %d outside 1..%d", who, embed_dim, KGCN_CONV1D_MAX_CHANNELS);
  const long n = (long)batch * length;
  if (!dtable || (n > 0 && (!tokens || !dembedded))) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(embedding_grad_kernel, dim3((unsigned)symbols, (unsigned)((embed_dim + 31) / 32)), dim3(256), 0,
                     as_stream(stream), tokens, n, dembedded, embed_dim, dtable);
  return check_launch("embedding_grad_kernel");
}
