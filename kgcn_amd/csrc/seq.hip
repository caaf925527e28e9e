// Protein-sequence encoder of example_model/model_multimodal.py:70-93:
//   Embedding(S, E) -> Conv1D(F, k, padding="same", relu) -> MaxPooling1D(p) -> LSTM(H, go_backwards=True) -> h after step 0
//
//   conv-pool  one pass: the embedding rows of a window of tokens are gathered into LDS, the conv, bias, relu and the max over
//              each pool window are formed in registers; neither the [B, L, E] embedding nor the [B, L, F] conv output is
//              written.  SAME padding at stride 1: (k-1)/2 positions on the left, the rest on the right.  Training writes the
//              arg-max of every pooled output as a byte (the lowest index among equal maxima; 0xFF when the maximum is not > 0,
//              i.e. relu passes no gradient).  The backward routes d pooled to that position, forms d W / d bias and the
//              per-position embedding gradient, and adds the latter into a per-workgroup [S, E] table (each table row is owned
//              by one thread group, visited in position order): fixed-order partials, fixed-order second stage.
//   LSTM       Keras v1 cell, gate order i, f, c, o; recurrent activation hard_sigmoid clip(0.2 z + 0.5, 0, 1) (or sigmoid),
//              tanh elsewhere, zero initial state, the steps of the padded sequence last to first, no masking.  One workgroup
//              owns 256 / H' sequences (H' = H rounded up to 16 / 32 / 64) for all steps; one thread per (sequence, unit)
//              forms the four gate pre-activations from [x_t | h] against [W_x ; W_h] held in LDS (fp32 FMAs).  Training
//              writes the BPTT stash: z (the 4H pre-activations), h and c of every step, 6H floats per sequence and step.
//              The backward walks the steps in reverse processing order, writes dX and overwrites z with dz; a third kernel
//              forms d W_x, d W_h, d bias from [x_t | h_prev | 1]^T dz in per-workgroup partials (fixed-order second stage).
//   IG         integrated gradients of the multimodal model (kgcn/visualization.py:187-231 with the embedded sequence fed in):
//              the scaled forward is the conv-pool with batch row b reading token row b / rep and its embedding rows times
//              scale[b]; the input gradient routes d pooled through the arg-max bytes and forms the gradient with respect to the
//              scaled embedded input, summed over the rep copies of every compound with per-row weights, optionally times the
//              embedding row (the attribution itself).  It forms no weight gradient.  The smooth methods (:235-259) add noise to
//              the embedded input: a third staging mode draws sigma[b] * N(0, 1) per window element from a counter-based
//              stream keyed by (seed, compound, sample, position, column), so the noisy input is never written either.
// Every second stage is a parameter gradient and goes through reduce_or_defer (kgcn_reduce_defer).  No float atomics: results
// are bitwise reproducible.
#include "workspace.h"
#include "philox.h"

namespace kgcn {

namespace {
constexpr int kTile = 16;                 // pooled positions per conv-pool tile (4 per wave)
constexpr int kConvGridFwd = 2048;
constexpr int kConvGridBwd = 512;
constexpr int kLstmChunks = 256;          // row chunks of the LSTM weight-gradient kernel

__host__ __device__ __forceinline__ int round4(int x) { return (x + 3) & ~3; }

struct ConvArgs {
  const int32_t* tok;
  const float* table;
  const float* w;       // [k, E, F]
  int B, L, S, E, E4, F, k, p, padL, T;   // T = L / p pooled positions
  long tiles;           // B * ceil(T / kTile)
  const float* scale;   // [B] per-row factor of the gathered embedding (scaled forward only)
  int rep;              // batch row b reads token row b / rep (scaled forward and input gradient; 1 otherwise)
  const float* sigma;   // [B] noise scale of the row (perturbed forward only, as the next three)
  const int32_t* sample;   // [B] sample number k of the row
  const int32_t* ids;   // [B / rep] dataset index g of the token row
  uint64_t seed;
};

// window of conv-input rows of tile (b, t0): rows r = 0 .. nrows-1 are sequence positions l = t0 p - padL + r.  kStageScaled: row b
// reads token row b / rep and its embedding rows times scale[b] (the scaled [B, L, E] input is never written).  kStagePerturbed:
// the same plus sigma[b] times the attribution noise of stream KGCN_IG_STREAM_SEQUENCE (philox.h), keyed by the ABSOLUTE
// position l (row l of the [L, E] array), so neighbouring tiles regenerate identical halo rows; padding positions and the
// columns e >= E stay exactly 0, and a row with sigma[b] == 0 takes the scaled expression and draws nothing
enum { kStagePlain = 0, kStageScaled = 1, kStagePerturbed = 2 };
template <int kMode = kStagePlain>
__device__ __forceinline__ void stage_window(const ConvArgs& a, int b, int t0, int nrows, float* win, int* twin) {
  constexpr bool kScaled = kMode != kStagePlain;
  const int l0 = t0 * a.p - a.padL;
  const long trow = kScaled ? (long)(b / a.rep) : (long)b;
  for (int i = threadIdx.x; i < nrows; i += blockDim.x) {
    const int l = l0 + i;
    twin[i] = (l >= 0 && l < a.L) ? a.tok[trow * a.L + l] : -1;
  }
  __syncthreads();
  const float sc = kScaled ? a.scale[b] : 1.f;
  if constexpr (kMode == kStagePerturbed) {
    const float sg = a.sigma[b];
    if (sg != 0.f) {                             // uniform over the workgroup
      const int E4q = a.E4 >> 2;                 // Philox blocks per row = ceil(E / 4)
      const uint32_t g = (uint32_t)a.ids[trow], smp = (uint32_t)a.sample[b];
      for (int i = threadIdx.x; i < nrows * E4q; i += blockDim.x) {
        const int r = i / E4q, q = i - r * E4q;
        const int s = twin[r];
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0) {
          float z[4];
          ig_noise4(a.seed, KGCN_IG_STREAM_SEQUENCE, g, smp, (uint64_t)((long)(l0 + r) * E4q + q), z);
          const float* tp = a.table + (long)s * a.E;
          const int e = 4 * q;
          o.x = fmaf(sg, z[0], tp[e] * sc);
          if (e + 1 < a.E) o.y = fmaf(sg, z[1], tp[e + 1] * sc);
          if (e + 2 < a.E) o.z = fmaf(sg, z[2], tp[e + 2] * sc);
          if (e + 3 < a.E) o.w = fmaf(sg, z[3], tp[e + 3] * sc);
        }
        *reinterpret_cast<f32x4*>(win + r * a.E4 + 4 * q) = o;
      }
      return;
    }
  }
  for (int i = threadIdx.x; i < nrows * a.E4; i += blockDim.x) {
    const int r = i / a.E4, e = i - r * a.E4;
    const int s = twin[r];
    const float x = (s >= 0 && e < a.E) ? a.table[(long)s * a.E + e] : 0.f;
    win[i] = kScaled ? x * sc : x;
  }
}

// lane = filter f (< 64), wave = 4 pooled positions of the tile; acc[i][j] = conv at position (t0 + 4 wave + i) p + j
template <int kMode>
__global__ __launch_bounds__(256) void convpool_fwd_kernel(ConvArgs a, const float* __restrict__ bias, float* __restrict__ out,
                                                           uint8_t* __restrict__ argmax) {
  extern __shared__ float lds[];
  const int KE4 = a.k * a.E4;
  float* ws = lds;                              // [k * E4][64]
  float* win = ws + KE4 * 64;                   // [kTile p + k - 1][E4]
  int* twin = reinterpret_cast<int*>(win + (kTile * a.p + a.k - 1) * a.E4);
  for (int i = threadIdx.x; i < KE4 * 64; i += blockDim.x) {
    const int r = i >> 6, f = i & 63, dk = r / a.E4, e = r - dk * a.E4;
    ws[i] = (f < a.F && e < a.E) ? a.w[((long)dk * a.E + e) * a.F + f] : 0.f;
  }
  const int f = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float bf = f < a.F ? bias[f] : 0.f;
  const int tpb = (a.T + kTile - 1) / kTile;
  const int nrows = kTile * a.p + a.k - 1;
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int b = (int)(tile / tpb), t0 = (int)(tile - (long)b * tpb) * kTile;
    __syncthreads();                            // the previous tile's window is no longer read
    stage_window<kMode>(a, b, t0, nrows, win, twin);
    __syncthreads();
    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int dk = 0; dk < a.k; ++dk) {
      for (int e = 0; e < a.E4; e += 4) {
        const float* wp = ws + (dk * a.E4 + e) * 64 + f;
        const float w0 = wp[0], w1 = wp[64], w2 = wp[128], w3 = wp[192];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j < a.p) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(win + ((wv * 4 + i) * a.p + j + dk) * a.E4 + e);
              acc[i][j] = fmaf(x.x, w0, fmaf(x.y, w1, fmaf(x.z, w2, fmaf(x.w, w3, acc[i][j]))));
            }
          }
        }
      }
    }
    if (f < a.F) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + wv * 4 + i;
        if (t >= a.T) continue;
        float m = -1.f;
        int arg = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j < a.p) {
            const float v = fmaxf(acc[i][j] + bf, 0.f);
            if (v > m) { m = v; arg = j; }
          }
        }
        const long o = ((long)b * a.T + t) * a.F + f;
        out[o] = m;
        if (argmax) argmax[o] = m > 0.f ? (uint8_t)arg : (uint8_t)0xFF;
      }
    }
  }
}

// d pooled of output o as the conv gradient at offset j of its pool window: all of it where the arg-max byte says j, else 0
__device__ __forceinline__ float routed_grad(const float* __restrict__ dout, const uint8_t* __restrict__ argmax, long o, int j) {
  return argmax[o] == j ? dout[o] : 0.f;
}

// Backward.  Phase 1 (lane f, wave rows r = dk E + e): d W[r, f] += g * window[c + dk, e] for the routed position c of every
// pooled output; d bias[f] += g.  Phase 2 (lane e, 8 groups over window rows): v[row, e] = sum_dk sum_f G[row - dk, f] W[dk, e, f]
// with G the routed conv gradient of this tile.  Phase 3: group q adds v[row] into table row s = token(row) for s % 8 == q, rows
// in order.
template <bool kTableInLds>
__global__ __launch_bounds__(256) void convpool_bwd_kernel(ConvArgs a, const float* __restrict__ dout, const uint8_t* __restrict__ argmax,
                                                           float* __restrict__ part_w, float* __restrict__ part_b,
                                                           float* __restrict__ part_t) {
  extern __shared__ float lds[];
  const int F4p = round4(a.F) + 4;               // row stride of W / G in LDS (lanes of phase 2 read different e rows)
  const int nrows = kTile * a.p + a.k - 1;
  const int ncpos = kTile * a.p;
  float* wb = lds;                               // [k][E][F4p]
  float* g = wb + a.k * a.E * F4p;               // [kTile p][F4p]
  float* win = g + ncpos * F4p;                  // [nrows][E4]
  float* v = win + nrows * a.E4;                 // [nrows][32]
  int* twin = reinterpret_cast<int*>(v + nrows * 32);
  float* tab = reinterpret_cast<float*>(twin + round4(nrows));   // [S][E] (kTableInLds)
  float* mytab = kTableInLds ? tab : part_t + (long)blockIdx.x * a.S * a.E;
  for (int i = threadIdx.x; i < a.k * a.E * F4p; i += blockDim.x) {
    const int fr = i % F4p, r = i / F4p;
    wb[i] = fr < a.F ? a.w[(long)r * a.F + fr] : 0.f;
  }
  for (int i = threadIdx.x; i < a.S * a.E; i += blockDim.x) mytab[i] = 0.f;
  const int f = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int KE = a.k * a.E;
  float accw[64];
#pragma unroll
  for (int q = 0; q < 64; ++q) accw[q] = 0.f;
  float accb = 0.f;
  const int tpb = (a.T + kTile - 1) / kTile;
  const int e2 = threadIdx.x & 31, grp = threadIdx.x >> 5;
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int b = (int)(tile / tpb), t0 = (int)(tile - (long)b * tpb) * kTile;
    __syncthreads();
    stage_window(a, b, t0, nrows, win, twin);
    for (int i = threadIdx.x; i < ncpos * F4p; i += blockDim.x) {
      const int c = i / F4p, fr = i - c * F4p;
      const int t = t0 + c / a.p, j = c % a.p;
      g[i] = (fr < a.F && t < a.T) ? routed_grad(dout, argmax, ((long)b * a.T + t) * a.F + fr, j) : 0.f;
    }
    __syncthreads();
    // phase 1
    if (f < a.F) {
      for (int tl = 0; tl < kTile; ++tl) {
        const int t = t0 + tl;
        if (t >= a.T) break;
        const long o = ((long)b * a.T + t) * a.F + f;
        const int am = argmax[o];
        if (am == 0xFF) continue;
        const float gv = dout[o];
        const int c = tl * a.p + am;
        if (wv == 0) accb += gv;
#pragma unroll
        for (int q = 0; q < 64; ++q) {
          const int r = wv + 4 * q;
          if (r < KE) {
            const int dk = r / a.E, e = r - dk * a.E;
            accw[q] = fmaf(gv, win[(c + dk) * a.E4 + e], accw[q]);
          }
        }
      }
    }
    // phase 2
    if (e2 < a.E) {
      for (int row = grp; row < nrows; row += 8) {
        float s = 0.f;
        for (int dk = 0; dk < a.k; ++dk) {
          const int c = row - dk;
          if (c < 0 || c >= ncpos) continue;
          const float* gp = g + c * F4p;
          const float* wp = wb + (dk * a.E + e2) * F4p;
          for (int fr = 0; fr < a.F; fr += 4) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(gp + fr);
            const f32x4 ww = *reinterpret_cast<const f32x4*>(wp + fr);
            s = fmaf(gg.x, ww.x, fmaf(gg.y, ww.y, fmaf(gg.z, ww.z, fmaf(gg.w, ww.w, s))));
          }
        }
        v[row * 32 + e2] = s;
      }
    }
    __syncthreads();
    // phase 3
    if (e2 < a.E) {
      for (int row = 0; row < nrows; ++row) {
        const int s = twin[row];
        if (s >= 0 && (s & 7) == grp) mytab[s * a.E + e2] += v[row * 32 + e2];
      }
    }
  }
  __syncthreads();
  if (f < a.F) {
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      const int r = wv + 4 * q;
      if (r < KE) part_w[(long)blockIdx.x * KE * a.F + (long)r * a.F + f] = accw[q];
    }
    if (wv == 0) part_b[(long)blockIdx.x * a.F + f] = accb;
  }
  if (kTableInLds)
    for (int i = threadIdx.x; i < a.S * a.E; i += blockDim.x) part_t[(long)blockIdx.x * a.S * a.E + i] = tab[i];
}

int conv_args(const int32_t* tokens, int32_t B, int32_t L, const float* table, int32_t S, int32_t E, const float* w, int32_t k,
              int32_t F, int32_t p, const char* who, ConvArgs& a) {
  if (B < 0 || L < 1 || L > KGCN_SEQ_MAX_LENGTH) return fail("%s: length %d outside 1..%d", who, L, KGCN_SEQ_MAX_LENGTH);
  if (E < 1 || E > KGCN_SEQ_MAX_EMBED) return fail("%s: embedding width %d outside 1..%d", who, E, KGCN_SEQ_MAX_EMBED);
  if (F < 1 || F > KGCN_SEQ_MAX_FILTERS) return fail("%s: %d filters outside 1..%d", who, F, KGCN_SEQ_MAX_FILTERS);
  if (k < 1 || k > KGCN_SEQ_MAX_KERNEL) return fail("%s: kernel size %d outside 1..%d", who, k, KGCN_SEQ_MAX_KERNEL);
  if (p < 1 || p > KGCN_SEQ_MAX_POOL) return fail("%s: pool size %d outside 1..%d", who, p, KGCN_SEQ_MAX_POOL);
  if (S < 1 || S > KGCN_SEQ_MAX_SYMBOLS) return fail("%s: %d symbols outside 1..%d", who, S, KGCN_SEQ_MAX_SYMBOLS);
  if ((int64_t)B * L >= (int64_t)INT32_MAX) return fail("%s: batch x length exceeds int32", who);
  if (B > 0 && (!tokens || !table || !w)) return fail("%s: NULL operand", who);
  a.tok = tokens; a.table = table; a.w = w;
  a.B = B; a.L = L; a.S = S; a.E = E; a.E4 = round4(E); a.F = F; a.k = k; a.p = p; a.padL = (k - 1) / 2; a.T = L / p;
  a.tiles = (long)B * ((a.T + kTile - 1) / kTile);
  a.scale = nullptr; a.rep = 1;
  a.sigma = nullptr; a.sample = nullptr; a.ids = nullptr; a.seed = 0;
  return 0;
}

size_t convpool_fwd_lds(const ConvArgs& a) {
  const int nrows = kTile * a.p + a.k - 1;
  return ((size_t)a.k * a.E4 * 64 + (size_t)nrows * a.E4 + nrows) * 4;
}
size_t convpool_bwd_lds(const ConvArgs& a, bool table_in_lds) {
  const int nrows = kTile * a.p + a.k - 1, F4p = round4(a.F) + 4;
  return ((size_t)a.k * a.E * F4p + (size_t)kTile * a.p * F4p + (size_t)nrows * a.E4 + (size_t)nrows * 32 + round4(nrows) +
          (table_in_lds ? (size_t)a.S * a.E : 0)) * 4;
}
int convpool_bwd_grid(const ConvArgs& a) { return (int)(a.tiles < kConvGridBwd ? (a.tiles > 0 ? a.tiles : 1) : kConvGridBwd); }

// the one forward launch (a.tiles > 0).  The staging mode follows from the operands the entry point put into ConvArgs
template <int kMode>
int launch_convpool_fwd_as(const ConvArgs& a, const float* bias, float* out, uint8_t* argmax, hipStream_t s, const char* label) {
  const size_t lds = convpool_fwd_lds(a);
  if (int rc = allow_full_lds<convpool_fwd_kernel<kMode>>(lds, "seq kernels")) return rc;
  const int grid = (int)(a.tiles < kConvGridFwd ? a.tiles : kConvGridFwd);
  hipLaunchKernelGGL(convpool_fwd_kernel<kMode>, dim3(grid), dim3(256), lds, s, a, bias, out, argmax);
  return check_launch(label);
}
int launch_convpool_fwd(const ConvArgs& a, const float* bias, float* out, uint8_t* argmax, hipStream_t s) {
  if (a.sigma) return launch_convpool_fwd_as<kStagePerturbed>(a, bias, out, argmax, s, "convpool_fwd_kernel<perturbed>");
  if (a.scale) return launch_convpool_fwd_as<kStageScaled>(a, bias, out, argmax, s, "convpool_fwd_kernel<scaled>");
  return launch_convpool_fwd_as<kStagePlain>(a, bias, out, argmax, s, "convpool_fwd_kernel");
}

// ---- integrated gradients of the sequence input ---------------------------------------------------------------------------
// Gradient with respect to the (scaled) embedded input of the conv-pool, summed over the rep copies of a compound:
//   dx[c, m, e] = sum_r wt[c rep + r] sum_dk sum_f G_r[m + padL - dk, f] W[dk, e, f]   (times table[tok[c, m], e] if asked)
// with G_r the conv gradient of row c rep + r routed through its arg-max bytes.  Workgroup (compound c, kIgPos output
// positions); lane e (< 32), thread group grp (8 of them) owns positions grp + 8 q.  Per copy, in copy order: the routed conv
// gradient of the window [kIgPos + k - 1][F4p] is staged in LDS, every thread forms its four positions against W (in LDS) and
// adds them, times the copy's weight, into registers.  No weight gradient, no atomics: a fixed summation order.
constexpr int kIgPos = 32;
__global__ __launch_bounds__(256) void convpool_input_grad_kernel(ConvArgs a, const float* __restrict__ dout,
                                                                  const uint8_t* __restrict__ argmax, const float* __restrict__ wt,
                                                                  int times_table, float* __restrict__ dx) {
  extern __shared__ float lds[];
  const int F4p = round4(a.F) + 4;
  const int nw = kIgPos + a.k - 1;
  float* wb = lds;                               // [k][E][F4p]
  float* g = wb + a.k * a.E * F4p;               // [nw][F4p]
  const int c = blockIdx.x, m0 = blockIdx.y * kIgPos;
  const int lbase = m0 + a.padL - (a.k - 1);     // conv position of window row 0
  const int TP = a.T * a.p;
  for (int i = threadIdx.x; i < a.k * a.E * F4p; i += blockDim.x) {
    const int fr = i % F4p, r = i / F4p;
    wb[i] = fr < a.F ? a.w[(long)r * a.F + fr] : 0.f;
  }
  const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < a.rep; ++r) {
    const long b = (long)c * a.rep + r;
    const float wr = wt ? wt[b] : 1.f;
    if (wr == 0.f) continue;                     // uniform over the workgroup
    __syncthreads();                             // W is staged / the previous copy's window is no longer read
    for (int i = threadIdx.x; i < nw * F4p; i += blockDim.x) {
      const int row = i / F4p, fr = i - row * F4p;
      const int l = lbase + row;
      const int t = l / a.p, j = l - t * a.p;
      g[i] = (fr < a.F && l >= 0 && l < TP) ? routed_grad(dout, argmax, (b * a.T + t) * a.F + fr, j) : 0.f;
    }
    __syncthreads();
    if (e < a.E) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int dk = 0; dk < a.k; ++dk) {
        const float* wp = wb + (dk * a.E + e) * F4p;
        const float* gp = g + (grp + a.k - 1 - dk) * F4p;     // window row of position grp + 8 q: + 8 q rows
        for (int fr = 0; fr < a.F; fr += 4) {
          const f32x4 ww = *reinterpret_cast<const f32x4*>(wp + fr);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(gp + 8 * q * F4p + fr);
            v[q] = fmaf(gg.x, ww.x, fmaf(gg.y, ww.y, fmaf(gg.z, ww.z, fmaf(gg.w, ww.w, v[q]))));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fmaf(wr, v[q], acc[q]);
    }
  }
  if (e < a.E) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + grp + 8 * q;
      if (m >= a.L) continue;
      float val = acc[q];
      if (times_table) val *= a.table[(long)a.tok[(long)c * a.L + m] * a.E + e];
      dx[((long)c * a.L + m) * a.E + e] = val;
    }
  }
}

size_t convpool_input_grad_lds(const ConvArgs& a) {
  const int F4p = round4(a.F) + 4;
  return ((size_t)a.k * a.E * F4p + (size_t)(kIgPos + a.k - 1) * F4p) * 4;
}

// the batch of the scaled forward / input gradient: `batch` rows, rep copies of each of the batch / rep token rows
int rep_args(int32_t batch, int32_t rep, const char* who) {
  if (rep < 1) return fail("%s: %d copies per token row", who, rep);
  if (batch < 0 || batch % rep) return fail("%s: %d rows are not whole groups of %d copies", who, batch, rep);
  return 0;
}

// ---- LSTM ---------------------------------------------------------------------------------------------------------------
struct LstmArgs {
  const float* x;       // [B, T, D]
  const float* wx;      // [D, 4H]
  const float* wh;      // [H, 4H]
  const float* bias;    // [4H]
  int B, T, D, H, Hp, seqs, KA4, wstride, act;
};

__device__ __forceinline__ float rec_act(float z, int act) {
  if (act == KGCN_SEQ_ACT_SIGMOID) return 1.f / (1.f + expf(-z));
  // Keras hard_sigmoid: 0.2 x + 0.5, then clip.  The _rn forms do not keep the compiler from fusing the two into one FMA
  // (see rec_act_grad); the clip gives exactly 0 and 1 at z = -2.5 and 2.5 either way
  const float y = __fadd_rn(__fmul_rn(0.2f, z), 0.5f);
  return fminf(fmaxf(y, 0.f), 1.f);
}
// derivative; tf.clip_by_value passes the gradient at the boundaries, z = -2.5 and z = 2.5, and nowhere beyond.  The test is on
// z and not on y: rounded twice, 0.2 z + 0.5 is exactly 1 for the float above 2.5 as well (a tie that rounds to even), and
// __fmul_rn is a plain product in HIP, so that under -ffp-contract=fast y is one FMA, -7.5e-9 at z = -2.5 (0.2f > 0.2)
__device__ __forceinline__ float rec_act_grad(float z, float a, int act) {
  if (act == KGCN_SEQ_ACT_SIGMOID) return a * (1.f - a);
  return (z >= -2.5f && z <= 2.5f) ? 0.2f : 0.f;
}

// thread (sequence s = tid / Hp, unit u = tid % Hp); LDS: W [4][Hp][wstride] over k = [x (D) | h (H)], state [2][seqs][KA4]
__global__ __launch_bounds__(256) void lstm_fwd_kernel(LstmArgs a, float* __restrict__ h_out, long h_ld, float* __restrict__ stash) {
  extern __shared__ float lds[];
  float* wl = lds;
  float* st = wl + 4 * a.Hp * a.wstride;
  const int H = a.H, D = a.D;
  for (int i = threadIdx.x; i < 4 * a.Hp * a.wstride; i += blockDim.x) {
    const int kk = i % a.wstride, r = i / a.wstride, u = r % a.Hp, gt = r / a.Hp;
    float v = 0.f;
    if (u < H) {
      const int n = gt * H + u;
      if (kk < D) v = a.wx[(long)kk * 4 * H + n];
      else if (kk < D + H) v = a.wh[(long)(kk - D) * 4 * H + n];
    }
    wl[i] = v;
  }
  for (int i = threadIdx.x; i < 2 * a.seqs * a.KA4; i += blockDim.x) st[i] = 0.f;
  __syncthreads();                              // the first step's x goes into the zeroed slab, written by other threads
  const int s = threadIdx.x / a.Hp, u = threadIdx.x - s * a.Hp;
  const int b = blockIdx.x * a.seqs + s;
  const bool live = u < H && b < a.B;
  float bg[4];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt) bg[gt] = u < H ? a.bias[gt * H + u] : 0.f;
  float c = 0.f, h = 0.f;
  // x staging: element q of the [seqs, D] slab of a step; <= 4 per thread (seqs D <= 256 * 4)
  const int nx = a.seqs * D;
  float xr[4];
  auto load_x = [&](int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = threadIdx.x + q * 256;
      xr[q] = 0.f;
      if (i < nx && t >= 0) {
        const int ss = i / D, kk = i - ss * D, bb = blockIdx.x * a.seqs + ss;
        if (bb < a.B) xr[q] = a.x[((long)bb * a.T + t) * D + kk];
      }
    }
  };
  load_x(a.T - 1);
  int buf = 0;
  for (int t = a.T - 1; t >= 0; --t) {                        // go_backwards: the last input step first
    float* cur = st + buf * a.seqs * a.KA4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = threadIdx.x + q * 256;
      if (i < nx) {
        const int ss = i / D;
        cur[ss * a.KA4 + (i - ss * D)] = xr[q];
      }
    }
    load_x(t - 1);                                            // the next step's inputs are in flight during this one
    __syncthreads();
    float z[4] = {bg[0], bg[1], bg[2], bg[3]};
    const float* xh = cur + s * a.KA4;
    for (int kk = 0; kk < a.KA4; kk += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xh + kk);
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wl + (gt * a.Hp + u) * a.wstride + kk);
        z[gt] = fmaf(v.x, w.x, fmaf(v.y, w.y, fmaf(v.z, w.z, fmaf(v.w, w.w, z[gt]))));
      }
    }
    const float ig = rec_act(z[0], a.act), fg = rec_act(z[1], a.act), og = rec_act(z[3], a.act);
    c = fg * c + ig * tanhf(z[2]);
    h = og * tanhf(c);
    float* nxt = st + (buf ^ 1) * a.seqs * a.KA4;
    if (u < H) nxt[s * a.KA4 + D + u] = h;
    if (stash && live) {
      float* sp = stash + ((long)b * a.T + t) * 6 * H;
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) sp[gt * H + u] = z[gt];
      sp[4 * H + u] = h;
      sp[5 * H + u] = c;
    }
    buf ^= 1;
  }
  if (live) h_out[(long)b * h_ld + u] = h;
}

// thread (s, u): dz of its four gates, then dh_prev[s, u] = dz[s, :] . W_h[u, :] and dx[s, t, kk] = dz[s, :] . W_x[kk, :] for
// kk = u, u + Hp, ...  LDS: Wx [D][4H + 4], Wh [H][4H + 4], dz [seqs][4H + 4], dh [2][seqs][Hp]
__global__ __launch_bounds__(256) void lstm_bwd_kernel(LstmArgs a, const float* __restrict__ dh_in, long dh_ld,
                                                       float* __restrict__ stash, float* __restrict__ dx) {
  extern __shared__ float lds[];
  const int H = a.H, D = a.D, N4 = 4 * H, ws = 4 * H + 4;
  float* wx = lds;
  float* wh = wx + D * ws;
  float* dzl = wh + H * ws;
  float* dhl = dzl + a.seqs * ws;
  for (int i = threadIdx.x; i < D * ws; i += blockDim.x) {
    const int r = i / ws, n = i - r * ws;
    wx[i] = n < N4 ? a.wx[(long)r * N4 + n] : 0.f;
  }
  for (int i = threadIdx.x; i < H * ws; i += blockDim.x) {
    const int r = i / ws, n = i - r * ws;
    wh[i] = n < N4 ? a.wh[(long)r * N4 + n] : 0.f;
  }
  const int s = threadIdx.x / a.Hp, u = threadIdx.x - s * a.Hp;
  const int b = blockIdx.x * a.seqs + s;
  const bool live = u < H && b < a.B;
  for (int i = threadIdx.x; i < 2 * a.seqs * a.Hp; i += blockDim.x) dhl[i] = 0.f;
  __syncthreads();
  if (live && dh_in) dhl[s * a.Hp + u] = dh_in[(long)b * dh_ld + u];
  float dc = 0.f;
  int buf = 0;
  for (int t = 0; t < a.T; ++t) {                            // reverse of the processing order
    __syncthreads();                                          // dh of this step is complete; dz of the last step is read
    float dz[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      float* sp = stash + ((long)b * a.T + t) * 6 * H;
      const float zi = sp[u], zf = sp[H + u], zg = sp[2 * H + u], zo = sp[3 * H + u];
      const float ct = sp[5 * H + u];
      const float cp = t + 1 < a.T ? sp[6 * H + 5 * H + u] : 0.f;   // the state before this step: after input t + 1
      const float dh = dhl[buf * a.seqs * a.Hp + s * a.Hp + u];
      const float ig = rec_act(zi, a.act), fg = rec_act(zf, a.act), og = rec_act(zo, a.act), gg = tanhf(zg);
      const float tc = tanhf(ct);
      dc = dc + dh * og * (1.f - tc * tc);
      dz[0] = dc * gg * rec_act_grad(zi, ig, a.act);
      dz[1] = dc * cp * rec_act_grad(zf, fg, a.act);
      dz[2] = dc * ig * (1.f - gg * gg);
      dz[3] = dh * tc * rec_act_grad(zo, og, a.act);
      dc = dc * fg;
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) sp[gt * H + u] = dz[gt];          // z -> dz (read by the weight-gradient kernel)
    }
    if (u < H) {
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) dzl[s * ws + gt * H + u] = dz[gt];
    }
    __syncthreads();
    const float* dzs = dzl + s * ws;
    if (u < H) {
      const float* wr = wh + u * ws;
      float acc = 0.f;
      for (int n = 0; n < N4; n += 4) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(dzs + n);
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + n);
        acc = fmaf(g4.x, w4.x, fmaf(g4.y, w4.y, fmaf(g4.z, w4.z, fmaf(g4.w, w4.w, acc))));
      }
      dhl[(buf ^ 1) * a.seqs * a.Hp + s * a.Hp + u] = acc;
    }
    if (b < a.B) {
      for (int kk = u; kk < D; kk += a.Hp) {
        const float* wr = wx + kk * ws;
        float acc = 0.f;
        for (int n = 0; n < N4; n += 4) {
          const f32x4 g4 = *reinterpret_cast<const f32x4*>(dzs + n);
          const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + n);
          acc = fmaf(g4.x, w4.x, fmaf(g4.y, w4.y, fmaf(g4.z, w4.z, fmaf(g4.w, w4.w, acc))));
        }
        if (dx) dx[((long)b * a.T + t) * D + kk] = acc;
      }
    }
    buf ^= 1;
  }
}

// rows r = (b, t) of chunk blockIdx.x; column n = threadIdx.x (< 4H); k tile blockIdx.y of a_r = [x_r (D) | h_prev (H) | 1]
constexpr int kWgRows = 32, kWgK = 16;
__global__ __launch_bounds__(256) void lstm_wgrad_kernel(LstmArgs a, const float* __restrict__ stash, long rows, long rows_per_chunk,
                                                         float* __restrict__ part_x, float* __restrict__ part_h,
                                                         float* __restrict__ part_b) {
  __shared__ __attribute__((aligned(16))) float as[kWgRows][kWgK];
  __shared__ float dzs[kWgRows][256];
  const int H = a.H, D = a.D, N4 = 4 * H, KA = D + H + 1;
  const int n = threadIdx.x, k0 = blockIdx.y * kWgK;
  const long r0 = (long)blockIdx.x * rows_per_chunk;
  const long r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
  float acc[kWgK];
#pragma unroll
  for (int q = 0; q < kWgK; ++q) acc[q] = 0.f;
  for (long rb = r0; rb < r1; rb += kWgRows) {
    __syncthreads();
    for (int i = threadIdx.x; i < kWgRows * kWgK; i += blockDim.x) {
      const int rr = i / kWgK, kq = i - rr * kWgK, kk = k0 + kq;
      const long r = rb + rr;
      float v = 0.f;
      if (r < r1) {
        const long bb = r / a.T;
        const int t = (int)(r - bb * a.T);
        if (kk < D) v = a.x[r * D + kk];
        else if (kk < D + H) v = t + 1 < a.T ? stash[(r + 1) * 6 * H + 4 * H + (kk - D)] : 0.f;
        else if (kk == D + H) v = 1.f;
      }
      as[rr][kq] = v;
    }
    for (int i = threadIdx.x; i < kWgRows * N4; i += blockDim.x) {
      const int rr = i / N4, nn = i - rr * N4;
      const long r = rb + rr;
      dzs[rr][nn] = r < r1 ? stash[r * 6 * H + nn] : 0.f;
    }
    __syncthreads();
    if (n < N4) {
      for (int rr = 0; rr < kWgRows; ++rr) {
        const float g = dzs[rr][n];
#pragma unroll
        for (int q = 0; q < kWgK; q += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(&as[rr][q]);
          acc[q] = fmaf(v.x, g, acc[q]);
          acc[q + 1] = fmaf(v.y, g, acc[q + 1]);
          acc[q + 2] = fmaf(v.z, g, acc[q + 2]);
          acc[q + 3] = fmaf(v.w, g, acc[q + 3]);
        }
      }
    }
  }
  if (n < N4) {
#pragma unroll
    for (int q = 0; q < kWgK; ++q) {
      const int kk = k0 + q;
      if (kk < D) part_x[(long)blockIdx.x * D * N4 + (long)kk * N4 + n] = acc[q];
      else if (kk < D + H) part_h[(long)blockIdx.x * H * N4 + (long)(kk - D) * N4 + n] = acc[q];
      else if (kk == D + H) part_b[(long)blockIdx.x * N4 + n] = acc[q];
    }
  }
  (void)KA;
}

int lstm_args(const float* x, int32_t B, int32_t T, int32_t D, const float* wx, const float* wh, const float* bias, int32_t H,
              int32_t act, const char* who, LstmArgs& a) {
  if (B < 0 || T < 0 || T > KGCN_SEQ_MAX_LENGTH) return fail("%s: %d steps outside 0..%d", who, T, KGCN_SEQ_MAX_LENGTH);
  if (D < 1 || D > KGCN_SEQ_MAX_LSTM_INPUT) return fail("%s: input width %d outside 1..%d", who, D, KGCN_SEQ_MAX_LSTM_INPUT);
  if (H < 1 || H > KGCN_SEQ_MAX_UNITS) return fail("%s: %d units outside 1..%d", who, H, KGCN_SEQ_MAX_UNITS);
  if (act != KGCN_SEQ_ACT_HARD_SIGMOID && act != KGCN_SEQ_ACT_SIGMOID) return fail("%s: recurrent activation %d", who, act);
  if ((int64_t)B * T * 6 * H >= (int64_t)INT32_MAX * 8) return fail("%s: batch x steps too large", who);
  if (B > 0 && (!wx || !wh || !bias || (T > 0 && !x))) return fail("%s: NULL operand", who);
  a.x = x; a.wx = wx; a.wh = wh; a.bias = bias;
  a.B = B; a.T = T; a.D = D; a.H = H; a.act = act;
  a.Hp = H <= 16 ? 16 : (H <= 32 ? 32 : 64);
  a.seqs = 256 / a.Hp;
  a.KA4 = round4(D + H);
  a.wstride = ((a.KA4 / 4) & 1) ? a.KA4 : a.KA4 + 4;
  return 0;
}

long wgrad_rows_per_chunk(const LstmArgs& a) {
  const long rows = (long)a.B * a.T;
  long per = (rows + kLstmChunks - 1) / kLstmChunks;
  return per < 1 ? 1 : per;
}

// `parts` partial results of each gradient, one array after the other; n[i] is the length of one partial of array i
struct PartWorkspace { int parts; float* part[3]; long n[3]; size_t bytes; };
PartWorkspace part_layout(void* base, int parts, long n0, long n1, long n2) {
  Taker t(base, 4);
  PartWorkspace w{parts, {}, {n0, n1, n2}, 0};
  for (int i = 0; i < 3; ++i) w.part[i] = t.take<float>((size_t)parts * w.n[i]);
  w.bytes = t.off;
  return w;
}
// conv-pool backward: d W [k, E, F] | d bias [F] | d table [S, E], one partial per workgroup of the grid
PartWorkspace convpool_bwd_layout(void* base, const ConvArgs& a) {
  return part_layout(base, convpool_bwd_grid(a), (long)a.k * a.E * a.F, a.F, (long)a.S * a.E);
}
// LSTM weight gradients: d W_x [D, 4H] | d W_h [H, 4H] | d bias [4H], one partial per row chunk
PartWorkspace lstm_wgrad_layout(void* base, int32_t in_dim, int32_t units) {
  return part_layout(base, kLstmChunks, (long)in_dim * 4 * units, (long)units * 4 * units, 4L * units);
}
int reduce_parts(const PartWorkspace& w, float* out0, float* out1, float* out2, hipStream_t s) {
  float* out[3] = {out0, out1, out2};
  for (int i = 0; i < 3; ++i)
    if (int rc = reduce_or_defer(w.part[i], w.parts, w.n[i], out[i], s)) return rc;
  return 0;
}
}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_seq_convpool_workspace_bytes(int32_t batch, int32_t length, int32_t symbols, int32_t embed_dim,
                                                     int32_t kernel_size, int32_t filters, int32_t pool) {
  ConvArgs a;
  if (conv_args(nullptr, 0, length, nullptr, symbols, embed_dim, nullptr, kernel_size, filters, pool, "workspace", a)) return -1;
  a.tiles = (long)(batch > 0 ? batch : 0) * ((a.T + kTile - 1) / kTile);
  return (int64_t)convpool_bwd_layout(nullptr, a).bytes;
}

extern "C" int kgcn_seq_convpool_fwd_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* table, int32_t symbols,
                                         int32_t embed_dim, const float* w, const float* bias, int32_t kernel_size, int32_t filters,
                                         int32_t pool, float* out, uint8_t* argmax, void* stream) {
  const char* who = "kgcn_seq_convpool_fwd_f32";
  ConvArgs a;
  if (int rc = conv_args(tokens, batch, length, table, symbols, embed_dim, w, kernel_size, filters, pool, who, a)) return rc;
  if (a.tiles == 0) return 0;
  if (!bias || !out) return fail("%s: NULL operand", who);
  return launch_convpool_fwd(a, bias, out, argmax, as_stream(stream));
}

extern "C" int kgcn_seq_convpool_bwd_f32(const int32_t* tokens, int32_t batch, int32_t length, const float* table, int32_t symbols,
                                         int32_t embed_dim, const float* w, int32_t kernel_size, int32_t filters, int32_t pool,
                                         const float* dout, const uint8_t* argmax, float* dtable, float* dw, float* dbias,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_seq_convpool_bwd_f32";
  ConvArgs a;
  if (int rc = conv_args(tokens, batch, length, table, symbols, embed_dim, w, kernel_size, filters, pool, who, a)) return rc;
  if (!dtable || !dw || !dbias) return fail("%s: NULL gradient", who);
  if (a.tiles > 0 && (!dout || !argmax)) return fail("%s: NULL operand", who);
  const PartWorkspace ws = convpool_bwd_layout(workspace, a);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)ws.bytes)) return rc;
  hipStream_t s = as_stream(stream);
  const int grid = ws.parts;
  float *part_w = ws.part[0], *part_b = ws.part[1], *part_t = ws.part[2];
  if (a.tiles == 0) {                                 // no pooled output: zero gradients (the partials are zeroed and reduced)
    if (int rc = zero_async(who, workspace, ws.bytes, s)) return rc;
  } else {
    const bool in_lds = convpool_bwd_lds(a, true) <= (size_t)kLdsBytes;
    const size_t lds = convpool_bwd_lds(a, in_lds);
    if (in_lds) {
      if (int rc = allow_full_lds<convpool_bwd_kernel<true>>(lds, "seq kernels")) return rc;
      hipLaunchKernelGGL(convpool_bwd_kernel<true>, dim3(grid), dim3(256), lds, s, a, dout, argmax, part_w, part_b, part_t);
    } else {
      if (int rc = allow_full_lds<convpool_bwd_kernel<false>>(lds, "seq kernels")) return rc;
      hipLaunchKernelGGL(convpool_bwd_kernel<false>, dim3(grid), dim3(256), lds, s, a, dout, argmax, part_w, part_b, part_t);
    }
    if (int rc = check_launch("convpool_bwd_kernel")) return rc;
  }
  return reduce_parts(ws, dw, dbias, dtable, s);
}

extern "C" int kgcn_seq_convpool_scaled_fwd_f32(const int32_t* tokens, int32_t batch, int32_t rep, const float* scale, int32_t length,
                                                const float* table, int32_t symbols, int32_t embed_dim, const float* w, const float* bias,
                                                int32_t kernel_size, int32_t filters, int32_t pool, float* out, uint8_t* argmax,
                                                void* stream) {
  const char* who = "kgcn_seq_convpool_scaled_fwd_f32";
  ConvArgs a;
  if (int rc = rep_args(batch, rep, who)) return rc;
  if (int rc = conv_args(tokens, batch, length, table, symbols, embed_dim, w, kernel_size, filters, pool, who, a)) return rc;
  if (a.tiles == 0) return 0;
  if (!bias || !out || !scale) return fail("%s: NULL operand", who);
  a.scale = scale; a.rep = rep;
  return launch_convpool_fwd(a, bias, out, argmax, as_stream(stream));
}

extern "C" int kgcn_seq_convpool_perturbed_fwd_f32(const int32_t* tokens, int32_t batch, int32_t rep, const float* scale,
                                                   const float* sigma, const int32_t* sample, const int32_t* ids, uint64_t seed,
                                                   int32_t length, const float* table, int32_t symbols, int32_t embed_dim,
                                                   const float* w, const float* bias, int32_t kernel_size, int32_t filters,
                                                   int32_t pool, float* out, uint8_t* argmax, void* stream) {
  const char* who = "kgcn_seq_convpool_perturbed_fwd_f32";
  ConvArgs a;
  if (int rc = rep_args(batch, rep, who)) return rc;
  if (int rc = conv_args(tokens, batch, length, table, symbols, embed_dim, w, kernel_size, filters, pool, who, a)) return rc;
  if (a.tiles == 0) return 0;
  if (!bias || !out || !scale || !sigma || !sample || !ids) return fail("%s: NULL operand", who);
  a.scale = scale; a.rep = rep; a.sigma = sigma; a.sample = sample; a.ids = ids; a.seed = seed;
  return launch_convpool_fwd(a, bias, out, argmax, as_stream(stream));
}

extern "C" int kgcn_seq_convpool_input_grad_f32(const int32_t* tokens, int32_t batch, int32_t rep, int32_t length, const float* table,
                                                int32_t symbols, int32_t embed_dim, const float* w, int32_t kernel_size,
                                                int32_t filters, int32_t pool, const float* dout, const uint8_t* argmax,
                                                const float* row_weight, int32_t times_table, float* dx, void* stream) {
  const char* who = "kgcn_seq_convpool_input_grad_f32";
  ConvArgs a;
  if (int rc = rep_args(batch, rep, who)) return rc;
  if (int rc = conv_args(tokens, batch, length, table, symbols, embed_dim, w, kernel_size, filters, pool, who, a)) return rc;
  if (batch == 0) return 0;
  if (!dx || (a.T > 0 && (!dout || !argmax))) return fail("%s: NULL operand", who);
  a.rep = rep;
  const size_t lds = convpool_input_grad_lds(a);
  if (int rc = allow_full_lds<convpool_input_grad_kernel>(lds, "seq kernels")) return rc;
  hipLaunchKernelGGL(convpool_input_grad_kernel, dim3(batch / rep, (length + kIgPos - 1) / kIgPos), dim3(256), lds,
                     as_stream(stream), a, dout, argmax, row_weight, times_table ? 1 : 0, dx);
  return check_launch("convpool_input_grad_kernel");
}

extern "C" int64_t kgcn_seq_lstm_stash_floats(int32_t batch, int32_t steps, int32_t units) {
  return (int64_t)batch * steps * 6 * units;
}

extern "C" int64_t kgcn_seq_lstm_workspace_bytes(int32_t batch, int32_t steps, int32_t in_dim, int32_t units) {
  (void)batch; (void)steps;
  return (int64_t)lstm_wgrad_layout(nullptr, in_dim, units).bytes;
}

extern "C" int kgcn_seq_lstm_fwd_f32(const float* x, int32_t batch, int32_t steps, int32_t in_dim, const float* wx, const float* wh,
                                     const float* bias, int32_t units, int32_t recurrent_act, float* h_out, int64_t h_ld,
                                     float* stash, void* stream) {
  const char* who = "kgcn_seq_lstm_fwd_f32";
  LstmArgs a;
  if (int rc = lstm_args(x, batch, steps, in_dim, wx, wh, bias, units, recurrent_act, who, a)) return rc;
  if (batch == 0) return 0;
  if (!h_out || h_ld < units) return fail("%s: output NULL or its row stride %lld < %d", who, (long long)h_ld, units);
  const size_t lds = ((size_t)4 * a.Hp * a.wstride + 2 * (size_t)a.seqs * a.KA4) * 4;
  if (int rc = allow_full_lds<lstm_fwd_kernel>(lds, "seq kernels")) return rc;
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3((batch + a.seqs - 1) / a.seqs), dim3(256), lds, as_stream(stream), a, h_out, (long)h_ld,
                     stash);
  return check_launch("lstm_fwd_kernel");
}

extern "C" int kgcn_seq_lstm_bwd_f32(const float* x, int32_t batch, int32_t steps, int32_t in_dim, const float* wx, const float* wh,
                                     const float* bias, int32_t units, int32_t recurrent_act, const float* dh, int64_t dh_ld,
                                     float* stash, float* dx, float* dwx, float* dwh, float* dbias, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_seq_lstm_bwd_f32";
  LstmArgs a;
  if (int rc = lstm_args(x, batch, steps, in_dim, wx, wh, bias, units, recurrent_act, who, a)) return rc;
  if (dh && dh_ld < units) return fail("%s: gradient row stride %lld < %d", who, (long long)dh_ld, units);
  if (batch > 0 && steps > 0 && !stash) return fail("%s: NULL stash", who);
  // the weight gradients' refusals come before the first launch: a refused call has written nothing
  const bool wgrad = dwx || dwh || dbias;
  if (wgrad && (!dwx || !dwh || !dbias)) return fail("%s: d W_x, d W_h and d bias are formed together", who);
  const PartWorkspace ws = lstm_wgrad_layout(wgrad ? workspace : nullptr, in_dim, units);
  if (wgrad)
    if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)ws.bytes)) return rc;
  hipStream_t s = as_stream(stream);
  const int N4 = 4 * units;
  if (batch > 0 && steps > 0) {
    const size_t lds = ((size_t)(in_dim + units + a.seqs) * (N4 + 4) + 2 * (size_t)a.seqs * a.Hp) * 4;
    if (int rc = allow_full_lds<lstm_bwd_kernel>(lds, "seq kernels")) return rc;
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3((batch + a.seqs - 1) / a.seqs), dim3(256), lds, s, a, dh, (long)dh_ld, stash, dx);
    if (int rc = check_launch("lstm_bwd_kernel")) return rc;
  }
  if (!wgrad) return 0;
  const long rows = (long)batch * steps;
  if (rows == 0) {
    if (int rc = zero_async(who, workspace, ws.bytes, s)) return rc;
  } else {
    const long per = wgrad_rows_per_chunk(a);
    const int ktiles = (in_dim + units + 1 + kWgK - 1) / kWgK;
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(kLstmChunks, ktiles), dim3(N4 <= 64 ? 64 : (N4 <= 128 ? 128 : 256)), 0, s, a, stash,
                       rows, per, ws.part[0], ws.part[1], ws.part[2]);
    if (int rc = check_launch("lstm_wgrad_kernel")) return rc;
  }
  return reduce_parts(ws, dwx, dwh, dbias, s);
}
