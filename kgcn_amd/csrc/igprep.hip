// Perturbed inputs of the smooth attribution methods (kgcn/visualization.py:235-259 smooth_grad / smooth_ig; kgcn/feed.py:88-89
// add_perturbation: x * scaling + N(0, noise_scale)), drawn where they are consumed instead of on the host.
//
//   noise   one N(0, 1) per (seed, stream s, compound g, sample k, row r, column w) of a 2-D array [R, W]: normal number w & 3 of
//           the Philox4x64-10 block with counter (r ceil(W / 4) + (w >> 2), k, g, s) and key (seed, 0), Box-Muller as in the VAE
//           noise (philox.h).  g is the compound's index in the DATASET and k the sample number, so the value does not depend on
//           where in a launch (which chunk, which batch row) the copy sits.
//   rows    out[b, r, w] = x[b / rep, r, w] * scale[b] + sigma[b] * z(ids[b / rep], sample[b], r, w): the node features [N, F]
//           of rep copies of every compound (stream 0).  One thread per Philox block = four outputs of one row.
//   values  the same for the stored values of one adjacency channel of a batched CSR (stream 1 + channel): graph b's entries
//           rowptr[b rows] .. rowptr[(b + 1) rows] are the array [1, nnz_b] in CSR order.
// A copy with sigma[b] == 0 is x * scale[b], the product the clean path forms, and draws nothing.  The conv-pool stages the noise
// of the embedded sequence itself (seq.hip, stream 0x100).
#include "kgcn_common.h"
#include "philox.h"

namespace kgcn {

namespace {
struct PerturbArgs {
  const float* scale;     // [B]
  const float* sigma;     // [B]
  const int32_t* sample;  // [B]
  const int32_t* ids;     // rows: [B / rep]; values: [B]
  uint64_t seed;
  uint32_t stream;
};

// thread i = (b, r, q): columns 4 q .. 4 q + 3 of row r of copy b
__global__ __launch_bounds__(256) void ig_perturb_rows_kernel(PerturbArgs a, const float* __restrict__ x, long B, int rep, int R, int W,
                                                              int vec, float* __restrict__ out) {
  const int W4 = (W + 3) >> 2;
  const long per = (long)R * W4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * per) return;
  const long b = i / per;
  const long blk = i - b * per;
  const int r = (int)(blk / W4), q = (int)(blk - (long)r * W4);
  const float sc = a.scale[b], sg = a.sigma[b];
  const float* src = x + ((b / rep) * R + r) * (long)W + 4 * q;
  float* dst = out + (b * R + r) * (long)W + 4 * q;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (sg != 0.f) ig_noise4(a.seed, a.stream, (uint32_t)a.ids[b / rep], (uint32_t)a.sample[b], (uint64_t)blk, z);
  if (vec) {                                             // W % 4 == 0 and aligned bases: every block is one 16-byte access
    const f32x4 v = *reinterpret_cast<const f32x4*>(src);
    f32x4 o;
    o.x = v.x * sc; o.y = v.y * sc; o.z = v.z * sc; o.w = v.w * sc;
    if (sg != 0.f) { o.x = fmaf(sg, z[0], o.x); o.y = fmaf(sg, z[1], o.y); o.z = fmaf(sg, z[2], o.z); o.w = fmaf(sg, z[3], o.w); }
    *reinterpret_cast<f32x4*>(dst) = o;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * q + j < W) {
        const float v = src[j] * sc;
        dst[j] = sg != 0.f ? fmaf(sg, z[j], v) : v;
      }
    }
  }
}

// workgroup (graph b, slice blockIdx.y of its Philox blocks)
__global__ __launch_bounds__(256) void ig_perturb_values_kernel(PerturbArgs a, const int32_t* __restrict__ rowptr, int rows, long nnz,
                                                                const float* __restrict__ vals, float* __restrict__ out) {
  const long b = blockIdx.x;
  long e0 = rowptr[b * rows], e1 = rowptr[(b + 1) * rows];
  if (e0 < 0) e0 = 0;
  if (e1 > nnz) e1 = nnz;
  const long n = e1 - e0;                                // <= 0: a graph without entries
  const float sc = a.scale[b], sg = a.sigma[b];
  const uint32_t g = (uint32_t)a.ids[b], k = (uint32_t)a.sample[b];
  for (long q = (long)blockIdx.y * 256 + threadIdx.x; 4 * q < n; q += (long)gridDim.y * 256) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (sg != 0.f) ig_noise4(a.seed, a.stream, g, k, (uint64_t)q, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = 4 * q + j;
      if (e < n) {
        const float v = vals[e0 + e] * sc;
        out[e0 + e] = sg != 0.f ? fmaf(sg, z[j], v) : v;
      }
    }
  }
}

int perturb_args(const float* scale, const float* sigma, const int32_t* sample, const int32_t* ids, uint32_t stream, uint64_t seed,
                 const char* who, PerturbArgs& a) {
  if (!scale || !sigma || !sample || !ids) return fail("%s: NULL scale / sigma / sample / ids", who);
  a.scale = scale; a.sigma = sigma; a.sample = sample; a.ids = ids; a.seed = seed; a.stream = stream;
  return 0;
}
}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_ig_perturb_rows_f32(const float* x, int64_t batch, int32_t rep, int32_t rows, int32_t width, const float* scale,
                                        const float* sigma, const int32_t* sample, const int32_t* ids, uint32_t noise_stream,
                                        uint64_t seed, float* out, void* stream) {
  const char* who = "kgcn_ig_perturb_rows_f32";
  if (rep < 1 || batch < 0 || batch % rep) return fail("%s: %lld rows are not whole groups of %d copies", who, (long long)batch, rep);
  if (rows < 0 || width < 0) return fail("%s: negative array shape [%d, %d]", who, rows, width);
  const int64_t per = (int64_t)rows * ((width + 3) / 4);
  if (batch == 0 || per == 0) return 0;
  if (batch > ((int64_t)INT32_MAX * 256) / per) return fail("%s: %lld x [%d, %d] exceeds the grid", who, (long long)batch, rows, width);
  PerturbArgs a;
  if (int rc = perturb_args(scale, sigma, sample, ids, noise_stream, seed, who, a)) return rc;
  if (!x || !out) return fail("%s: NULL operand", who);
  const int vec = (width & 3) == 0 && aligned16(x) && aligned16(out);
  const int64_t total = batch * per;
  hipLaunchKernelGGL(ig_perturb_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), a, x, (long)batch,
                     rep, rows, width, vec, out);
  return check_launch("ig_perturb_rows_kernel");
}

extern "C" int kgcn_ig_perturb_values_f32(const int32_t* rowptr, int32_t num_graphs, int32_t rows, int64_t nnz,
                                          int32_t max_nnz_per_graph, const float* values, const float* scale, const float* sigma,
                                          const int32_t* sample, const int32_t* ids, uint32_t noise_stream, uint64_t seed, float* out,
                                          void* stream) {
  const char* who = "kgcn_ig_perturb_values_f32";
  if (num_graphs < 0 || rows < 0 || nnz < 0) return fail("%s: negative size", who);
  if ((int64_t)num_graphs * rows >= (int64_t)INT32_MAX || nnz >= (int64_t)INT32_MAX) return fail("%s: batch exceeds int32 offsets", who);
  if (num_graphs == 0 || nnz == 0) return 0;
  PerturbArgs a;
  if (int rc = perturb_args(scale, sigma, sample, ids, noise_stream, seed, who, a)) return rc;
  if (!rowptr || !values || !out) return fail("%s: NULL operand", who);
  // slices per graph: a hint only (the kernel strides over whatever it is given)
  const int64_t blocks = ((int64_t)(max_nnz_per_graph > 0 ? max_nnz_per_graph : 0) + 3) / 4;
  int64_t slices = (blocks + 255) / 256;
  slices = slices < 1 ? 1 : (slices > 64 ? 64 : slices);
  hipLaunchKernelGGL(ig_perturb_values_kernel, dim3((unsigned)num_graphs, (unsigned)slices), dim3(256), 0, as_stream(stream), a, rowptr,
                     rows, (long)nnz, values, out);
  return check_launch("ig_perturb_values_kernel");
}
