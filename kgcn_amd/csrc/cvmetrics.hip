// Binary-classification metrics of all tasks in one call (gcn.py:170-256, compute_metrics: roc_curve + auc,
// average_precision_score and the confusion counts at score > threshold), as exact integers plus one fp64 sum per task.
//
//   key      one 64-bit key per used element: task << 33 | ~ordered(score) << 1 | label.  ordered() is the order-preserving
//            uint32 image of a float with -0.0 mapped onto +0.0 (scikit-learn ties them); its complement makes an ASCENDING
//            sort put every task's scores in descending order.  A masked-out element gets task = T and sorts behind all tasks.
//   sort     one rocprim::radix_sort_keys over the n T keys, bits [0, 33 + bits(T)).
//   scan     one workgroup per task: its segment by binary search, P / TP / FP / non-finite counts by one strided pass, then a
//            walk over the segment in chunks of kChunk elements.  A tie group (equal scores = one threshold of the curves) ends
//            where the next score differs; at a group end
//              tp_g, fp_g     = inclusive prefix counts (a block prefix sum of the labels + the running count),
//              tp_g-1, fp_g-1 = the exclusive counts at the group's start (a block max-scan finds the start; a group that
//                               began in an earlier chunk takes them from the carry),
//              auc_num2 += (fp_g - fp_g-1) (tp_g + tp_g-1)                         integers: AUC = auc_num2 / (2 P N)
//              ap       += ((tp_g - tp_g-1) / P) (tp_g / (tp_g + fp_g))            fp64
//            The AP terms of a chunk are added by one fixed tree (wave shuffles, then the four wave sums in order) and the
//            chunk sums serially in descending-threshold order: two runs agree bit for bit.  The stage writes its outputs
//            once per task and uses no atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include "block_reduce.h"
#include "workspace.h"

namespace kgcn {
namespace {

constexpr int kBlock = 256;
constexpr int kItems = 4;                     // consecutive elements per thread
constexpr int kChunk = kBlock * kItems;
constexpr int kWaves = kBlock / kWave;
typedef unsigned long long u64;

// all on the bits: the order of finite floats, denormals included, whatever the denormal mode of the float compares
__device__ __forceinline__ uint32_t ordered(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) return 0x80000000u;                      // -0.0 and +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_ordered(u64 key) { return ~(uint32_t)(key >> 1); }
__device__ __forceinline__ bool ordered_nonfinite(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return (u & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(kBlock) void metrics_key_kernel(const float* __restrict__ score, long ld, const float* __restrict__ label,
                                                             const float* __restrict__ mask, long n, int T, u64* __restrict__ keys) {
  const long m = n * T;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) {
    const long r = i / T;
    const int t = (int)(i - r * T);
    u64 key = (u64)(unsigned)T << 33;
    if (!mask || mask[i] != 0.f)
      key = ((u64)(unsigned)t << 33) | ((u64)(~ordered(score[r * ld + t])) << 1) | (label[i] != 0.f ? 1ull : 0ull);
    keys[i] = key;
  }
}

// first position whose task field is >= t
__device__ __forceinline__ long task_begin(const u64* __restrict__ keys, long m, unsigned t) {
  long lo = 0, hi = m;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((unsigned)(keys[mid] >> 33) < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// out [T, 8] int64: n_used, P, TP, FP (score > threshold), n_nonfinite, auc_num2, n_groups, 0;  ap [T] fp64
__global__ __launch_bounds__(kBlock) void metrics_scan_kernel(const u64* __restrict__ keys, long m, float threshold,
                                                              long long* __restrict__ out, double* __restrict__ ap_out) {
  __shared__ u64 red[kBlock];
  __shared__ long seg[2];
  __shared__ int ex[kChunk];                  // positives of the chunk in front of each element
  __shared__ int wsum[kWaves], wmax[kWaves];
  __shared__ double wap[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const unsigned task = blockIdx.x;
  if (tid == 0) {
    seg[0] = task_begin(keys, m, task);
    seg[1] = task_begin(keys, m, task + 1);
  }
  __syncthreads();
  const long s = seg[0], e = seg[1];

  const uint32_t thr = ordered(threshold);
  u64 cp = 0, ctp = 0, cfp = 0, cnf = 0;
  for (long p = s + tid; p < e; p += kBlock) {
    const u64 key = keys[p];
    const uint32_t v = key_ordered(key);
    const bool pos = key & 1ull;
    cp += pos ? 1 : 0;
    if (ordered_nonfinite(v)) ++cnf;
    if (v > thr) {
      ctp += pos ? 1 : 0;
      cfp += pos ? 0 : 1;
    }
  }
  const u64 P = block_sum(cp, red);
  const u64 TP = block_sum(ctp, red);
  const u64 FP = block_sum(cfp, red);
  const u64 NF = block_sum(cnf, red);
  const double Pd = (double)P;

  // carries, the same in every thread
  u64 tp_run = 0;                             // positives in front of the chunk
  u64 tp_prev = 0, fp_prev = 0;               // counts in front of the tie group that is open at the chunk's start
  double ap = 0.0;
  u64 auc = 0, groups = 0;                    // per thread; summed at the end (integers: any order is exact)
  for (long base = s; base < e; base += kChunk) {
    const long p0 = base + (long)tid * kItems;
    u64 k[kItems + 2];                        // the thread's elements with one neighbour on either side
#pragma unroll
    for (int q = 0; q < kItems + 2; ++q) {
      const long p = p0 - 1 + q;
      k[q] = (p >= s && p < e) ? keys[p] : ~0ull;             // never a key: a task field is at most KGCN_BINARY_METRICS_MAX_TASKS
    }
    int lab[kItems], start[kItems];
    bool end[kItems];
    int tsum = 0, tmax = -1;
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const bool valid = p0 + q < e;
      lab[q] = valid ? (int)(k[q + 1] & 1ull) : 0;
      end[q] = valid && (k[q + 2] >> 1) != (k[q + 1] >> 1);
      start[q] = valid && (k[q] >> 1) != (k[q + 1] >> 1) ? tid * kItems + q : -1;
      tsum += lab[q];
      tmax = max(tmax, start[q]);
    }
    // inclusive scans over the threads of a wave: positives (sum) and the latest group start (max)
    int isum = tsum, imax = tmax;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int us = __shfl_up(isum, off), um = __shfl_up(imax, off);
      if (lane >= off) {
        isum += us;
        imax = max(imax, um);
      }
    }
    if (lane == kWave - 1) {
      wsum[wv] = isum;
      wmax[wv] = imax;
    }
    int xmax = __shfl_up(imax, 1);            // exclusive max over the wave
    if (lane == 0) xmax = -1;
    __syncthreads();
    int xsum = isum - tsum, csum = 0, cmax = -1;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wv) {
        xsum += wsum[w];
        xmax = max(xmax, wmax[w]);
      }
      csum += wsum[w];
      cmax = max(cmax, wmax[w]);
    }
    int incl[kItems], from[kItems];
    {
      int run = xsum, j = xmax;
#pragma unroll
      for (int q = 0; q < kItems; ++q) {
        ex[tid * kItems + q] = run;
        run += lab[q];
        incl[q] = run;
        if (start[q] >= 0) j = start[q];
        from[q] = j;
      }
    }
    __syncthreads();
    double term = 0.0;
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      if (end[q]) {
        const u64 tp_g = tp_run + (u64)incl[q];
        const u64 fp_g = (u64)(p0 + q - s + 1) - tp_g;
        u64 tp_b = tp_prev, fp_b = fp_prev;
        if (from[q] >= 0) {
          tp_b = tp_run + (u64)ex[from[q]];
          fp_b = (u64)(base + from[q] - s) - tp_b;
        }
        auc += (fp_g - fp_b) * (tp_g + tp_b);
        ++groups;
        if (P) term += ((double)(tp_g - tp_b) / Pd) * ((double)tp_g / (double)(tp_g + fp_g));
      }
    }
    // the open group at the chunk's end started at cmax (or before the chunk: the carry stands)
    if (cmax >= 0) {
      tp_prev = tp_run + (u64)ex[cmax];
      fp_prev = (u64)(base + cmax - s) - tp_prev;
    }
    tp_run += (u64)csum;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) term += __shfl_down(term, off);
    if (lane == 0) wap[wv] = term;
    __syncthreads();
    double chunk = wap[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) chunk += wap[w];
    ap += chunk;
  }
  const u64 auc_all = block_sum(auc, red);
  const u64 groups_all = block_sum(groups, red);
  if (tid == 0) {
    long long* o = out + (long)task * 8;
    o[0] = (long long)(e - s);
    o[1] = (long long)P;
    o[2] = (long long)TP;
    o[3] = (long long)FP;
    o[4] = (long long)NF;
    o[5] = (long long)auc_all;
    o[6] = (long long)groups_all;
    o[7] = 0;
    ap_out[task] = ap;
  }
}

int end_bit_of(int32_t tasks) {
  int bits = 0;
  while ((1ll << bits) <= (long long)tasks) ++bits;      // the task field holds 0 .. tasks
  return 33 + bits;
}

size_t sort_temp_bytes(size_t m, int end_bit) {
  size_t b = 0;
  (void)rocprim::radix_sort_keys(nullptr, b, (u64*)nullptr, (u64*)nullptr, m, 0u, (unsigned)end_bit, (hipStream_t)0);
  return b;
}

struct Layout {
  u64 *keys, *sorted;
  void* temp;
  size_t temp_bytes, total;
};
Layout layout(unsigned char* base, int64_t m, int32_t tasks) {
  Layout o{};
  Taker t{base};
  o.keys = t.take<u64>((size_t)m);
  o.sorted = t.take<u64>((size_t)m);
  o.temp_bytes = sort_temp_bytes((size_t)m, end_bit_of(tasks));
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

int check_shape(const char* who, int64_t n, int32_t tasks) {
  if (n < 1 || tasks < 1 || tasks > KGCN_BINARY_METRICS_MAX_TASKS)
    return fail("%s: bad shape n=%lld tasks=%d (1..%d tasks)", who, (long long)n, tasks, KGCN_BINARY_METRICS_MAX_TASKS);
  if (n > KGCN_BINARY_METRICS_MAX_ELEMENTS || n * (int64_t)tasks > KGCN_BINARY_METRICS_MAX_ELEMENTS)
    return fail("%s: %lld x %d elements exceed %lld", who, (long long)n, tasks, (long long)KGCN_BINARY_METRICS_MAX_ELEMENTS);
  return 0;
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_binary_metrics_workspace_bytes(int64_t n, int32_t tasks) {
  if (check_shape("kgcn_binary_metrics_workspace_bytes", n, tasks)) return -1;
  return (int64_t)layout(nullptr, n * tasks, tasks).total;
}

extern "C" int kgcn_binary_metrics_f32(const float* score, int64_t score_ld, const float* label, const float* mask, int64_t n,
                                       int32_t tasks, float threshold, int64_t* counts, double* ap, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_binary_metrics_f32";
  if (int rc = check_shape(who, n, tasks)) return rc;
  if (score_ld < tasks) return fail("%s: score_ld %lld < %d tasks", who, (long long)score_ld, tasks);
  if (threshold != threshold) return fail("%s: the threshold is NaN", who);
  if (!score || !label || !counts || !ap) return fail("%s: NULL operand", who);
  const int64_t m = n * tasks;
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)layout(nullptr, m, tasks).total)) return rc;
  hipStream_t s = as_stream(stream);
  const Layout o = layout(aligned_base(workspace), m, tasks);
  long blocks = (long)((m + kBlock - 1) / kBlock);
  if (blocks > 8L * kNumCU) blocks = 8L * kNumCU;
  hipLaunchKernelGGL(metrics_key_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, score, (long)score_ld, label, mask, (long)n,
                     tasks, o.keys);
  if (int rc = check_launch(who)) return rc;
  size_t temp = o.temp_bytes;
  if (rocprim::radix_sort_keys(o.temp, temp, o.keys, o.sorted, (size_t)m, 0u, (unsigned)end_bit_of(tasks), s) != hipSuccess)
    return fail("%s: rocprim::radix_sort_keys failed", who);
  hipLaunchKernelGGL(metrics_scan_kernel, dim3((unsigned)tasks), dim3(kBlock), 0, s, o.sorted, (long)m, threshold,
                     reinterpret_cast<long long*>(counts), ap);
  return check_launch(who);
}
