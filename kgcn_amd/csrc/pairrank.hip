// Ranking of all node pairs of the link-prediction model (sample_kg/network_prediction/script/predscore.py: the score-ordered
// list of run_enrichment.sh, its train / test / new marks and the enrichment counts) without the [N, N] score matrix.
//
//   score    s_ij = sum_k (h[i,k] w[k]) h[j,k] for i < j, fp32 on v_mfma_f32_32x32x2_f32, k ascending; the row operand is scaled
//            by w (one rounding) while it is staged, w = NULL for gcn / ip.  A 256-thread workgroup owns a 64 x 64 tile of
//            the upper triangle (tile pairs ti <= tj only, decoded from the linear block index), each wave a 32 x 32 block with
//            one accumulator chain; K runs through LDS in chunks of 32 (row stride 33 floats: the operand reads of a 32-lane
//            group and the staging writes both fall on 32 distinct banks).  Every pass below recomputes the tiles with this one
//            routine, so a pair has the same bits in all of them.
//   order    predscore.py:153 sorts (score, row, col) tuples in reverse: score, then row, then col, all descending.  A score
//            becomes an order-preserving uint32 key (-0.0 counts as +0.0, as Python compares them equal; NaN -> key 0: below
//            every number, -inf included -- Python's order with a NaN in the list is undefined, this one is defined), and
//            key << 32 | row << 16 | col is that order under ONE descending radix sort.  The composite is unique per pair, so
//            the sorted list does not depend on the order the candidates were appended in.  16 bits an index: N <= 65,536.
//   select   radix select of the key T of the cutoff-th largest score: three passes over the key bits (11 / 11 / 10).  Each
//            histograms the current digit of the keys that match the digits chosen so far -- in LDS with integer atomics,
//            non-empty bins flushed to the global histogram with integer atomics -- and a one-workgroup kernel picks the bin
//            and clears the histogram.  The host is not involved between the passes.
//   emit     recomputes the tiles, appends the composite of every pair with key >= T (count(key > T) + count(key == T) of them,
//            what select reported) at a wave-aggregated integer counter, never past the capacity; sorts; unpacks the first
//            `cutoff` entries.  The call reads the counter back and fails when it disagrees with the capacity.
//   table    convert / process_table / enrichment of predscore.py:194-280 on the sorted list: membership of row << 16 | col in
//            the sorted target (train + test) and test code arrays by binary search, score_ranking = 1 + the entries with a
//            strictly larger key (= len - rankdata(max) + 1), an exclusive scan of the non-train marks (rocPRIM) for the
//            position in the table without train edges, and integer counts of the test entries below each threshold.
// No float atomics anywhere: every output is bitwise reproducible.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "workspace.h"

namespace kgcn {

namespace {
constexpr int kTile = 64;            // output tile edge of a workgroup
constexpr int kKc = 32;              // K chunk staged in LDS
constexpr int kLd = kKc + 1;         // LDS row stride (floats)
constexpr int kBins = 2048;          // bins of the widest digit
constexpr int kMaxTop = KGCN_PAIRRANK_MAX_TOP;

__host__ __device__ __forceinline__ int digit_bits(int pass) { return pass == 2 ? 10 : 11; }
__host__ __device__ __forceinline__ int digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }

struct State {
  unsigned long long prefix;         // the digits chosen so far (high bits of T)
  long long remaining;               // rank still to find among the keys that match the prefix (1-based)
  long long count_gt;                // keys above every key that matches the prefix
  unsigned long long appended;       // emit's counter
};

__device__ __forceinline__ uint32_t score_key(float v) {
  if (v != v) return 0u;
  if (v == 0.0f) return 0x80000000u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t key) {
  if (key == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// the wave's 32 x 32 block of tile (ti, tj): acc[r] is pair (ti 64 + wr 32 + (r & 3) + 8 (r >> 2) + 4 hi, tj 64 + wc 32 + li)
__device__ __forceinline__ f32x16 score_block(const float* __restrict__ h, const float* __restrict__ w, int N, int D, int ti, int tj,
                                              float* as, float* bs) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, hi = lane >> 5, wr = wv >> 1, wc = wv & 1;
  const bool live = !(ti == tj && wr > wc);            // below the diagonal: nothing to score
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int kk = tid & (kKc - 1);
  const float* xa = as + (wr * 32 + li) * kLd + hi;
  const float* xb = bs + (wc * 32 + li) * kLd + hi;
  for (int k0 = 0; k0 < D; k0 += kKc) {
    const int k = k0 + kk;
    const float wk = (w && k < D) ? w[k] : 1.0f;
    for (int r = tid >> 5; r < kTile; r += 8) {
      const long gi = (long)ti * kTile + r, gj = (long)tj * kTile + r;
      float a = 0.f, b = 0.f;
      if (k < D) {
        if (gi < N) a = w ? __fmul_rn(h[gi * D + k], wk) : h[gi * D + k];
        if (gj < N) b = h[gj * D + k];
      }
      as[r * kLd + kk] = a;
      bs[r * kLd + kk] = b;
    }
    __syncthreads();
    if (live) {
      const int steps = (min(kKc, D - k0) + 1) >> 1;   // an odd tail multiplies the chunk's zero padding
      for (int s = 0; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], xb[2 * s], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  return acc;
}

struct TileArgs {
  const float* h;
  const float* w;
  State* st;
  unsigned* hist;
  const long long* counts;           // emit: T, count(key > T), count(key == T)
  unsigned long long* cand;
  long long capacity;
  int N, D, pass;
};

// MODE 0: one histogram pass of the select; MODE 1: emit
template <int MODE>
__global__ __launch_bounds__(256) void pair_tile_kernel(TileArgs a) {
  __shared__ float as[kTile * kLd], bs[kTile * kLd];
  __shared__ unsigned lh[MODE == 0 ? kBins : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, hi = lane >> 5, wr = wv >> 1, wc = wv & 1;
  int ti, tj;
  tile_of((long)blockIdx.x, ti, tj);
  if (MODE == 0)
    for (int q = tid; q < kBins; q += 256) lh[q] = 0u;   // ordered before the atomics by score_block's barriers
  const f32x16 acc = score_block(a.h, a.w, a.N, a.D, ti, tj, as, bs);
  const int j = tj * kTile + wc * 32 + li;
  const int i0 = ti * kTile + wr * 32 + 4 * hi;
  if (MODE == 0) {
    const int shift = digit_shift(a.pass), bits = digit_bits(a.pass);
    const uint32_t prefix = (uint32_t)a.st->prefix;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + (r & 3) + 8 * (r >> 2);
      if (i < j && j < a.N) {
        const uint32_t key = score_key(acc[r]);
        if (a.pass == 0 || (key >> (shift + bits)) == prefix) atomicAdd(&lh[(key >> shift) & ((1u << bits) - 1u)], 1u);
      }
    }
    __syncthreads();
    for (int q = tid; q < kBins; q += 256)
      if (lh[q]) atomicAdd(&a.hist[q], lh[q]);
  } else {
    const uint32_t T = (uint32_t)a.counts[0];
    unsigned long long mine[16];
    unsigned taken = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + (r & 3) + 8 * (r >> 2);
      const uint32_t key = score_key(acc[r]);
      mine[r] = ((unsigned long long)key << 32) | ((unsigned long long)(unsigned)i << 16) | (unsigned long long)(unsigned)j;
      if (i < j && j < a.N && key >= T) taken |= 1u << r;
    }
    const int n = __popc(taken);
    // the wave's entries get one contiguous range: inclusive scan of the lane counts, one atomic by the last lane
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    const int total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (lane == 63 && total > 0) base = atomicAdd(&a.st->appended, (unsigned long long)total);
    base = __shfl(base, 63);
    unsigned long long at = base + (unsigned long long)(incl - n);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (taken & (1u << r)) {
        if (at < (unsigned long long)a.capacity) a.cand[at] = mine[r];   // a full buffer drops the entry; the counter tells
        ++at;
      }
    }
  }
}

// one workgroup: the bin that holds the `remaining`-th largest matching key, bins taken from the top; clears the histogram
__global__ __launch_bounds__(256) void pair_pick_kernel(State* st, unsigned* hist, int pass, long long cutoff, long long* out) {
  __shared__ unsigned long long part[256];
  const int t = threadIdx.x, bits = digit_bits(pass), nb = 1 << bits, per = nb / 256;
  unsigned long long s = 0;
  for (int q = 0; q < per; ++q) s += hist[nb - 1 - (t * per + q)];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    const long long rem = pass == 0 ? cutoff : st->remaining;
    unsigned long long cum = 0;
    int c = 0;
    while (c < 255 && cum + part[c] < (unsigned long long)rem) cum += part[c++];
    int q = 0;
    while (q < per - 1 && cum + hist[nb - 1 - (c * per + q)] < (unsigned long long)rem) cum += hist[nb - 1 - (c * per + q++)];
    const int bin = nb - 1 - (c * per + q);
    const unsigned long long prefix = ((pass == 0 ? 0ull : st->prefix) << bits) | (unsigned long long)bin;
    const long long gt = (pass == 0 ? 0ll : st->count_gt) + (long long)cum;
    st->prefix = prefix;
    st->remaining = rem - (long long)cum;
    st->count_gt = gt;
    if (pass == 2) {
      out[0] = (long long)prefix;
      out[1] = gt;
      out[2] = (long long)hist[bin];
    }
  }
  __syncthreads();
  for (int q = t; q < kBins; q += 256) hist[q] = 0u;
}

__global__ __launch_bounds__(256) void pair_unpack_kernel(const unsigned long long* __restrict__ sorted, long n,
                                                          float* __restrict__ score, int32_t* __restrict__ row,
                                                          int32_t* __restrict__ col) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const unsigned long long c = sorted[p];
  score[p] = key_score((uint32_t)(c >> 32));
  row[p] = (int32_t)((c >> 16) & 0xffffull);
  col[p] = (int32_t)(c & 0xffffull);
}

// ---- the table ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool has_code(const uint32_t* __restrict__ codes, long n, uint32_t x) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (codes[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && codes[lo] == x;
}

struct TableArgs {
  const float* score;
  const int32_t* row;
  const int32_t* col;
  const uint32_t* target;
  const uint32_t* test;
  uint8_t* train_edge;
  uint8_t* test_edge;
  uint8_t* new_edge;
  long long* ranking;
  int* nontrain;
  const int* pos;
  unsigned long long* hits;
  long long* covered;
  long n, ntarget, ntest;
  long long top[kMaxTop];
  int ntop;
};

__global__ __launch_bounds__(256) void pair_mark_kernel(TableArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t code = ((uint32_t)a.row[p] << 16) | ((uint32_t)a.col[p] & 0xffffu);
  const bool te = has_code(a.test, a.ntest, code);
  const bool tr = !te && has_code(a.target, a.ntarget, code);
  a.train_edge[p] = tr ? 1 : 0;
  a.test_edge[p] = te ? 1 : 0;
  a.new_edge[p] = (tr || te) ? 0 : 1;
  a.nontrain[p] = tr ? 0 : 1;
  // the first entry of this entry's tie group: the list is in descending key order
  const uint32_t key = score_key(a.score[p]);
  long lo = 0, hi = p;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (score_key(a.score[mid]) > key) lo = mid + 1;
    else hi = mid;
  }
  a.ranking[p] = (long long)lo + 1;
}

__global__ __launch_bounds__(256) void pair_hits_kernel(TableArgs a) {
  __shared__ unsigned cnt[kMaxTop];
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < kMaxTop) cnt[threadIdx.x] = 0u;
  __syncthreads();
  if (p < a.n) {
    const long long at = a.pos[p];
    if (a.test_edge[p])
      for (int q = 0; q < a.ntop; ++q)
        if (at < a.top[q]) atomicAdd(&cnt[q], 1u);
    if (p == a.n - 1) {
      const long long kept = at + a.nontrain[p];
      for (int q = 0; q < a.ntop; ++q) a.covered[q] = kept >= a.top[q] ? 1 : 0;
    }
  }
  __syncthreads();
  if (threadIdx.x < a.ntop && cnt[threadIdx.x]) atomicAdd(&a.hits[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

size_t sort_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::radix_sort_keys_desc(nullptr, b, (unsigned long long*)nullptr, (unsigned long long*)nullptr, n, 0u, 64u,
                                      (hipStream_t)0);
  return b;
}
size_t scan_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>(), (hipStream_t)0);
  return b;
}

struct Layout {
  State* st;
  unsigned* hist;
  unsigned long long *cand, *sorted;
  void* temp;
  size_t temp_bytes, total;
};
Layout rank_layout(unsigned char* base, long long capacity) {
  Layout o{};
  Taker t{base};
  o.st = t.take<State>(1);
  o.hist = t.take<unsigned>(kBins);
  o.cand = t.take<unsigned long long>((size_t)capacity);
  o.sorted = t.take<unsigned long long>((size_t)capacity);
  o.temp_bytes = capacity > 0 ? sort_temp_bytes((size_t)capacity) : 0;
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

struct TableLayout {
  int *nontrain, *pos;
  void* temp;
  size_t temp_bytes, total;
};
TableLayout table_layout(unsigned char* base, long long n) {
  TableLayout o{};
  Taker t{base};
  o.nontrain = t.take<int>((size_t)n);
  o.pos = t.take<int>((size_t)n);
  o.temp_bytes = n > 0 ? scan_temp_bytes((size_t)n) : 0;
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

int check_shape(const char* who, int32_t nodes, int32_t dim) {
  if (nodes < 2 || nodes > KGCN_PAIRRANK_MAX_NODES) return fail("%s: %d nodes outside 2..%d", who, nodes, KGCN_PAIRRANK_MAX_NODES);
  if (dim < 1 || dim > KGCN_LP_MAX_DIM) return fail("%s: dim %d outside 1..%d", who, dim, KGCN_LP_MAX_DIM);
  return 0;
}
long long all_pairs(int32_t nodes) { return (long long)nodes * (nodes - 1) / 2; }
// the entries asked for: 0 or more than there are means all
long long entries_of(int32_t nodes, int64_t cutoff) {
  const long long total = all_pairs(nodes);
  return cutoff == 0 || cutoff > total ? total : (long long)cutoff;
}
unsigned tile_blocks(int32_t nodes) {
  const unsigned nt = (unsigned)((nodes + kTile - 1) / kTile);
  return nt * (nt + 1) / 2;
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_pair_rank_workspace_bytes(int32_t nodes, int32_t dim, int64_t capacity, int64_t entries) {
  const char* who = "kgcn_pair_rank_workspace_bytes";
  if (check_shape(who, nodes, dim)) return -1;
  if (capacity < 0 || capacity > KGCN_PAIRRANK_MAX_CANDIDATES)
    return refuse_query("%s: %lld candidates outside 0..%d", who, (long long)capacity, KGCN_PAIRRANK_MAX_CANDIDATES);
  if (entries < 0 || entries > KGCN_PAIRRANK_MAX_CANDIDATES)
    return refuse_query("%s: %lld table entries outside 0..%d", who, (long long)entries, KGCN_PAIRRANK_MAX_CANDIDATES);
  const size_t a = rank_layout(nullptr, capacity).total, b = table_layout(nullptr, entries).total;
  return (int64_t)(a > b ? a : b);
}

extern "C" int kgcn_pair_rank_select_f32(const float* h, int32_t nodes, int32_t dim, const float* w, int64_t cutoff, int64_t* counts,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_pair_rank_select_f32";
  if (int rc = check_shape(who, nodes, dim)) return rc;
  if (cutoff < 0) return fail("%s: negative cutoff %lld", who, (long long)cutoff);
  if (!h || !counts) return fail("%s: NULL operand", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)rank_layout(nullptr, 0).total)) return rc;
  hipStream_t s = as_stream(stream);
  const Layout o = rank_layout(aligned_base(workspace), 0);
  if (int rc = zero_async(who, o.st, al256(sizeof(State)) + kBins * sizeof(unsigned), s)) return rc;   // the state and the histogram
  const long long k = entries_of(nodes, cutoff);
  for (int pass = 0; pass < 3; ++pass) {
    TileArgs a{h, w, o.st, o.hist, nullptr, nullptr, 0, nodes, dim, pass};
    hipLaunchKernelGGL(pair_tile_kernel<0>, dim3(tile_blocks(nodes)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pair_pick_kernel, dim3(1), dim3(256), 0, s, o.st, o.hist, pass, k, reinterpret_cast<long long*>(counts));
  }
  return check_launch(who);
}

extern "C" int kgcn_pair_rank_emit_f32(const float* h, int32_t nodes, int32_t dim, const float* w, int64_t cutoff,
                                       const int64_t* counts, int64_t capacity, float* score, int32_t* row, int32_t* col,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_pair_rank_emit_f32";
  if (int rc = check_shape(who, nodes, dim)) return rc;
  if (cutoff < 0) return fail("%s: negative cutoff %lld", who, (long long)cutoff);
  if (!h || !counts || !score || !row || !col) return fail("%s: NULL operand", who);
  const long long k = entries_of(nodes, cutoff);
  if (capacity < k || capacity > KGCN_PAIRRANK_MAX_CANDIDATES)
    return fail("%s: capacity %lld outside %lld..%d (the %lld entries asked for .. KGCN_PAIRRANK_MAX_CANDIDATES)", who,
                (long long)capacity, k, KGCN_PAIRRANK_MAX_CANDIDATES, k);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)rank_layout(nullptr, capacity).total)) return rc;
  hipStream_t s = as_stream(stream);
  const Layout o = rank_layout(aligned_base(workspace), capacity);
  if (int rc = zero_async(who, &o.st->appended, sizeof(unsigned long long), s)) return rc;
  TileArgs a{h, w, o.st, o.hist, reinterpret_cast<const long long*>(counts), o.cand, (long long)capacity, nodes, dim, 0};
  hipLaunchKernelGGL(pair_tile_kernel<1>, dim3(tile_blocks(nodes)), dim3(256), 0, s, a);
  if (int rc = check_launch(who)) return rc;
  // the counter decides whether the buffer holds every candidate: the one read-back of this call
  unsigned long long appended = 0;
  if (hipMemcpyAsync(&appended, &o.st->appended, sizeof(appended), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail("%s: reading the candidate count failed: %s", who, hipGetErrorString(hipGetLastError()));
  if (appended > (unsigned long long)capacity)
    return fail("%s: %llu candidates do not fit the capacity %lld (nothing was written past it)", who, appended, (long long)capacity);
  if (appended < (unsigned long long)k)
    return fail("%s: %llu candidates for %lld entries (counts not from kgcn_pair_rank_select_f32 of these operands?)", who,
                appended, k);
  size_t temp = sort_temp_bytes((size_t)appended);
  if (temp > o.temp_bytes) return fail("%s: sort scratch %zu > %zu bytes", who, temp, o.temp_bytes);
  if (rocprim::radix_sort_keys_desc(o.temp, temp, o.cand, o.sorted, (size_t)appended, 0u, 64u, s) != hipSuccess)
    return fail("%s: rocprim::radix_sort_keys_desc failed", who);
  hipLaunchKernelGGL(pair_unpack_kernel, dim3(blocks_of((long)k)), dim3(256), 0, s, o.sorted, (long)k, score, row, col);
  return check_launch(who);
}

extern "C" int kgcn_pair_rank_table_i32(const float* score, const int32_t* row, const int32_t* col, int64_t entries,
                                        const uint32_t* target_codes, int64_t num_target, const uint32_t* test_codes,
                                        int64_t num_test, const int64_t* top_ratio, int32_t num_top, uint8_t* train_edge,
                                        uint8_t* test_edge, uint8_t* new_edge, int64_t* score_ranking, int64_t* hits,
                                        int64_t* covered, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_pair_rank_table_i32";
  if (entries < 1 || entries > KGCN_PAIRRANK_MAX_CANDIDATES)
    return fail("%s: %lld entries outside 1..%d", who, (long long)entries, KGCN_PAIRRANK_MAX_CANDIDATES);
  if (num_target < 0 || num_test < 0 || num_target >= (int64_t)INT32_MAX || num_test >= (int64_t)INT32_MAX)
    return fail("%s: %lld target / %lld test codes", who, (long long)num_target, (long long)num_test);
  if (num_top < 0 || num_top > kMaxTop) return fail("%s: %d thresholds outside 0..%d", who, num_top, kMaxTop);
  if (!score || !row || !col || !train_edge || !test_edge || !new_edge || !score_ranking || (num_target > 0 && !target_codes) ||
      (num_test > 0 && !test_codes) || (num_top > 0 && (!top_ratio || !hits || !covered)))
    return fail("%s: NULL operand", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)table_layout(nullptr, entries).total)) return rc;
  hipStream_t s = as_stream(stream);
  const TableLayout o = table_layout(aligned_base(workspace), entries);
  TableArgs a{score, row, col, target_codes, test_codes, train_edge, test_edge, new_edge, reinterpret_cast<long long*>(score_ranking),
              o.nontrain, o.pos, reinterpret_cast<unsigned long long*>(hits), reinterpret_cast<long long*>(covered),
              (long)entries, (long)num_target, (long)num_test, {}, num_top};
  for (int q = 0; q < num_top; ++q) a.top[q] = top_ratio[q];
  const unsigned nb = blocks_of((long)entries);
  hipLaunchKernelGGL(pair_mark_kernel, dim3(nb), dim3(256), 0, s, a);
  size_t temp = o.temp_bytes;
  if (rocprim::exclusive_scan(o.temp, temp, o.nontrain, o.pos, 0, (size_t)entries, rocprim::plus<int>(), s) != hipSuccess)
    return fail("%s: rocprim::exclusive_scan failed", who);
  if (num_top > 0) {
    if (int rc = zero_async(who, hits, (size_t)num_top * sizeof(int64_t), s)) return rc;
    hipLaunchKernelGGL(pair_hits_kernel, dim3(nb), dim3(256), 0, s, a);
  }
  return check_launch(who);
}
