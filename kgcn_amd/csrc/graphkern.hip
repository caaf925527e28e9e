// Classical graph kernels of graph_kernel/gk.py on the device: Weisfeiler-Lehman subtree features, shortest-path features and the
// Gram matrix over them (kgcn_amd/graph_kernel.py).  Everything here is integer-exact and bitwise reproducible.
//
//   input    a plain (row_pad == 0) kgcn_csr_batch of T graphs x M padded rows, num_nodes [T] and dense-rank node labels [T*M].
//            Rows >= num_nodes[t] do not exist; stored values are ignored, every stored entry is one edge occurrence (a repeated
//            entry is a multi-edge).  An entry whose column is no node of its graph (num_nodes <= column < M) is not the same to
//            the two feature kernels: the shortest-path search ignores it; the refinement counts it in the degree and takes the
//            colour the colour array holds at that column, -1 from the drivers, into the signature.  GraphSet, the public driver,
//            refuses such input; tests/test_gpu_graph_kernel_ops.py holds each kernel to its half (cases `directed`, wl_direct).
//   runs     both feature kernels end in (column u64, graph i32, count i32), one run per (feature, graph) with a non-zero count.
//            A call with run_col == NULL counts the runs of every graph and scans the counts into run_ptr [T + 1]; the call with
//            the buffers writes graph t's runs at run_ptr[t], in ascending column order: no atomics, the list is reproducible.
//   refine   the signature of a node is (own colour, sorted multiset of its neighbours' colours).  Eight lanes share a row: every
//            entry's place in the sorted list is the count of entries before it (value, then position: any degree works), the
//            list goes to sorted_nbr [nnz], and the row's 128-bit key is two independent 64-bit mixes of (own colour, degree,
//            sum over the neighbours of a mixed colour): a sum, so the key needs no order.  hash_mask is and-ed onto both words.
//   rank     two stable 64-bit radix passes (low word, then high word) carry the row index; a row opens a new colour when its
//            key differs from its predecessor's; an inclusive scan of those flags is the dense colour.  Where two neighbours
//            in that order have EQUAL keys their true signatures are compared, and every difference is counted (integer atomic):
//            the caller refuses a non-zero count, so a partition is exact or refused, never silently merged.  Rows that do not
//            exist carry the all-ones key and the colour -1; existence is part of the compared signature.
//   wl runs  one workgroup per graph: its colours are sorted in LDS by counting, run-length encoded and emitted with the
//            iteration's column offset.
//   sp       one workgroup per graph, M <= 128: breadth-first search from every source (one thread a source, its queue and its
//            distance row in LDS: O(n + entries) a source; Floyd-Warshall in LDS measured 1.3x slower at 50 nodes and 1.75x at 128,
//            profiles/sp_bfs_vs_floyd_warshall.txt), then the n^2 keys label_k << 20 | label_j << 8 | distance (255 = unreachable) are sorted in LDS by a
//            bitonic network (64 KB of keys + 16 KB of distances at M = 128) and run-length encoded.
//   gram     the runs are sorted by column.  A column that occurs in one graph only touches K[g][g]: count^2 goes to an int64
//            diagonal by integer atomics (integer addition does not depend on order) and the column is never laid out.  The
//            other columns get dense indices by a scan and are laid out chunk_cols at a time as a [G_pad, chunk_cols] int32
//            count matrix, which v_mfma_f64_16x16x4_f64 multiplies with itself into the upper-triangle 64 x 64 tiles of K,
//            mirrored on store.  All summands are non-negative integers, so every partial sum is exact below 2^53: the result
//            has the bits of the reference's float64 csr.dot, in any order.  No float atomics.
//   norm     K_ij / sqrt(K_ii K_jj), 0 where a diagonal entry is 0: one f64 product, one correctly rounded sqrt and division.
//   copies   refine, rank, wl runs and sp also serve `copies` colourings of the same graphs in one launch sequence (graphkern.h;
//            the hash graph kernels of hashkern.hip): colours [copies, T*M] over the one stored batch.  Copies whose initial
//            colours are disjoint stay apart in the one global ranking.  copies == 1 is the plain kernel, bit for bit.
#include "gram_tile.h"
#include "graphkern.h"

namespace kgcn {
namespace {

constexpr int kGroup = 8;            // lanes that share a row in the refinement
constexpr int kSpMaxNodes = 128;     // distances and queue entries are bytes, n^2 keys fit the LDS
constexpr int kSpMaxLabels = 4096;   // 12 bits a label in the 32-bit key
constexpr int kWlRunsMaxNodes = 4096;

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// ---- refinement ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wl_refine_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cv,
                                                        const int32_t* __restrict__ num_nodes, const int32_t* __restrict__ colors,
                                                        int T, int M, int copies, long nnz, u64 mask,
                                                        int32_t* __restrict__ sorted, u64* __restrict__ key_hi,
                                                        u64* __restrict__ key_lo) {
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) / kGroup, stored = (long)T * M, rows = copies * stored;
  const int sub = threadIdx.x & (kGroup - 1);
  const bool in = row < rows;
  int beg = 0, deg = 0;
  long base = 0, out = 0;                                    // of the copy's colours of this graph, of its sorted lists
  bool exists = false;
  if (in) {
    const long c = copies > 1 ? row / stored : 0, p = row - c * stored;
    const int t = (int)(p / M);
    base = c * stored + (long)t * M;
    out = c * nnz;
    exists = (int)(p - (long)t * M) < num_nodes[t];
    beg = rowptr[p];
    deg = rowptr[p + 1] - beg;
  }
  auto colour_of = [&](int e) -> int32_t {
    const int32_t c = cv[2 * (long)(beg + e)];
    return (unsigned)c < (unsigned)M ? colors[base + c] : -2;
  };
  u64 s1 = 0, s2 = 0;
  for (int e = sub; e < deg; e += kGroup) {
    const int32_t c = colour_of(e);
    int pos = 0;
    for (int q = 0; q < deg; ++q) {
      const int32_t cq = colour_of(q);
      pos += (cq < c || (cq == c && q < e)) ? 1 : 0;
    }
    sorted[out + beg + pos] = c;
    s1 += mix64((u64)(uint32_t)c + 0x9e3779b97f4a7c15ull);
    s2 += mix64(((u64)(uint32_t)c << 1 | 1ull) * 0xd6e8feb86659fd93ull);
  }
#pragma unroll
  for (int off = 1; off < kGroup; off <<= 1) {
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
  }
  if (in && sub == 0) {
    const u64 own = (u64)(uint32_t)colors[row] << 32 | (u64)(uint32_t)deg;
    key_hi[row] = exists ? (mix64(s1 ^ mix64(own)) & mask) : ~0ull;
    key_lo[row] = exists ? (mix64(s2 + mix64(own ^ 0xa0761d6478bd642full)) & mask) : ~0ull;
  }
}

// Two rows that do not exist are one signature whatever the batch stores in them (entries, a colour): they share the all-ones
// key and get no colour.
struct RankArgs {
  const int32_t* rowptr;
  const int32_t* num_nodes;
  const int32_t* colors;
  const int32_t* sorted;
  const u64* key_hi;
  const u64* key_lo;
  const uint32_t* order;             // rows in (key_hi, key_lo) order
  u64* info;                         // colours, mismatches
  long nnz;
  uint32_t stored;                   // T * M
  int M;

  __device__ __forceinline__ bool exists(uint32_t row) const {
    const uint32_t p = row % stored, t = p / (uint32_t)M;
    return (int)(p - t * (uint32_t)M) < num_nodes[t];
  }
  // true signatures of two rows: existence, own colour, degree, sorted neighbour colours
  __device__ bool same_signature(uint32_t x, uint32_t y) const {
    const bool ex = exists(x);
    if (ex != exists(y)) return false;
    if (!ex) return true;
    if (colors[x] != colors[y]) return false;
    const uint32_t cx = x / stored, px = x - cx * stored, cy = y / stored, py = y - cy * stored;
    const int bx = rowptr[px], by = rowptr[py], d = rowptr[px + 1] - bx;
    if (rowptr[py + 1] - by != d) return false;
    const int32_t *sx = sorted + cx * nnz + bx, *sy = sorted + cy * nnz + by;
    for (int e = 0; e < d; ++e)
      if (sx[e] != sy[e]) return false;
    return true;
  }
  // equal keys; a pair of equal keys over different signatures is counted for the caller to refuse
  __device__ __forceinline__ bool same_as_prev(long p) const {
    const uint32_t row = order[p], prev = order[p - 1];
    const bool eq = key_hi[row] == key_hi[prev] && key_lo[row] == key_lo[prev];
    if (eq && !same_signature(row, prev)) atomicAdd(&info[1], 1ull);
    return eq;
  }
};

// ---- runs of a sorted key list in LDS -----------------------------------------------------------------------------------------
struct RunOut {
  long long* counts;                 // count mode: runs of every slot
  const long long* run_ptr;          // emit mode
  u64* col;
  int32_t* graph;
  int32_t* count;
  long long capacity;
  u64 offset, stride;                // column = offset + copy * stride + key
};

// s [n] ascending in LDS; part [256] LDS scratch.  All 256 threads call.  slot = copy * T + t.
__device__ void emit_runs(const uint32_t* s, int n, int slot, int t, u64 offset, const RunOut& o, int* part) {
  const int tid = threadIdx.x, per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
  int heads = 0;
  for (int p = lo; p < hi; ++p) heads += (p == 0 || s[p] != s[p - 1]) ? 1 : 0;
  part[tid] = heads;
  __syncthreads();
  int k = 0;
  for (int q = 0; q < tid; ++q) k += part[q];
  if (!o.col) {
    if (tid == 255) o.counts[slot] = (long long)(k + heads);
    return;
  }
  const long long base = o.run_ptr[slot];
  for (int p = lo; p < hi; ++p) {
    if (p != 0 && s[p] == s[p - 1]) continue;
    const uint32_t v = s[p];
    int a = p + 1, b = n;            // first position past the run of v
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (s[mid] <= v) a = mid + 1;
      else b = mid;
    }
    const long long at = base + k++;
    if (at < o.capacity) {
      o.col[at] = offset + (u64)v;
      o.graph[at] = t;
      o.count[at] = a - p;
    }
  }
}

__global__ __launch_bounds__(256) void wl_runs_kernel(const int32_t* __restrict__ colors, const int32_t* __restrict__ num_nodes,
                                                      int T, int M, RunOut o) {
  extern __shared__ uint32_t lds[];
  __shared__ int part[256];
  uint32_t *cs = lds, *ss = lds + M;
  const int slot = blockIdx.x, c = slot / T, t = slot - c * T, tid = threadIdx.x, n = max(0, min(M, num_nodes[t]));
  for (int i = tid; i < n; i += 256) cs[i] = (uint32_t)colors[(long)slot * M + i];
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const uint32_t c = cs[i];
    int pos = 0;
    for (int j = 0; j < n; ++j) pos += (cs[j] < c || (cs[j] == c && j < i)) ? 1 : 0;
    ss[pos] = c;
  }
  __syncthreads();
  emit_runs(ss, n, slot, t, o.offset + (u64)c * o.stride, o, part);
}

// ---- shortest-path features -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_features_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cv,
                                                          const int32_t* __restrict__ num_nodes, const int32_t* __restrict__ labels,
                                                          int M, int copies, int key_words, RunOut o) {
  extern __shared__ uint32_t lds[];                            // all of it dynamic: the opt-in to the full LDS leaves no room
  uint32_t* keys = lds;                                        // for a static array beside it.  [key_words]; the queues of
  int* part = reinterpret_cast<int*>(lds + key_words);         // the search live in the keys first
  uint8_t* dist = reinterpret_cast<uint8_t*>(lds + key_words + 256); // [n, n]
  uint8_t* queue = reinterpret_cast<uint8_t*>(lds);            // [n, n] bytes <= 4 key_words
  const int t = blockIdx.x, tid = threadIdx.x, n = max(0, min(M, num_nodes[t])), nn = n * n;
  const long base = (long)t * M;
  for (int s = tid; s < n; s += 256) {
    uint8_t *d = dist + s * n, *q = queue + s * n;
    for (int j = 0; j < n; ++j) d[j] = 255;
    d[s] = 0;
    q[0] = (uint8_t)s;
    int head = 0, tail = 1;
    while (head < tail) {
      const int u = q[head++];
      const uint8_t du = d[u];
      const int e1 = rowptr[base + u + 1];
      for (int e = rowptr[base + u]; e < e1; ++e) {
        const int v = cv[2 * (long)e];
        if ((unsigned)v < (unsigned)n && d[v] == 255) {      // every node enters the queue once: tail <= n
          d[v] = (uint8_t)(du + 1);
          q[tail++] = (uint8_t)v;
        }
      }
    }
  }
  __syncthreads();
  int np2 = 1;
  while (np2 < nn) np2 <<= 1;                                  // <= key_words: the host sized it for M
  const int T = gridDim.x;
  for (int c = 0; c < copies; ++c) {                           // the distances stay; the keys, their sort and the runs per copy
    const int32_t* lab = labels + ((long)c * T + t) * M;
    for (int i = tid; i < np2; i += 256) {
      uint32_t key = 0xffffffffu;
      if (i < nn) {
        const int k = i / n, j = i - k * n;
        key = ((uint32_t)lab[k] & 0xfffu) << 20 | ((uint32_t)lab[j] & 0xfffu) << 8 | (uint32_t)dist[i];
      }
      keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < np2; i += 256) {
          const int x = i ^ j;
          if (x > i) {
            const uint32_t a = keys[i], b = keys[x];
            if ((a > b) == ((i & k) == 0)) {
              keys[i] = b;
              keys[x] = a;
            }
          }
        }
        __syncthreads();
      }
    emit_runs(keys, nn, c * T + t, t, (u64)c << 32, o, part);
    __syncthreads();                                           // the next copy rewrites keys and part
  }
}

// ---- Gram -------------------------------------------------------------------------------------------------------------------
struct GramArgs {
  const u64* col_s;
  const uint32_t* idx_s;
  const int32_t* run_graph;
  const int32_t* run_count;
  int* dflag;                        // 1 at the first run of a column that occurs in more than one graph
  const int* incl;                   // inclusive scan of dflag
  int* dcol;                         // dense column of run p, -1 for a one-graph column
  u64* diag;
  u64* stats;                        // columns, one-graph columns, dense columns
  long n;
  int G;
};

__global__ __launch_bounds__(256) void gram_flag_kernel(GramArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  bool head = false, single = false;
  if (p < a.n) {
    const u64 c = a.col_s[p];
    head = p == 0 || a.col_s[p - 1] != c;
    single = head && (p == a.n - 1 || a.col_s[p + 1] != c);
    a.dflag[p] = (head && !single) ? 1 : 0;
    if (single) {
      const uint32_t r = a.idx_s[p];
      const u64 v = (u64)(uint32_t)a.run_count[r];
      const int g = a.run_graph[r];
      if ((unsigned)g < (unsigned)a.G) atomicAdd(&a.diag[g], v * v);
    }
  }
  const u64 mh = __ballot(head), ms = __ballot(single);
  if ((threadIdx.x & 63) == 0) {
    if (mh) atomicAdd(&a.stats[0], (u64)__popcll(mh));
    if (ms) atomicAdd(&a.stats[1], (u64)__popcll(ms));
  }
}

__global__ __launch_bounds__(256) void gram_dcol_kernel(GramArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const u64 c = a.col_s[p];
  const bool single = (p == 0 || a.col_s[p - 1] != c) && (p == a.n - 1 || a.col_s[p + 1] != c);
  a.dcol[p] = single ? -1 : a.incl[p] - 1;
  if (p == a.n - 1) a.stats[2] = (u64)a.incl[p];
}

// the runs of dense columns [c0, c0 + cc) -> counts [G_pad, cc]
__global__ __launch_bounds__(256) void gram_scatter_kernel(const int* __restrict__ dcol, const uint32_t* __restrict__ idx_s,
                                                           const int32_t* __restrict__ run_graph,
                                                           const int32_t* __restrict__ run_count, long n, long c0, int cc, int G,
                                                           int32_t* __restrict__ counts) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const long d = (long)dcol[p] - c0;
  if (d < 0 || d >= cc) return;
  const uint32_t r = idx_s[p];
  const int g = run_graph[r];
  if ((unsigned)g < (unsigned)G) counts[(long)g * cc + d] = run_count[r];
}

// K tile (ti, tj) += counts[ti rows] . counts[tj rows]^T over the chunk (gram_tile.h; chunk_cols is a multiple of kKc).  The
// panels stay int32: a count becomes a double where the fragment is read.
__global__ __launch_bounds__(256) void gram_tile_kernel(const int32_t* __restrict__ counts, int cc, int G, double* __restrict__ K) {
  __shared__ int32_t as[kTile * kLd], bs[kTile * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, hi = lane >> 4, wr = wv >> 1, wc = wv & 1;
  int ti, tj;
  tile_of((long)blockIdx.x, ti, tj);
  f64x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * kTile + wr * 32 + x * 16 + hi + 4 * r, j = tj * kTile + wc * 32 + y * 16 + li;
        acc[x][y][r] = (i < G && j < G) ? K[(long)i * G + j] : 0.0;
      }
  gram_tile_64(                                                // G_pad rows: no row is past the matrix
      as, bs, cc, [&](int r, int k0, int kk) { return counts[((long)ti * kTile + r) * cc + k0 + kk]; },
      [&](int r, int k0, int kk) { return counts[((long)tj * kTile + r) * cc + k0 + kk]; }, acc);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * kTile + wr * 32 + x * 16 + hi + 4 * r, j = tj * kTile + wc * 32 + y * 16 + li;
        if (i < G && j < G) {
          K[(long)i * G + j] = acc[x][y][r];
          if (ti != tj) K[(long)j * G + i] = acc[x][y][r];     // a diagonal tile computes both of its halves itself
        }
      }
}

__global__ __launch_bounds__(256) void gram_diag_kernel(const u64* __restrict__ diag, int G, double* __restrict__ K) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < G) K[(long)g * G + g] += (double)diag[g];
}

__global__ __launch_bounds__(256) void gram_normalize_kernel(const double* __restrict__ K, int G, double* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)G * G) return;
  const int i = (int)(p / G), j = (int)(p - (long)i * G);
  const double a = K[(long)i * G + i], b = K[(long)j * G + j];
  out[p] = (a == 0.0 || b == 0.0) ? 0.0 : K[p] / sqrt(a * b);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
size_t scan64_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (long long*)nullptr, (long long*)nullptr, n, rocprim::plus<long long>(), (hipStream_t)0);
  return b;
}
struct RunsLayout {
  long long* counts;
  void* temp;
  size_t temp_bytes, total;
};
RunsLayout runs_layout(unsigned char* base, size_t graphs) {
  RunsLayout o{};
  Taker t{base};
  o.counts = t.take<long long>(graphs);
  o.temp_bytes = graphs ? scan64_temp_bytes(graphs) : 0;
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

struct GramLayout {
  uint32_t *idx0, *idx_s;
  u64* col_s;
  int *dflag, *incl, *dcol;
  u64* diag;
  int32_t* counts;
  void* temp;
  size_t temp_bytes, total;
  int g_pad;
};
GramLayout gram_layout(unsigned char* base, size_t n, int graphs, int chunk_cols) {
  GramLayout o{};
  Taker t{base};
  o.g_pad = (graphs + kTile - 1) / kTile * kTile;
  o.idx0 = t.take<uint32_t>(n);
  o.idx_s = t.take<uint32_t>(n);
  o.col_s = t.take<u64>(n);
  o.dflag = t.take<int>(n);
  o.incl = t.take<int>(n);
  o.dcol = t.take<int>(n);
  o.diag = t.take<u64>((size_t)graphs);
  o.counts = t.take<int32_t>((size_t)o.g_pad * (size_t)chunk_cols);
  const size_t a = n ? sort_temp_bytes(n) : 0, b = n ? scan_temp_bytes(n) : 0;
  o.temp_bytes = a > b ? a : b;
  o.temp = t.take<unsigned char>(o.temp_bytes);
  o.total = t.off + 256;
  return o;
}

int check_graph_batch(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels) {
  if (int rc = validate_csr(a, who)) return rc;
  if (!num_nodes || !labels) return fail("%s: NULL operand", who);
  if (a->rows != a->cols) return fail("%s: an adjacency is square, got %d x %d", who, a->rows, a->cols);
  return 0;
}

int check_gram(const char* who, int64_t runs, int32_t graphs, int32_t chunk_cols) {
  if (runs < 0 || runs >= (int64_t)INT32_MAX) return fail("%s: %lld runs outside 0..2^31-2", who, (long long)runs);
  if (graphs < 1 || graphs > 46340) return fail("%s: %d graphs outside 1..46,340 (G^2 stays in int32 tiles)", who, graphs);
  if (chunk_cols < kKc || chunk_cols % kKc || chunk_cols > (1 << 20))
    return fail("%s: chunk_cols %d must be a multiple of %d in %d..%d", who, chunk_cols, kKc, kKc, 1 << 20);
  return 0;
}

// count mode: counts -> run_ptr (0, inclusive scan)
int scan_counts(const char* who, const RunsLayout& o, int32_t graphs, int64_t* run_ptr, hipStream_t s) {
  if (int rc = zero_async(who, run_ptr, sizeof(int64_t), s)) return rc;
  size_t temp = o.temp_bytes;
  if (rocprim::inclusive_scan(o.temp, temp, o.counts, reinterpret_cast<long long*>(run_ptr) + 1, (size_t)graphs,
                              rocprim::plus<long long>(), s) != hipSuccess)
    return fail("%s: rocprim::inclusive_scan failed", who);
  return check_launch(who);
}

int check_runs_args(const char* who, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count, int64_t capacity,
                    void* workspace, int64_t workspace_bytes, int32_t graphs) {
  if (!run_ptr) return fail("%s: run_ptr is NULL", who);
  if (run_col && (!run_graph || !run_count)) return fail("%s: run_col without run_graph / run_count", who);
  if (run_col && capacity < 0) return fail("%s: negative capacity", who);
  return run_col ? 0 : check_workspace(who, workspace, workspace_bytes, (int64_t)runs_layout(nullptr, (size_t)graphs).total);
}

}  // namespace

// ---- the launchers graphkern.h declares -----------------------------------------------------------------------------------------
int check_copies(const char* who, const kgcn_csr_batch* a, int32_t copies) {
  if (copies < 1) return fail("%s: %d copies", who, copies);
  if ((int64_t)copies * a->num_graphs * a->rows >= (int64_t)INT32_MAX)
    return fail("%s: %d copies x %d graphs x %d rows: positions and colours are int32, up to 2^31-2 rows in all", who, copies,
                a->num_graphs, a->rows);
  if ((int64_t)copies * a->num_graphs >= (int64_t)INT32_MAX) return fail("%s: %d copies x %d graphs of run slots", who, copies, a->num_graphs);
  return 0;
}

int wl_refine_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int copies,
                  uint64_t hash_mask, int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream) {
  if (int rc = check_graph_batch(who, a, num_nodes, colors)) return rc;
  if (int rc = check_copies(who, a, copies)) return rc;
  if (!key_hi || !key_lo || (a->nnz > 0 && !sorted_nbr)) return fail("%s: NULL output", who);
  const long rows = (long)copies * a->num_graphs * a->rows;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(wl_refine_kernel, dim3(blocks_of(rows * kGroup)), dim3(256), 0, as_stream(stream), a->rowptr, a->cv, num_nodes,
                     colors, a->num_graphs, a->rows, copies, (long)a->nnz, (u64)hash_mask, sorted_nbr, reinterpret_cast<u64*>(key_hi),
                     reinterpret_cast<u64*>(key_lo));
  return check_launch(who);
}

int wl_rank_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, int copies,
                const int32_t* sorted_nbr, const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors, int64_t* info,
                void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_graph_batch(who, a, num_nodes, colors)) return rc;
  if (int rc = check_copies(who, a, copies)) return rc;
  if (!key_hi || !key_lo || !new_colors || !info || (a->nnz > 0 && !sorted_nbr)) return fail("%s: NULL operand", who);
  const long stored = (long)a->num_graphs * a->rows, n = copies * stored;
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)rank_layout(nullptr, (size_t)n).total)) return rc;
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, info, 2 * sizeof(int64_t), s)) return rc;
  if (n == 0) return 0;
  const RankLayout o = rank_layout(aligned_base(workspace), (size_t)n);
  const u64 *hi = reinterpret_cast<const u64*>(key_hi), *lo = reinterpret_cast<const u64*>(key_lo);
  if (int rc = rank_order(who, o, hi, lo, n, s)) return rc;
  const RankArgs r{a->rowptr, num_nodes, colors, sorted_nbr, hi, lo, o.idx2, reinterpret_cast<u64*>(info), (long)a->nnz, (uint32_t)stored,
                   a->rows};
  return rank_sorted(who, r, o, new_colors, r.info, n, s);
}

int wl_runs_run(const char* who, const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, int copies,
                uint64_t column_offset, uint64_t column_stride, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph,
                int32_t* run_count, int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream) {
  if (graphs < 0 || rows < 0 || copies < 1 || (int64_t)copies * graphs * rows >= (int64_t)INT32_MAX ||
      (int64_t)copies * graphs >= (int64_t)INT32_MAX)
    return fail("%s: %d copies x %d graphs x %d rows", who, copies, graphs, rows);
  if (rows > kWlRunsMaxNodes) return fail("%s: %d rows a graph, up to %d (its colours are sorted in LDS)", who, rows, kWlRunsMaxNodes);
  if (!colors || !num_nodes) return fail("%s: NULL operand", who);
  const int slots = copies * graphs;
  if (int rc = check_runs_args(who, run_ptr, run_col, run_graph, run_count, capacity, workspace, workspace_bytes, slots)) return rc;
  hipStream_t s = as_stream(stream);
  if (slots == 0) return zero_async(who, run_ptr, sizeof(int64_t), s);
  RunsLayout o = runs_layout(run_col ? nullptr : aligned_base(workspace), (size_t)slots);
  RunOut ro{o.counts, reinterpret_cast<const long long*>(run_ptr), reinterpret_cast<u64*>(run_col), run_graph, run_count,
            (long long)capacity, (u64)column_offset, (u64)column_stride};
  hipLaunchKernelGGL(wl_runs_kernel, dim3((unsigned)slots), dim3(256), (size_t)(2 * rows + 2) * sizeof(uint32_t), s, colors, num_nodes,
                     graphs, rows, ro);
  if (int rc = check_launch(who)) return rc;
  return run_col ? 0 : scan_counts(who, o, slots, run_ptr, s);
}

int sp_features_run(const char* who, const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int copies,
                    int32_t num_labels, int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count,
                    int64_t capacity, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_graph_batch(who, a, num_nodes, labels)) return rc;
  if (int rc = check_copies(who, a, copies)) return rc;
  if (a->rows > kSpMaxNodes)
    return fail("%s: %d nodes a graph, up to %d: a distance and a queue entry are one byte each and the n^2 sorted keys of a graph "
                "(64 KB at 128 nodes) must fit the LDS of its workgroup", who, a->rows, kSpMaxNodes);
  if (num_labels < 0 || num_labels > kSpMaxLabels)
    return fail("%s: %d distinct labels, up to %d: the key packs (label, label, distance) into 12 + 12 + 8 bits", who, num_labels,
                kSpMaxLabels);
  const int graphs = a->num_graphs, M = a->rows, slots = copies * graphs;
  if (int rc = check_runs_args(who, run_ptr, run_col, run_graph, run_count, capacity, workspace, workspace_bytes, slots)) return rc;
  hipStream_t s = as_stream(stream);
  if (graphs == 0) return zero_async(who, run_ptr, sizeof(int64_t), s);
  int key_words = 1;
  while (key_words < M * M) key_words <<= 1;
  const size_t lds = (size_t)key_words * 4 + 256 * sizeof(int) + (((size_t)M * M + 3) & ~(size_t)3);
  if (int rc = allow_full_lds<sp_features_kernel>(lds, who)) return rc;
  RunsLayout o = runs_layout(run_col ? nullptr : aligned_base(workspace), (size_t)slots);
  RunOut ro{o.counts, reinterpret_cast<const long long*>(run_ptr), reinterpret_cast<u64*>(run_col), run_graph, run_count,
            (long long)capacity, 0ull, 0ull};
  hipLaunchKernelGGL(sp_features_kernel, dim3((unsigned)graphs), dim3(256), lds, s, a->rowptr, a->cv, num_nodes, labels, M, copies,
                     key_words, ro);
  if (int rc = check_launch(who)) return rc;
  return run_col ? 0 : scan_counts(who, o, slots, run_ptr, s);
}

}  // namespace kgcn

using namespace kgcn;

extern "C" int kgcn_wl_refine_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, uint64_t hash_mask,
                                  int32_t* sorted_nbr, uint64_t* key_hi, uint64_t* key_lo, void* stream) {
  return wl_refine_run("kgcn_wl_refine_i32", a, num_nodes, colors, 1, hash_mask, sorted_nbr, key_hi, key_lo, stream);
}

extern "C" int64_t kgcn_wl_rank_workspace_bytes(int64_t rows) {
  if (rows < 0 || rows >= (int64_t)INT32_MAX) return refuse_query("kgcn_wl_rank_workspace_bytes: %lld rows outside 0..2^31-2", (long long)rows);
  return (int64_t)rank_layout(nullptr, (size_t)rows).total;
}

extern "C" int kgcn_wl_rank_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* colors, const int32_t* sorted_nbr,
                                const uint64_t* key_hi, const uint64_t* key_lo, int32_t* new_colors, int64_t* info, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return wl_rank_run("kgcn_wl_rank_i32", a, num_nodes, colors, 1, sorted_nbr, key_hi, key_lo, new_colors, info, workspace,
                     workspace_bytes, stream);
}

extern "C" int64_t kgcn_graph_runs_workspace_bytes(int32_t graphs) {
  if (graphs < 0) return refuse_query("kgcn_graph_runs_workspace_bytes: %d graphs", graphs);
  return (int64_t)runs_layout(nullptr, (size_t)graphs).total;
}

extern "C" int kgcn_wl_runs_i32(const int32_t* colors, const int32_t* num_nodes, int32_t graphs, int32_t rows, uint64_t column_offset,
                                int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count, int64_t capacity,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  return wl_runs_run("kgcn_wl_runs_i32", colors, num_nodes, graphs, rows, 1, column_offset, 0, run_ptr, run_col, run_graph, run_count,
                     capacity, workspace, workspace_bytes, stream);
}

extern "C" int kgcn_sp_features_i32(const kgcn_csr_batch* a, const int32_t* num_nodes, const int32_t* labels, int32_t num_labels,
                                    int64_t* run_ptr, uint64_t* run_col, int32_t* run_graph, int32_t* run_count, int64_t capacity,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  return sp_features_run("kgcn_sp_features_i32", a, num_nodes, labels, 1, num_labels, run_ptr, run_col, run_graph, run_count, capacity,
                         workspace, workspace_bytes, stream);
}

extern "C" int64_t kgcn_graph_gram_workspace_bytes(int64_t runs, int32_t graphs, int32_t chunk_cols) {
  if (check_gram("kgcn_graph_gram_workspace_bytes", runs, graphs, chunk_cols)) return -1;
  return (int64_t)gram_layout(nullptr, (size_t)runs, graphs, chunk_cols).total;
}

extern "C" int kgcn_gram_plan_i64(const uint64_t* run_col, const int32_t* run_graph, const int32_t* run_count, int64_t runs,
                                  int32_t graphs, int32_t chunk_cols, int64_t* stats, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  const char* who = "kgcn_gram_plan_i64";
  if (int rc = check_gram(who, runs, graphs, chunk_cols)) return rc;
  if (!stats || (runs > 0 && (!run_col || !run_graph || !run_count))) return fail("%s: NULL operand", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)gram_layout(nullptr, (size_t)runs, graphs, chunk_cols).total)) return rc;
  hipStream_t s = as_stream(stream);
  GramLayout o = gram_layout(aligned_base(workspace), (size_t)runs, graphs, chunk_cols);
  if (int rc = zero_async(who, stats, 3 * sizeof(int64_t), s)) return rc;
  if (int rc = zero_async(who, o.diag, (size_t)graphs * sizeof(u64), s)) return rc;
  if (runs == 0) return 0;
  const long n = (long)runs;
  const unsigned nb = blocks_of(n);
  hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, s, o.idx0, n);
  size_t temp = o.temp_bytes;
  if (rocprim::radix_sort_pairs(o.temp, temp, reinterpret_cast<const u64*>(run_col), o.col_s, o.idx0, o.idx_s, (size_t)n, 0u, 64u, s) !=
      hipSuccess)
    return fail("%s: rocprim::radix_sort_pairs failed", who);
  GramArgs g{o.col_s, o.idx_s, run_graph, run_count, o.dflag, o.incl, o.dcol, o.diag, reinterpret_cast<u64*>(stats), n, graphs};
  hipLaunchKernelGGL(gram_flag_kernel, dim3(nb), dim3(256), 0, s, g);
  temp = o.temp_bytes;
  if (rocprim::inclusive_scan(o.temp, temp, o.dflag, o.incl, (size_t)n, rocprim::plus<int>(), s) != hipSuccess)
    return fail("%s: rocprim::inclusive_scan failed", who);
  hipLaunchKernelGGL(gram_dcol_kernel, dim3(nb), dim3(256), 0, s, g);
  return check_launch(who);
}

extern "C" int kgcn_gram_dense_f64(const int32_t* run_graph, const int32_t* run_count, int64_t runs, int32_t graphs, int64_t dense_cols,
                                   int32_t chunk_cols, double* gram, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "kgcn_gram_dense_f64";
  if (int rc = check_gram(who, runs, graphs, chunk_cols)) return rc;
  if (!gram || (runs > 0 && (!run_graph || !run_count))) return fail("%s: NULL operand", who);
  if (dense_cols < 0 || dense_cols > runs / 2) return fail("%s: %lld dense columns for %lld runs", who, (long long)dense_cols, (long long)runs);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)gram_layout(nullptr, (size_t)runs, graphs, chunk_cols).total)) return rc;
  hipStream_t s = as_stream(stream);
  GramLayout o = gram_layout(aligned_base(workspace), (size_t)runs, graphs, chunk_cols);
  if (int rc = zero_async(who, gram, (size_t)graphs * graphs * sizeof(double), s)) return rc;
  const unsigned nt = (unsigned)(o.g_pad / kTile);
  for (int64_t c0 = 0; c0 < dense_cols; c0 += chunk_cols) {
    if (int rc = zero_async(who, o.counts, (size_t)o.g_pad * chunk_cols * sizeof(int32_t), s)) return rc;
    hipLaunchKernelGGL(gram_scatter_kernel, dim3(blocks_of((long)runs)), dim3(256), 0, s, o.dcol, o.idx_s, run_graph, run_count,
                       (long)runs, (long)c0, chunk_cols, graphs, o.counts);
    hipLaunchKernelGGL(gram_tile_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, o.counts, chunk_cols, graphs, gram);
  }
  hipLaunchKernelGGL(gram_diag_kernel, dim3(blocks_of(graphs)), dim3(256), 0, s, o.diag, graphs, gram);
  return check_launch(who);
}

extern "C" int kgcn_gram_normalize_f64(const double* gram, int32_t graphs, double* out, void* stream) {
  const char* who = "kgcn_gram_normalize_f64";
  if (graphs < 1 || graphs > 46340) return fail("%s: %d graphs outside 1..46,340", who, graphs);
  if (!gram || !out) return fail("%s: NULL operand", who);
  hipLaunchKernelGGL(gram_normalize_kernel, dim3(blocks_of((long)graphs * graphs)), dim3(256), 0, as_stream(stream), gram, graphs, out);
  return check_launch(who);
}
