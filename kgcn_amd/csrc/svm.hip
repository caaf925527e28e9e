// Batched C-SVC over a precomputed kernel: the nested KFold / SVC(kernel="precomputed") loop of the reference's graph_kernel/gk.py:243-292
// as one batch of independent dual problems over ONE shared Gram matrix (the driver is kgcn_amd/graph_kernel.py svm_fit / svm_cv).
// The solver is libsvm's (svm.cpp Solver::Solve, select_working_set, calculate_rho; TAU = 1e-12) in fp64, without shrinking and
// without a kernel cache; include/kgcn_hip.h states the contract, tests/kernel_svm_oracle.py restates every step in numpy.
//
//   smo       one workgroup a problem.  G, alpha, QD (fp64), the row indices and the signs of the problem live in LDS; element t
//             belongs to thread t % kThreads, which also keeps K[i, idx_t] of the selected row i in registers from the selection of j
//             to the gradient update.  A problem of up to 256 rows runs on one wave, up to 1,024 on four, beyond on sixteen: at most
//             four elements a thread.  The reductions carry (value, index) and order equal values by index, so the iterates do not
//             depend on that choice.  Every thread computes the two-variable update itself from the same four LDS values: the same
//             operations on the same bits, so all threads agree and no broadcast is needed.  Three barriers an iteration.
//   decision  one thread an (job, evaluation row): a sequential sum over the training rows in their stored order.
//   vote      one thread an (vote, evaluation row): libsvm's one-vs-one count without a vote array.
// Nothing is fused: the Makefile builds this file with -ffp-contract=off (see hashkern.hip for why a pragma is not enough).  Every
// descriptor a kernel reads is range-checked in the kernel before it is used as an address: a bad one is reported, never followed.
#include <math.h>

#include "workspace.h"

namespace kgcn {
namespace {

typedef unsigned long long u64;
constexpr int kMaxRows = KGCN_SVM_MAX_ROWS;
constexpr int kPerThread = 4;                    // elements a thread owns: 64 / 256 / 1,024 threads for 256 / 1,024 / 4,096 rows
constexpr int kSlotDoubles = 4 * 16;             // one reduction slot: (value, carried, maximum, index) of up to 16 waves
constexpr double kTau = 1e-12;                   // svm.cpp: #define TAU 1e-12

struct Sets {
  const long long* ptr;
  const int32_t* idx;
  const int8_t* sign;
  long long total;
  int count, max_rows;
};

// set s -> its first entry and length, false when anything about it is out of range
__device__ __forceinline__ bool set_range(const Sets& s, int set, long long& first, int& n) {
  first = 0;
  n = 0;
  if (set < 0 || set >= s.count) return false;
  const long long b0 = s.ptr[set], b1 = s.ptr[set + 1];
  if (b0 < 0 || b1 < b0 || b1 > s.total || b1 - b0 > (long long)s.max_rows) return false;
  first = b0;
  n = (int)(b1 - b0);
  return true;
}

struct SmoArgs {
  const double* K;
  int graphs;
  Sets train;
  const int32_t* prob_set;
  const double* prob_C;
  double tol;
  long long max_iter;
  int iters_per_launch, first;
  double *alpha, *rho, *Gws;
  long long* n_iter;
  int32_t* status;
  unsigned* unfinished;
};

// (v, i) <- the best of the workgroup under max (kMin: min), the LAST index among equal values; c travels with the winner;
// m <- the plain maximum.  Every thread returns the same values.  slot: kSlotDoubles of LDS nobody else touches until the next
// barrier but one.
template <int kThreads, bool kMin>
__device__ __forceinline__ void block_pick(double& v, int& i, double& c, double& m, double* slot) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64), oc = __shfl_xor(c, off, 64), om = __shfl_xor(m, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    const bool take = kMin ? (ov < v || (ov == v && oi > i)) : (ov > v || (ov == v && oi > i));
    if (take) { v = ov; i = oi; c = oc; }
    if (om > m) m = om;
  }
  constexpr int kWaves = kThreads / 64;
  if (kWaves > 1) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      slot[4 * w] = v;
      slot[4 * w + 1] = c;
      slot[4 * w + 2] = m;
      slot[4 * w + 3] = (double)i;
    }
    __syncthreads();
    v = slot[0]; c = slot[1]; m = slot[2]; i = (int)slot[3];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      const double ov = slot[4 * k], om = slot[4 * k + 2];
      const int oi = (int)slot[4 * k + 3];
      const bool take = kMin ? (ov < v || (ov == v && oi > i)) : (ov > v || (ov == v && oi > i));
      if (take) { v = ov; i = oi; c = slot[4 * k + 1]; }
      if (om > m) m = om;
    }
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void svm_smo_kernel(SmoArgs a) {
  extern __shared__ double lds[];
  const int p = blockIdx.x, tid = threadIdx.x, stride = a.train.max_rows;
  if (!a.first && a.status[p] != KGCN_SVM_RUNNING) return;             // finished in an earlier slice (uniform: one word a workgroup)
  double* sG = lds;
  double* sA = lds + stride;
  double* sQD = lds + 2 * stride;
  double* slots = lds + 3 * stride;
  int32_t* sIdx = reinterpret_cast<int32_t*>(slots + 2 * kSlotDoubles);
  int8_t* sY = reinterpret_cast<int8_t*>(sIdx + stride);

  // ---- the descriptor, checked before anything is addressed through it
  long long b0;
  int n;
  const double C = a.prob_C[p];
  bool bad = !set_range(a.train, a.prob_set[p], b0, n) || n < 1 || !(C > 0.0) || !(C < INFINITY);
  int idx[kPerThread];
  double y[kPerThread];
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const int t = tid + e * kThreads;
    idx[e] = 0;
    y[e] = 1.0;
    if (t < n) {
      idx[e] = a.train.idx[b0 + t];
      const int sg = a.train.sign[b0 + t];
      y[e] = (double)sg;
      if (idx[e] < 0 || idx[e] >= a.graphs || (sg != 1 && sg != -1)) bad = true;
    }
  }
  int* any_bad = reinterpret_cast<int*>(slots);                       // (no __syncthreads_or: it takes static LDS, and with it the
  if (tid == 0) *any_bad = 0;                                          //  kernel could not be given the CU's whole LDS as dynamic)
  __syncthreads();
  if (bad) *any_bad = 1;
  __syncthreads();
  if (*any_bad) {
    if (tid == 0) a.status[p] = KGCN_SVM_REFUSED;
    return;
  }
  const long ldk = a.graphs;
  const long base = (long)p * stride;
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const int t = tid + e * kThreads;
    if (t < n) {
      sIdx[t] = idx[e];
      sY[t] = (int8_t)y[e];
      sQD[t] = a.K[(long)idx[e] * ldk + idx[e]];                       // svm.cpp SVC_Q: QD[i] = kernel(i, i)
      sA[t] = a.first ? 0.0 : a.alpha[base + t];                       // solve_c_svc: alpha = 0, p = -1, so G = -1
      sG[t] = a.first ? -1.0 : a.Gws[base + t];
    }
  }
  long long iter = a.first ? 0 : a.n_iter[p];
  const long long by_rows = 100ll * n;
  const long long max_iter = a.max_iter > 0 ? a.max_iter : (by_rows > 10000000ll ? by_rows : 10000000ll);
  __syncthreads();

  int st = KGCN_SVM_RUNNING;
  for (int k = 0;; ++k) {
    if (iter >= max_iter) { st = KGCN_SVM_MAX_ITER; break; }
    if (k >= a.iters_per_launch) break;
    // ---- select_working_set, first half: i = argmax of -y_t G_t over I_up
    double bv = -INFINITY, dummy_c = 0.0, dummy_m = -INFINITY;
    int bi = -1;
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
      const int t = tid + e * kThreads;
      if (t < n) {
        const double al = sA[t], v = -(y[e] * sG[t]);
        const bool up = y[e] > 0.0 ? al < C : al > 0.0;                  // !is_upper_bound / !is_lower_bound
        if (up && v >= bv) { bv = v; bi = t; }
      }
    }
    block_pick<kThreads, false>(bv, bi, dummy_c, dummy_m, slots);
    if (bi < 0) { st = KGCN_SVM_CONVERGED; break; }                    // Gmax = -INF: no j qualifies, libsvm returns 1
    const int i = bi;
    const double Gmax = bv, QDi = sQD[i];
    const double* Ki = a.K + (long)sIdx[i] * ldk;
    double ki[kPerThread];
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) ki[e] = tid + e * kThreads < n ? Ki[idx[e]] : 0.0;
    // ---- second half: j = argmin of -grad_diff^2 / quad_coef over I_low with grad_diff > 0; Gmax2 = max of y_t G_t over I_low
    double ov = INFINITY, okij = 0.0, g2 = -INFINITY;
    int oj = -1;
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
      const int t = tid + e * kThreads;
      if (t < n) {
        const double al = sA[t], yg = y[e] * sG[t];
        const bool low = y[e] > 0.0 ? al > 0.0 : al < C;               // !is_lower_bound / !is_upper_bound
        if (low) {
          if (yg >= g2) g2 = yg;
          const double gd = Gmax + yg;
          if (gd > 0.0) {
            double q = (QDi + sQD[t]) - 2.0 * ki[e];
            if (!(q > 0.0)) q = kTau;
            const double ob = -(gd * gd) / q;
            if (ob <= ov) { ov = ob; oj = t; okij = ki[e]; }
          }
        }
      }
    }
    block_pick<kThreads, true>(ov, oj, okij, g2, slots + kSlotDoubles);
    if (Gmax + g2 < a.tol || oj < 0) { st = KGCN_SVM_CONVERGED; break; }
    const int j = oj;
    ++iter;
    const double* Kj = a.K + (long)sIdx[j] * ldk;
    double kj[kPerThread];
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) kj[e] = tid + e * kThreads < n ? Kj[idx[e]] : 0.0;
    // ---- Solver::Solve: update alpha[i] and alpha[j], handle bounds carefully (every thread, from the same values)
    const double yi = (double)sY[i], yj = (double)sY[j], Gi = sG[i], Gj = sG[j], old_i = sA[i], old_j = sA[j];
    double quad = (QDi + sQD[j]) - 2.0 * okij;
    if (quad <= 0.0) quad = kTau;
    double ai = old_i, aj = old_j;
    if (yi != yj) {
      const double delta = (-Gi - Gj) / quad, diff = ai - aj;
      ai = ai + delta;
      aj = aj + delta;
      if (diff > 0.0) {
        if (aj < 0.0) { aj = 0.0; ai = diff; }
      } else {
        if (ai < 0.0) { ai = 0.0; aj = -diff; }
      }
      if (diff > 0.0) {                                               // C_i - C_j = 0: one C for both classes
        if (ai > C) { ai = C; aj = C - diff; }
      } else {
        if (aj > C) { aj = C; ai = C + diff; }
      }
    } else {
      const double delta = (Gi - Gj) / quad, sum = ai + aj;
      ai = ai - delta;
      aj = aj + delta;
      if (sum > C) {
        if (ai > C) { ai = C; aj = sum - C; }
      } else {
        if (aj < 0.0) { aj = 0.0; ai = sum; }
      }
      if (sum > C) {
        if (aj > C) { aj = C; ai = sum - C; }
      } else {
        if (ai < 0.0) { ai = 0.0; aj = sum; }
      }
    }
    const double dai = ai - old_i, daj = aj - old_j;
    __syncthreads();                                                   // everyone has read element i and j
    // ---- G[t] += Q_i[t] * delta_alpha_i + Q_j[t] * delta_alpha_j, Q_it = y_i y_t K_it (exact)
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
      const int t = tid + e * kThreads;
      if (t < n) {
        const double pi = ((yi * y[e]) * ki[e]) * dai, pj = ((yj * y[e]) * kj[e]) * daj;
        sG[t] = sG[t] + (pi + pj);
        if (t == i) sA[t] = ai;
        if (t == j) sA[t] = aj;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const int t = tid + e * kThreads;
    if (t < n) {
      a.alpha[base + t] = sA[t];
      a.Gws[base + t] = sG[t];
    }
  }
  if (tid != 0) return;
  a.n_iter[p] = iter;
  a.status[p] = st;
  if (st == KGCN_SVM_RUNNING) {
    atomicAdd(a.unfinished, 1u);
    return;
  }
  // ---- Solver::calculate_rho, one thread, t ascending
  double ub = INFINITY, lb = -INFINITY, sum_free = 0.0;
  int nr_free = 0;
  for (int t = 0; t < n; ++t) {
    const double yt = (double)sY[t], yG = yt * sG[t], al = sA[t];
    if (al >= C) {
      if (yt < 0.0) ub = ub < yG ? ub : yG;
      else lb = lb > yG ? lb : yG;
    } else if (al <= 0.0) {
      if (yt > 0.0) ub = ub < yG ? ub : yG;
      else lb = lb > yG ? lb : yG;
    } else {
      ++nr_free;
      sum_free = sum_free + yG;
    }
  }
  a.rho[p] = nr_free > 0 ? sum_free / (double)nr_free : (ub + lb) / 2.0;
}

struct DecArgs {
  const double* K;
  int graphs;
  Sets train;
  const int32_t* prob_set;
  int problems;
  const double *alpha, *rho;
  Sets eval;
  const int32_t *job_prob, *job_eval;
  const long long* job_out;
  int jobs;
  double* dec;
  long long dec_total;
  u64* errors;
};

__global__ __launch_bounds__(256) void svm_decision_kernel(DecArgs a) {
  const int q = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  const int p = a.job_prob[q];
  long long b0, e0;
  int n, m;
  const long long o0 = a.job_out[q], o1 = a.job_out[q + 1];
  bool ok = p >= 0 && p < a.problems && set_range(a.eval, a.job_eval[q], e0, m) && o0 >= 0 && o1 - o0 == (long long)m && o1 <= a.dec_total;
  ok = ok && set_range(a.train, a.prob_set[p], b0, n);
  if (!ok) {
    if (r == 0) atomicAdd(a.errors, 1ull);
    return;
  }
  if (r >= m) return;
  const int row = a.eval.idx[e0 + r];
  if (row < 0 || row >= a.graphs) {
    atomicAdd(a.errors, 1ull);
    return;
  }
  const double* Kr = a.K + (long)row * a.graphs;
  const double* al = a.alpha + (long)p * a.train.max_rows;
  double acc = 0.0;
  bool bad = false;
  for (int t = 0; t < n; ++t) {
    const int c = a.train.idx[b0 + t];
    if (c < 0 || c >= a.graphs) {
      bad = true;
      break;
    }
    acc = acc + (al[t] * (double)a.train.sign[b0 + t]) * Kr[c];
  }
  if (bad) {
    atomicAdd(a.errors, 1ull);
    return;
  }
  a.dec[o0 + r] = acc - a.rho[p];
}

struct VoteArgs {
  const double* dec;
  long long dec_total;
  const long long* job_out;
  int jobs;
  Sets eval;
  const int32_t *vote_first_job, *vote_eval;
  const long long* vote_out;
  int votes, classes;
  const int32_t* labels;
  int graphs;
  int32_t* pred;
  long long pred_total;
  u64 *correct, *errors;
};

__global__ __launch_bounds__(256) void svm_vote_kernel(VoteArgs a) {
  const int v = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  const int k = a.classes, npairs = k * (k - 1) / 2, q0 = a.vote_first_job[v];
  long long e0;
  int m;
  const long long o0 = a.vote_out[v], o1 = a.vote_out[v + 1];
  bool ok = q0 >= 0 && q0 + npairs <= a.jobs && set_range(a.eval, a.vote_eval[v], e0, m) && o0 >= 0 && o1 - o0 == (long long)m &&
            o1 <= a.pred_total;
  for (int s = 0; ok && s < npairs; ++s) {
    const long long d0 = a.job_out[q0 + s], d1 = a.job_out[q0 + s + 1];
    ok = d0 >= 0 && d1 - d0 == (long long)m && d1 <= a.dec_total;
  }
  if (!ok) {
    if (r == 0) atomicAdd(a.errors, 1ull);
    return;
  }
  if (r >= m) return;
  const int row = a.eval.idx[e0 + r];
  if (row < 0 || row >= a.graphs) {
    atomicAdd(a.errors, 1ull);
    return;
  }
  // svm_predict_values: vote[c] = pairs (c, b) with dec > 0 + pairs (b, c) with !(dec > 0); the first maximum
  int best = 0, best_votes = -1;
  for (int c = 0; c < k; ++c) {
    int votes = 0;
    for (int b = 0; b < c; ++b) votes += a.dec[a.job_out[q0 + b * (2 * k - b - 1) / 2 + (c - b - 1)] + r] > 0.0 ? 0 : 1;
    for (int b = c + 1; b < k; ++b) votes += a.dec[a.job_out[q0 + c * (2 * k - c - 1) / 2 + (b - c - 1)] + r] > 0.0 ? 1 : 0;
    if (votes > best_votes) {
      best_votes = votes;
      best = c;
    }
  }
  a.pred[o0 + r] = best;
  if (a.labels[row] == best) atomicAdd(&a.correct[v], 1ull);
}

int check_sets(const char* who, const char* what, const Sets& s, bool need_sign) {
  if (s.count < 0 || s.total < 0 || s.max_rows < 0 || s.total > (long long)s.count * s.max_rows)
    return fail("%s: %s sets: count %d, total %lld, max_rows %d", who, what, s.count, s.total, s.max_rows);
  if (!s.ptr || (s.total > 0 && (!s.idx || (need_sign && !s.sign)))) return fail("%s: %s sets: NULL array", who, what);
  return 0;
}

int check_rows(const char* who, int32_t max_rows) {
  if (max_rows < 1 || max_rows > kMaxRows)
    return fail("%s: %d training rows in the longest set outside 1..%d (G, alpha and QD of a problem live in LDS)", who, max_rows, kMaxRows);
  return 0;
}

size_t smo_lds_bytes(int stride) {
  return (size_t)stride * (3 * sizeof(double) + sizeof(int32_t) + sizeof(int8_t)) + 2 * kSlotDoubles * sizeof(double);
}

struct Workspace {
  unsigned* unfinished;              // the unfinished-problem word
  double* grad;                      // [problems, max_rows]
  size_t total;
};
Workspace carve(unsigned char* base, int32_t problems, int32_t max_rows) {
  Workspace o{};
  Taker t{base};
  o.unfinished = t.take<unsigned>(1);
  const size_t head = t.off, rows = (size_t)problems * max_rows;
  o.grad = t.take<double>(rows);
  o.total = head + rows * sizeof(double) + 256;                // the last array is counted as it is, not rounded up
  return o;
}

template <int kThreads>
int launch_smo(const char* who, const SmoArgs& a, int problems, hipStream_t s) {
  const size_t lds = smo_lds_bytes(a.train.max_rows);
  if (int rc = allow_full_lds<svm_smo_kernel<kThreads>>(lds, who)) return rc;
  hipLaunchKernelGGL((svm_smo_kernel<kThreads>), dim3(problems), dim3(kThreads), lds, s, a);
  return check_launch(who);
}

}  // namespace
}  // namespace kgcn

using namespace kgcn;

extern "C" int64_t kgcn_svm_workspace_bytes(int32_t problems, int32_t max_rows) {
  if (problems < 0) return refuse_query("kgcn_svm_workspace_bytes: %d problems", problems);
  if (check_rows("kgcn_svm_workspace_bytes", max_rows)) return -1;
  return (int64_t)carve(nullptr, problems, max_rows).total;
}

extern "C" int kgcn_svm_smo_f64(const double* K, int32_t graphs, const int64_t* set_ptr, const int32_t* set_idx, const int8_t* set_sign,
                                int32_t sets, int64_t set_total, int32_t max_rows, const int32_t* prob_set, const double* prob_C,
                                int32_t problems, const double* tol, int64_t max_iter, int32_t iters_per_launch, int32_t first,
                                double* alpha, double* rho, int64_t* n_iter, int32_t* status, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  const char* who = "kgcn_svm_smo_f64";
  const Sets train{reinterpret_cast<const long long*>(set_ptr), set_idx, set_sign, (long long)set_total, sets, max_rows};
  if (int rc = check_rows(who, max_rows)) return rc;
  if (int rc = check_sets(who, "training", train, true)) return rc;
  if (graphs < 1 || graphs > 46340) return fail("%s: %d rows of K outside 1..46,340", who, graphs);
  if (problems < 0) return fail("%s: %d problems", who, problems);
  if (!tol || !(*tol > 0.0) || !(*tol < INFINITY)) return fail("%s: the tolerance must be positive and finite", who);
  if (iters_per_launch < 1) return fail("%s: %d iterations a launch, at least 1", who, iters_per_launch);
  if (int rc = check_workspace(who, workspace, workspace_bytes, (int64_t)carve(nullptr, problems, max_rows).total)) return rc;
  const Workspace ws = carve(aligned_base(workspace), problems, max_rows);
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, ws.unfinished, sizeof(unsigned), s)) return rc;
  if (problems == 0) return 0;
  if (!K || !prob_set || !prob_C || !alpha || !rho || !n_iter || !status) return fail("%s: NULL operand", who);
  SmoArgs a{K, graphs, train, prob_set, prob_C, *tol, (long long)max_iter, iters_per_launch, first ? 1 : 0, alpha, rho,
            ws.grad, reinterpret_cast<long long*>(n_iter), status, ws.unfinished};
  if (max_rows <= 64 * kPerThread) return launch_smo<64>(who, a, problems, s);
  if (max_rows <= 256 * kPerThread) return launch_smo<256>(who, a, problems, s);
  return launch_smo<1024>(who, a, problems, s);
}

extern "C" int kgcn_svm_decision_f64(const double* K, int32_t graphs, const int64_t* set_ptr, const int32_t* set_idx,
                                     const int8_t* set_sign, int32_t sets, int64_t set_total, int32_t max_rows, const int32_t* prob_set,
                                     int32_t problems, const double* alpha, const double* rho, const int64_t* eval_ptr,
                                     const int32_t* eval_idx, int32_t evals, int64_t eval_total, int32_t eval_max_rows,
                                     const int32_t* job_prob, const int32_t* job_eval, const int64_t* job_out, int32_t jobs, double* dec,
                                     int64_t dec_total, int64_t* errors, void* stream) {
  const char* who = "kgcn_svm_decision_f64";
  const Sets train{reinterpret_cast<const long long*>(set_ptr), set_idx, set_sign, (long long)set_total, sets, max_rows};
  const Sets eval{reinterpret_cast<const long long*>(eval_ptr), eval_idx, nullptr, (long long)eval_total, evals, eval_max_rows};
  if (int rc = check_sets(who, "training", train, true)) return rc;
  if (int rc = check_sets(who, "evaluation", eval, false)) return rc;
  if (graphs < 1 || graphs > 46340) return fail("%s: %d rows of K outside 1..46,340", who, graphs);
  if (problems < 0 || jobs < 0 || jobs > 65535 || dec_total < 0) return fail("%s: %d problems, %d jobs (up to 65,535)", who, problems, jobs);
  if (!errors) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, errors, sizeof(int64_t), s)) return rc;
  if (jobs == 0 || eval_max_rows == 0) return 0;
  if (!K || !prob_set || !alpha || !rho || !job_prob || !job_eval || !job_out || !dec) return fail("%s: NULL operand", who);
  DecArgs a{K, graphs, train, prob_set, problems, alpha, rho, eval, job_prob, job_eval,
            reinterpret_cast<const long long*>(job_out), jobs, dec, (long long)dec_total, reinterpret_cast<u64*>(errors)};
  hipLaunchKernelGGL(svm_decision_kernel, dim3(blocks_of(eval_max_rows), jobs), dim3(256), 0, s, a);
  return check_launch(who);
}

extern "C" int kgcn_svm_vote_i32(const double* dec, int64_t dec_total, const int64_t* job_out, int32_t jobs, const int64_t* eval_ptr,
                                 const int32_t* eval_idx, int32_t evals, int64_t eval_total, int32_t eval_max_rows,
                                 const int32_t* vote_first_job, const int32_t* vote_eval, const int64_t* vote_out, int32_t votes,
                                 int32_t classes, const int32_t* labels, int32_t graphs, int32_t* pred, int64_t pred_total,
                                 int64_t* correct, int64_t* errors, void* stream) {
  const char* who = "kgcn_svm_vote_i32";
  const Sets eval{reinterpret_cast<const long long*>(eval_ptr), eval_idx, nullptr, (long long)eval_total, evals, eval_max_rows};
  if (int rc = check_sets(who, "evaluation", eval, false)) return rc;
  if (classes < 2 || classes > KGCN_SVM_MAX_CLASSES) return fail("%s: %d classes outside 2..%d", who, classes, KGCN_SVM_MAX_CLASSES);
  if (graphs < 1 || jobs < 0 || votes < 0 || votes > 65535 || dec_total < 0 || pred_total < 0)
    return fail("%s: %d graphs, %d jobs, %d votes (up to 65,535)", who, graphs, jobs, votes);
  if (!errors) return fail("%s: NULL operand", who);
  hipStream_t s = as_stream(stream);
  if (int rc = zero_async(who, errors, sizeof(int64_t), s)) return rc;
  if (votes == 0) return 0;
  if (!correct || !dec || !job_out || !vote_first_job || !vote_eval || !vote_out || !labels || !pred) return fail("%s: NULL operand", who);
  if (int rc = zero_async(who, correct, (size_t)votes * sizeof(int64_t), s)) return rc;
  if (eval_max_rows == 0) return 0;
  VoteArgs a{dec, (long long)dec_total, reinterpret_cast<const long long*>(job_out), jobs, eval, vote_first_job, vote_eval,
             reinterpret_cast<const long long*>(vote_out), votes, classes, labels, graphs, pred, (long long)pred_total,
             reinterpret_cast<u64*>(correct), reinterpret_cast<u64*>(errors)};
  hipLaunchKernelGGL(svm_vote_kernel, dim3(blocks_of(eval_max_rows), votes), dim3(256), 0, s, a);
  return check_launch(who);
}
