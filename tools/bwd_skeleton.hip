// Memory skeleton of the fused GraphConv backward (development tool, GPU box only): kernels that move exactly the HBM bytes of
// graphconv_bwd_planes_kernel -- per graph two [32 x 64] fp32 tiles in (x, g), a CSR slice in, one [32 x 64] tile out -- with NO
// contraction / aggregation work, so what they reach is the ceiling the memory system gives this byte pattern (2 : 1 read : write,
// 8 KiB tiles).  Round 2 measured the persistent form at 4 and 8 waves per CU (profiles/r02_microbench_bwd_memory_skeleton.txt:
// 0.472-0.484 ms whatever the occupancy); round 6 adds the questions the two-wave-roles kernel raises:
//   P   persistent waves, one graph per wave, prefetch depth 1 / 2, 4 / 8 / 12 waves per CU           (the shipped structure)
//   PX  as P with x loaded in the dW A-fragment layout of the shipped kernel (16 x 8-byte loads, two 256-byte rows each)
//   H   persistent PAIRS: two waves share a graph (wave A: g + CSR in, dX out; wave B: x in), 8 waves per CU   (the two-role form)
//   N   non-persistent, one wave per graph, no prefetch, as many waves per CU as registers allow       (the SpMM's structure)
// usage: bwd_skeleton [graphs [ingest | dxstore | fwdpairs]]
//   ingest:  only the LDS-DMA / nontemporal arms of skel_fi / skel_hi and their references
//   dxstore: only the dX store forms of skel_hi (S0 / S1 / S2, plain and nontemporal, pure and beside the arithmetic) and the
//            write-only / read-only streams that price a stored and a loaded byte on the box at hand
//   fwdpairs: only the forward as reader | aggregator wave pairs (skel_fp) against the shipped structure (skel_fi), both streams
//            nontemporal, pure and beside the arithmetic, three repetitions, with the medians, the spreads and the gate at the end
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// MODE 0: x as 8 x dwordx4 rows;  1: x in the fragment layout (16 x dwordx2)
template <int MODE, int DEPTH, int BAR = 0, int NT = 256>
__global__ __launch_bounds__(NT) void skel_p(const float* __restrict__ x, const float* __restrict__ g,
                                              const f4* __restrict__ cv, float* __restrict__ dx, int T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = gridDim.x * (blockDim.x >> 6);
  const int t0 = blockIdx.x * (blockDim.x >> 6) + wave;
  if (BAR == 0 && t0 >= T) return;
  const int cnt = t0 < T ? (T - 1 - t0) / nw + 1 : 0;
  const int cnt_max = BAR ? (T - 1) / nw + 1 : cnt;
  const int li = lane & 31, hi = lane >> 5;
  f4 xr[DEPTH][8], gr[DEPTH][8], cr[DEPTH][2];
  auto issue = [&](int k, int slot) {
    const int t = cnt > 0 ? t0 + (k < cnt ? k : cnt - 1) * nw : 0;
    const f4* gs = reinterpret_cast<const f4*>(g + (long)t * 2048);
    if constexpr (MODE == 0) {
      const f4* xs = reinterpret_cast<const f4*>(x + (long)t * 2048);
#pragma unroll
      for (int q = 0; q < 8; ++q) xr[slot][q] = xs[lane + 64 * q];
    } else {
      const float* xb = x + (long)t * 2048 + (8 * hi) * 64 + 2 * li;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const f2 v = *reinterpret_cast<const f2*>((q >> 3 ? xb + 16 * 64 : xb) + (q & 7) * 64);
        xr[slot][q >> 1][2 * (q & 1)] = v[0];
        xr[slot][q >> 1][2 * (q & 1) + 1] = v[1];
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) gr[slot][q] = gs[lane + 64 * q];
    cr[slot][0] = cv[(long)t * 80 + lane];
    cr[slot][1] = lane < 16 ? cv[(long)t * 80 + 64 + lane] : f4{0, 0, 0, 0};
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) issue(d, d);
  for (int i = 0; i < cnt_max; i += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if (BAR == 0 && i + d >= cnt) break;
      const int t = t0 + (i + d) * nw;
      f4 o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = xr[d][q] * gr[d][q] + cr[d][q & 1];
      issue(i + d + DEPTH, d);
      if constexpr (BAR != 0) __syncthreads();
      float* dst = dx + (long)t * 2048;
      if (i + d < cnt) {
#pragma unroll
        for (int q = 0; q < 8; ++q)          // the C layout of dX^T = W dFW^T: lane = row, 32-byte segments at 256-byte stride
          *reinterpret_cast<f4*>(dst + li * 64 + (q >> 2) * 32 + 8 * (q & 3) + 4 * hi) = o[q];
      }
    }
  }
}

// pairs: wave 2p moves g + CSR in and dX out, wave 2p+1 moves x in (and hands a checksum over through LDS so that nothing is dead)
typedef float f16v __attribute__((ext_vector_type(16)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
// LOAD: synthetic arithmetic per wave and graph next to the memory streams (no LDS traffic, no dependence on the loaded data beyond a
// final select): 1 = 48 v_mfma_f32_32x32x16_bf16 (the kernel's 96 per graph over the pair), 2 = those + 400 v_fma_f32, 3 = 400 v_fma_f32 only
template <int DEPTH, int BAR = 1, int LOAD = 0, int NT = 0, int CONTIG = 0, int LATE = 0>
__global__ __launch_bounds__(512) void skel_h(const float* __restrict__ x, const float* __restrict__ g,
                                              const f4* __restrict__ cv, float* __restrict__ dx, int T) {
  __shared__ float hand[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave >> 1, role = wave & 1;
  const int npairs = gridDim.x * 4;
  const int t0 = blockIdx.x * 4 + pair;
  const int cnt_max = (T - 1) / npairs + 1;
  const int cnt = t0 < T ? (T - 1 - t0) / npairs + 1 : 0;
  const int li = lane & 31, hi = lane >> 5;
  f4 r[DEPTH][8], cr[DEPTH][2];
  f16v acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  bf8 fa, fb;
#pragma unroll
  for (int e = 0; e < 8; ++e) { fa[e] = (__bf16)(0.001f * (lane + e)); fb[e] = (__bf16)(0.002f * (lane - e)); }
  float va[8] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
  const float vm = 0.999f + 1e-9f * lane, vb = 1e-7f * lane;
  auto issue = [&](int k, int slot) {
    const int kk = k < cnt ? k : (cnt > 0 ? cnt - 1 : 0);
    int t = cnt > 0 ? t0 + kk * npairs : 0;
    if constexpr (CONTIG != 0) {                               // every pair walks a contiguous range of graphs instead of a strided one
      const long tc = (long)t0 * cnt_max + kk;
      t = (int)(tc < T ? tc : T - 1);
    }
    const f4* s = reinterpret_cast<const f4*>((role ? x : g) + (long)t * 2048);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if constexpr ((NT & 1) != 0) r[slot][q] = __builtin_nontemporal_load(s + lane + 64 * q);
      else r[slot][q] = s[lane + 64 * q];
    }
    if (!role) {
      cr[slot][0] = cv[(long)t * 80 + lane];
      cr[slot][1] = lane < 16 ? cv[(long)t * 80 + 64 + lane] : f4{0, 0, 0, 0};
    }
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) issue(d, d);
  for (int i = 0; i < cnt_max; i += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const bool live = i + d < cnt;
      f4 o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = r[d][q];
      if (role) {
        f4 s = o[0] + o[1] + o[2] + o[3] + o[4] + o[5] + o[6] + o[7];
        hand[wave][lane] = s[0] + s[1] + s[2] + s[3];
      }
      if constexpr (LATE == 0) issue(i + d + DEPTH, d);      // LATE: the next graph is requested BEHIND the arithmetic (as the kernel's roles do)
      if constexpr (LOAD == 1 || LOAD == 2 || LOAD == 5) {
#pragma unroll
        for (int m = 0; m < (LOAD == 5 ? 24 : 12); ++m) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc1, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc2, 0, 0, 0);
          acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc3, 0, 0, 0);
        }
      }
      if constexpr (LOAD == 4) {                              // the same 48 MFMAs and 400 v_fma_f32, one MFMA then eight v_fma_f32
#pragma unroll
        for (int m = 0; m < 12; ++m) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q == 0) acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc0, 0, 0, 0);
            if (q == 1) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc1, 0, 0, 0);
            if (q == 2) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc2, 0, 0, 0);
            if (q == 3) acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc3, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 8; ++e) va[e] = __builtin_fmaf(va[e], vm, vb);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if constexpr (LOAD == 2 || LOAD == 3) {
#pragma unroll
        for (int m = 0; m < 50; ++m) {
#pragma unroll
          for (int e = 0; e < 8; ++e) va[e] = __builtin_fmaf(va[e], vm, vb);
        }
      }
      if constexpr (LATE != 0) issue(i + d + DEPTH, d);
      if constexpr (BAR != 0) __syncthreads();   // one workgroup barrier per graph, as the two-role kernel would pay
      if (!role && live) {
        const float hv = hand[wave + 1][lane];
        long td = t0 + (long)(i + d) * npairs;
        if constexpr (CONTIG != 0) { td = (long)t0 * cnt_max + (i + d); if (td >= T) td = T - 1; }
        float* dst = dx + td * 2048;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const f4 val = o[q] * hv + cr[d][q & 1];
          f4* dp = reinterpret_cast<f4*>(dst + li * 64 + (q >> 2) * 32 + 8 * (q & 3) + 4 * hi);
          if constexpr ((NT & 2) != 0) __builtin_nontemporal_store(val, dp);
          else *dp = val;
        }
      }
    }
  }
  if constexpr (LOAD != 0) {
    float z = va[0] + va[1] + va[2] + va[3] + va[4] + va[5] + va[6] + va[7];
#pragma unroll
    for (int e = 0; e < 16; ++e) z += acc0[e] + acc1[e] + acc2[e] + acc3[e];
    if (z == 123.456f) dx[lane] = z;
  }
}

// non-persistent: one wave per graph, everything requested at once
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void skel_n(const float* __restrict__ x, const float* __restrict__ g,
                                                   const f4* __restrict__ cv, float* __restrict__ dx, int T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * WPB + wave;
  if (t >= T) return;
  const int li = lane & 31, hi = lane >> 5;
  const f4* xs = reinterpret_cast<const f4*>(x + (long)t * 2048);
  const f4* gs = reinterpret_cast<const f4*>(g + (long)t * 2048);
  f4 xr[8], gr[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { xr[q] = xs[lane + 64 * q]; gr[q] = gs[lane + 64 * q]; }
  const f4 c0 = cv[(long)t * 80 + lane];
  const f4 c1 = lane < 16 ? cv[(long)t * 80 + 64 + lane] : f4{0, 0, 0, 0};
  float* dst = dx + (long)t * 2048;
#pragma unroll
  for (int q = 0; q < 8; ++q)
    *reinterpret_cast<f4*>(dst + li * 64 + (q >> 2) * 32 + 8 * (q & 3) + 4 * hi) = xr[q] * gr[q] + ((q & 1) ? c1 : c0);
}

// forward: x + CSR in, out tile out (17,316 algorithmic bytes per graph).  ROLE 0: every wave reads and writes its graph;
// ROLE 1: pairs -- wave A reads x + CSR, wave B writes the tile (handed over through LDS), one barrier per graph
template <int ROLE, int BAR, int NT>
__global__ __launch_bounds__(NT) void skel_f(const float* __restrict__ x, const f4* __restrict__ cv, float* __restrict__ out, int T) {
  __shared__ f4 tile[NT / 64][8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int units = ROLE ? NT / 128 : NT / 64, unit = ROLE ? wave >> 1 : wave, role = ROLE ? wave & 1 : 0;
  const int nu = gridDim.x * units;
  const int t0 = blockIdx.x * units + unit;
  const int cnt = t0 < T ? (T - 1 - t0) / nu + 1 : 0;
  const int cnt_max = (T - 1) / nu + 1;
  f4 r[8], c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
  auto issue = [&](int k) {
    const int t = cnt > 0 ? t0 + (k < cnt ? k : cnt - 1) * nu : 0;
    if (ROLE == 0 || role == 0) {
      const f4* s = reinterpret_cast<const f4*>(x + (long)t * 2048);
#pragma unroll
      for (int q = 0; q < 8; ++q) r[q] = s[lane + 64 * q];
      c0 = cv[(long)t * 80 + lane];
      c1 = lane < 16 ? cv[(long)t * 80 + 64 + lane] : f4{0, 0, 0, 0};
    }
  };
  issue(0);
  for (int i = 0; i < (BAR || ROLE ? cnt_max : cnt); ++i) {
    f4 o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = r[q] + ((q & 1) ? c1 : c0);
    if constexpr (ROLE != 0) {
      if (role == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) tile[wave][q][lane] = o[q];
      }
    }
    issue(i + 1);
    if constexpr (BAR != 0 || ROLE != 0) __syncthreads();
    if (i < cnt) {
      f4* dst = reinterpret_cast<f4*>(out + (long)(t0 + i * nu) * 2048);
      if constexpr (ROLE != 0) {
        if (role == 1) {
#pragma unroll
          for (int q = 0; q < 8; ++q) dst[lane + 64 * q] = tile[wave - 1][q][lane];
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) dst[lane + 64 * q] = o[q];
      }
    } else if (ROLE != 0) {
      __syncthreads();
    }
  }
}

// forward, persistent, prefetch depth DEPTH (graphs in flight per wave beyond the one being written), NT threads per workgroup
template <int DEPTH, int NT>
__global__ __launch_bounds__(NT) void skel_fd(const float* __restrict__ x, const f4* __restrict__ cv, float* __restrict__ out, int T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = gridDim.x * (NT / 64);
  const int t0 = blockIdx.x * (NT / 64) + wave;
  if (t0 >= T) return;
  const int cnt = (T - 1 - t0) / nw + 1;
  f4 r[DEPTH][8], c0[DEPTH], c1[DEPTH];
  auto issue = [&](int k, int slot) {
    const int t = t0 + (k < cnt ? k : cnt - 1) * nw;
    const f4* s = reinterpret_cast<const f4*>(x + (long)t * 2048);
#pragma unroll
    for (int q = 0; q < 8; ++q) r[slot][q] = s[lane + 64 * q];
    c0[slot] = cv[(long)t * 80 + lane];
    c1[slot] = lane < 16 ? cv[(long)t * 80 + 64 + lane] : f4{0, 0, 0, 0};
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) issue(d, d);
  for (int i = 0; i < cnt; i += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if (i + d >= cnt) break;
      f4 o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = r[d][q] + ((q & 1) ? c1[d] : c0[d]);
      issue(i + d + DEPTH, d);
      f4* dst = reinterpret_cast<f4*>(out + (long)(t0 + (i + d) * nw) * 2048);
#pragma unroll
      for (int q = 0; q < 8; ++q) dst[lane + 64 * q] = o[q];
    }
  }
}

// ---- ingest arms: how a tile gets from HBM into LDS and how the result leaves ---------------------------------------------------
// global_load_lds_dwordx4: 1 KiB per wave-instruction, LDS destination = wave-uniform base + 16 x lane, no VGPR destination.
// AUX 2 = the nt cache-policy bit of gfx950.
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
template <int AUX>
__device__ __forceinline__ void glds16(const f4* src_lane, f4* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src_lane, (lptr_t)lds_wave_base, 16, 0, AUX);
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int NTS> __device__ __forceinline__ void st16(f4* p, f4 v) {
  if constexpr (NTS != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}
template <int NTS> __device__ __forceinline__ void st4(float* p, float v) {
  if constexpr (NTS != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}
// lanes 32-63 of a <-> lanes 0-31 of b (v_permlane32_swap_b32)
__device__ __forceinline__ void swap32(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
// the arithmetic stand-ins of skel_h: 48 bf16 MFMAs (one contraction) / 400 v_fma_f32 (one aggregation)
struct Standin {
  f16v acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  bf8 fa, fb;
  float va[8] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
  float vm, vb;
  __device__ __forceinline__ Standin(int lane) : vm(0.999f + 1e-9f * lane), vb(1e-7f * lane) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { fa[e] = (__bf16)(0.001f * (lane + e)); fb[e] = (__bf16)(0.002f * (lane - e)); }
  }
  __device__ __forceinline__ void mfmas() {
#pragma unroll
    for (int m = 0; m < 12; ++m) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc3, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void fmas() {
#pragma unroll
    for (int m = 0; m < 50; ++m) {
#pragma unroll
      for (int e = 0; e < 8; ++e) va[e] = __builtin_fmaf(va[e], vm, vb);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void keep(float* p, int lane) {
    float z = va[0] + va[1] + va[2] + va[3] + va[4] + va[5] + va[6] + va[7];
#pragma unroll
    for (int e = 0; e < 16; ++e) z += acc0[e] + acc1[e] + acc2[e] + acc3[e];
    if (z == 123.456f) p[lane] = z;
  }
};

// forward, the shipped structure (one persistent 512-thread workgroup per CU, no barrier), with the kernel's order of phases:
//   x(t) LDS -> registers, 48 MFMAs [contraction] | request x(t + nw) | 400 v_fma_f32 [aggregation], 8 x 1 KiB out stores, CSR
// GLDS 0: x and the CSR slice wait in registers (requested a whole step ahead, as shipped; the LDS round trip of the tile is the
//         kernel's land_tile + fragment reads);  1: x and the CSR slice by LDS-DMA into the wave's ONE tile buffer, requested once
//         the contraction stand-in has read it, retired by a counted vmcnt (the 8 younger stores stay in flight)
// NTL: nontemporal loads (GLDS: the nt policy bit);  NTS: nontemporal stores;  LOAD 0: no arithmetic (the pure byte pattern)
template <int GLDS, int NTL, int NTS, int LOAD>
__global__ __launch_bounds__(512) void skel_fi(const float* __restrict__ x, const f4* __restrict__ cv, float* __restrict__ out, int T) {
  __shared__ f4 tile[8][512 + 128];      // 80 KiB of static LDS: fits the 160 KiB of a gfx950 CU, not the 64 KiB of earlier parts
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = gridDim.x * 8;
  const int t0 = blockIdx.x * 8 + wave;
  if (t0 >= T) return;
  const int cnt = (T - 1 - t0) / nw + 1;
  f4* tl = tile[wave];
  Standin sa(lane);
  f4 r[8], c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
  auto issue = [&](int k) __attribute__((always_inline)) {
    const int t = t0 + (k < cnt ? k : cnt - 1) * nw;
    const f4* s = reinterpret_cast<const f4*>(x + (long)t * 2048);
    const f4* c = cv + (long)t * 80;
    if constexpr (GLDS != 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) glds16<NTL ? 2 : 0>(s + lane + 64 * q, tl + 64 * q);
      glds16<0>(c + lane, tl + 512);
      glds16<0>(c + (lane < 16 ? 64 + lane : lane), tl + 576);      // (lanes >= 16 re-read the first piece: one wave-instruction)
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) r[q] = NTL ? __builtin_nontemporal_load(s + lane + 64 * q) : s[lane + 64 * q];
      c0 = c[lane];
      c1 = lane < 16 ? c[64 + lane] : f4{0, 0, 0, 0};
    }
  };
  issue(0);
  for (int i = 0; i < cnt; ++i) {
    f4 o[8];
    if constexpr (GLDS != 0) {
      if (i == 0) wait_vm<0>(); else wait_vm<8>();                  // the tile and its CSR slice; the previous graph's stores stay in flight
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = tl[lane + 64 * q] + tl[512 + ((q & 1) ? 64 + (lane & 15) : lane)];
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) tl[lane + 64 * q] = r[q];         // land_tile
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = tl[lane + 64 * q] + ((q & 1) ? c1 : c0);
    }
    if constexpr (LOAD != 0) sa.mfmas();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the tile buffer has been read
    issue(i + 1);
    if constexpr (LOAD != 0) sa.fmas();
    f4* dst = reinterpret_cast<f4*>(out + (long)(t0 + i * nw) * 2048);
#pragma unroll
    for (int q = 0; q < 8; ++q) st16<NTS>(dst + lane + 64 * q, o[q]);
  }
  if constexpr (LOAD != 0) sa.keep(out, lane);
}

// backward pairs with role A's g tile and CSR slice by LDS-DMA into the pair's ONE gather tile: role A reads g(i+1) out of LDS,
// 400 v_fma_f32 [aggregation], requests g(i+2), 48 MFMAs [dX], the 8 dX stores, a counted vmcnt that retires the tile and leaves the
// stores in flight, the barrier (role B gathers from the tile right behind it).  Role B as in skel_h (x in registers, 48 MFMAs).
// GLDS 0: the same order of phases with g waiting in registers (requested behind the aggregation, landed in LDS before the barrier)
// DXF: the form of role A's dX stores, the 32 registers o[] read as the two 32 x 32 accumulators c0 = o[0..3], c1 = o[4..7]
//   0  dX^T = W dFW^T (lane = node, 4 consecutive features per register quad): 8 x dwordx4, 32-byte segments at 256-byte stride
//   1  dX = dFW W^T (lane = feature 32 nt + li, register 4 q + j = node 8 q + 4 hi + j) as it stands: 32 x dword, two 128-byte lines each
//   2  as 1 behind v_permlane32_swap(c0[r], c1[r]): c0[r] is node 8 q + j, c1[r] node 8 q + 4 + j, lane = feature: 32 x dword,
//      one 256-byte row each
template <int GLDS, int NTL, int NTS, int LOAD, int DXF = 0>
__global__ __launch_bounds__(512) void skel_hi(const float* __restrict__ x, const float* __restrict__ g,
                                               const f4* __restrict__ cv, float* __restrict__ dx, int T) {
  __shared__ float hand[8][64];
  __shared__ f4 gt[4][512 + 128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave >> 1, role = wave & 1;
  const int npairs = gridDim.x * 4;
  const int t0 = blockIdx.x * 4 + pair;
  const int cnt_max = (T - 1) / npairs + 1;
  const int cnt = t0 < T ? (T - 1 - t0) / npairs + 1 : 0;
  const int li = lane & 31, hi = lane >> 5;
  f4* tl = gt[pair];
  Standin sa(lane);
  f4 r[8], c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
  auto graph = [&](int k) { return cnt > 0 ? t0 + (k < cnt ? k : cnt - 1) * npairs : 0; };
  auto issue = [&](int k) __attribute__((always_inline)) {
    const int t = graph(k);
    const f4* s = reinterpret_cast<const f4*>((role ? x : g) + (long)t * 2048);
    const f4* c = cv + (long)t * 80;
    if (GLDS != 0 && !role) {
#pragma unroll
      for (int q = 0; q < 8; ++q) glds16<NTL ? 2 : 0>(s + lane + 64 * q, tl + 64 * q);
      glds16<0>(c + lane, tl + 512);
      glds16<0>(c + (lane < 16 ? 64 + lane : lane), tl + 576);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) r[q] = NTL ? __builtin_nontemporal_load(s + lane + 64 * q) : s[lane + 64 * q];
      if (!role) {
        c0 = c[lane];
        c1 = lane < 16 ? c[64 + lane] : f4{0, 0, 0, 0};
      }
    }
  };
  issue(0);
  if (!role) {
    if constexpr (GLDS != 0) {
      wait_vm<0>();
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) tl[lane + 64 * q] = r[q] + ((q & 1) ? c1 : c0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  for (int i = 0; i < cnt_max; ++i) {
    const bool live = i < cnt;
    f4 o[8];
    if (role) {
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = r[q];
      const f4 s = o[0] + o[1] + o[2] + o[3] + o[4] + o[5] + o[6] + o[7];
      hand[wave][lane] = s[0] + s[1] + s[2] + s[3] + tl[lane][0];   // role B reads the gather tile too
      if constexpr (LOAD != 0) sa.mfmas();
      issue(i + 1);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        o[q] = tl[lane + 64 * q];
        if constexpr (GLDS != 0) o[q] += tl[512 + ((q & 1) ? 64 + (lane & 15) : lane)];
      }
      if constexpr (LOAD != 0) sa.fmas();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      issue(i + 1);
      if constexpr (LOAD != 0) sa.mfmas();
      const float hv = hand[wave + 1][lane];
      float* dst = dx + (long)graph(i) * 2048;
      if (live) {
        if constexpr (DXF == 0) {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            st16<NTS>(reinterpret_cast<f4*>(dst + li * 64 + (q >> 2) * 32 + 8 * (q & 3) + 4 * hi), o[q] * hv);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v0 = o[r >> 2][r & 3] * hv, v1 = o[4 + (r >> 2)][r & 3] * hv;
            if constexpr (DXF == 1) {
              float* dp = dst + (8 * (r >> 2) + 4 * hi + (r & 3)) * 64 + li;
              st4<NTS>(dp, v0);
              st4<NTS>(dp + 32, v1);
            } else {
              swap32(v0, v1);
              float* dp = dst + (8 * (r >> 2) + (r & 3)) * 64 + lane;
              st4<NTS>(dp, v0);
              st4<NTS>(dp + 4 * 64, v1);
            }
          }
        }
      }
      if constexpr (GLDS != 0) {
        static_assert(DXF == 0, "the counted wait of the LDS-DMA arm assumes 8 stores");
        if (live) wait_vm<8>(); else wait_vm<0>();
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) tl[lane + 64 * q] = r[q] + ((q & 1) ? c1 : c0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  if constexpr (LOAD != 0) sa.keep(dx, lane);
}

// one stream alone, persistent, 8 waves per CU, 8 KiB tiles as 8 x 1 KiB wave-instructions: what a stored / a loaded byte costs
template <int NTS>
__global__ __launch_bounds__(512) void skel_w(float* __restrict__ out, int T) {
  const int lane = threadIdx.x & 63, nw = gridDim.x * 8;
  const f4 v = {1.f * lane, 2.f, 3.f, 4.f};
  for (int t = blockIdx.x * 8 + (threadIdx.x >> 6); t < T; t += nw) {
    f4* dst = reinterpret_cast<f4*>(out + (long)t * 2048);
#pragma unroll
    for (int q = 0; q < 8; ++q) st16<NTS>(dst + lane + 64 * q, v);
  }
}
// T tiles of each of a and b in (depth 1: the next pair of tiles is requested before the current one is summed)
template <int NTL>
__global__ __launch_bounds__(512) void skel_r(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int T) {
  const int lane = threadIdx.x & 63, nw = gridDim.x * 8;
  const int t0 = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (t0 >= T) return;
  f4 r[16], acc = {0, 0, 0, 0};
  auto issue = [&](int t) __attribute__((always_inline)) {
    const f4* sa = reinterpret_cast<const f4*>(a + (long)t * 2048);
    const f4* sb = reinterpret_cast<const f4*>(b + (long)t * 2048);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      r[q] = NTL ? __builtin_nontemporal_load(sa + lane + 64 * q) : sa[lane + 64 * q];
      r[8 + q] = NTL ? __builtin_nontemporal_load(sb + lane + 64 * q) : sb[lane + 64 * q];
    }
  };
  issue(t0);
  for (int t = t0; t < T; t += nw) {
    f4 s = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; ++q) s += r[q];
    issue(t + nw < T ? t + nw : t);
    acc += s;
  }
  if (acc[0] + acc[1] + acc[2] + acc[3] == 123.456f) out[lane] = acc[0];
}

// forward as reader | aggregator wave PAIRS (one persistent 512-thread workgroup per CU, four pairs), both streams nontemporal,
// ONE barrier per graph, the hand-over double-buffered in LDS.  In iteration i
//   role R: x(i) registers -> the pair's A tile, x(i + AHEAD) + CSR(i + AHEAD) requested, A tile read back, 48 MFMAs [contraction],
//           the product tile and CSR(i) -> gather buffer i & 1, barrier                                  (loads only on its vmcnt)
//   role W: gather buffer (i - 1) & 1 -> registers, 400 v_fma_f32 [aggregation], 8 x 1 KiB out stores of graph i - 1, barrier
//                                                                                                          (stores only on its vmcnt)
// PLACE 0: the two roles of a pair on the same SIMD (pair = wave & 3, role = wave >> 2, as graphconv_bwd_pairs_kernel);
//       1: on adjacent waves (pair = wave >> 1, role = wave & 1, as arm FH)
// AHEAD: tiles the reader holds in registers beyond the one it is landing (1 or 2);  LOAD as skel_fi
// Every wave runs the same number of iterations (barrier counts cannot differ); a pair that owns a graph less re-requests its last
// one and stores nothing for it.
template <int PLACE, int AHEAD, int LOAD>
__global__ __launch_bounds__(512) void skel_fp(const float* __restrict__ x, const f4* __restrict__ cv, float* __restrict__ out, int T) {
  __shared__ f4 at[4][512];               // 32 KiB
  __shared__ f4 gt[4][2][512 + 128];      // 80 KiB: 112 KiB of the 160 KiB of a gfx950 CU
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = PLACE ? wave >> 1 : wave & 3, role = PLACE ? wave & 1 : wave >> 2;      // role 0 = R, 1 = W
  const int npairs = gridDim.x * 4;
  const int t0 = blockIdx.x * 4 + pair;
  const int cnt_max = (T - 1) / npairs + 1;
  const int cnt = t0 < T ? (T - 1 - t0) / npairs + 1 : 0;
  const int steps = (cnt_max + 1 + AHEAD - 1) / AHEAD * AHEAD;      // + 1: the writer runs one graph behind the reader
  f4* ta = at[pair];
  Standin sa(lane);
  f4 r[AHEAD][8], c0[AHEAD], c1[AHEAD];
#pragma unroll
  for (int d = 0; d < AHEAD; ++d) { c0[d] = f4{0, 0, 0, 0}; c1[d] = f4{0, 0, 0, 0}; }
  auto graph = [&](int k) { return cnt > 0 ? t0 + (k < cnt ? k : cnt - 1) * npairs : 0; };
  auto issue = [&](int k, int slot) __attribute__((always_inline)) {
    const int t = graph(k);
    const f4* s = reinterpret_cast<const f4*>(x + (long)t * 2048);
    const f4* c = cv + (long)t * 80;
#pragma unroll
    for (int q = 0; q < 8; ++q) r[slot][q] = __builtin_nontemporal_load(s + lane + 64 * q);
    c0[slot] = c[lane];
    c1[slot] = lane < 16 ? c[64 + lane] : f4{0, 0, 0, 0};
  };
  // the roles run loops of their own, as in graphconv_bwd_pairs_kernel (one loop with role branches inside makes the reader's tile
  // registers a merge of two paths, and the copies behind the merge wait for the loads just requested: s_waitcnt vmcnt(0) per graph)
  if (!role) {
#pragma unroll
    for (int d = 0; d < AHEAD; ++d) issue(d, d);
    for (int i = 0; i < steps; i += AHEAD) {
#pragma unroll
      for (int d = 0; d < AHEAD; ++d) {
        f4* tg = gt[pair][(i + d) & 1];
#pragma unroll
        for (int q = 0; q < 8; ++q) ta[lane + 64 * q] = r[d][q];    // land_tile
        tg[512 + lane] = c0[d];                                     // CSR(i) -> the slice of buffer i & 1
        if (lane < 16) tg[576 + lane] = c1[d];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue(i + d + AHEAD, d);       // nothing that was loaded lives across the request: the loads land in the registers they left
        f4 o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = ta[lane + 64 * q];       // the fragment reads
        if constexpr (LOAD != 0) sa.mfmas();
#pragma unroll
        for (int q = 0; q < 8; ++q) tg[lane + 64 * q] = o[q];       // the product tile
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
  } else {
    for (int i = 0; i < steps; ++i) {
      if (i > 0) {
        const f4* tp = gt[pair][(i - 1) & 1];
        f4 o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = tp[lane + 64 * q] + tp[512 + ((q & 1) ? 64 + (lane & 15) : lane)];
        if constexpr (LOAD != 0) sa.fmas();
        if (i - 1 < cnt) {
          f4* dst = reinterpret_cast<f4*>(out + (long)graph(i - 1) * 2048);
#pragma unroll
          for (int q = 0; q < 8; ++q) st16<1>(dst + lane + 64 * q, o[q]);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
  if constexpr (LOAD != 0) sa.keep(out, lane);
}

static float* X; static float* G; static float* DX; static f4* CV; static int T;
template <typename L>
static float timeit(L launch) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int w = 0; w < 5; ++w) launch();
  hipEventRecord(e0);
  for (int r = 0; r < 20; ++r) launch();
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  return ms / 20;
}
static void linef(const char* name, float ms) {
  const double bytes = (double)T * (8192 * 2 + 932);
  printf("  %-64s %.3f ms  %.0f GB/s  %.3f of 8 TB/s\n", name, ms, bytes / ms / 1e6, bytes / ms / 1e6 / 8000.0);
  fflush(stdout);
}
static void lineb(const char* name, float ms, double bytes) {
  printf("  %-64s %.3f ms  %.0f GB/s (%.0f MB per launch)\n", name, ms, bytes / ms / 1e6, bytes / 1e6);
  fflush(stdout);
}
static void line(const char* name, float ms) {
  const double bytes = (double)T * (8192 * 3 + 932);           // the kernel's ALGORITHMIC bytes (the skeleton reads 1,280 B of CSR)
  printf("  %-64s %.3f ms  %.0f GB/s  %.3f of 8 TB/s\n", name, ms, bytes / ms / 1e6, bytes / ms / 1e6 / 8000.0);
  fflush(stdout);
}

int main(int argc, char** argv) {
  T = argc > 1 ? atoi(argv[1]) : 100000;
  const size_t tb = (size_t)T * 8192;
  hipMalloc(&X, tb); hipMalloc(&G, tb); hipMalloc(&DX, tb); hipMalloc(&CV, (size_t)T * 1280);
  hipMemset(X, 0x11, tb); hipMemset(G, 0x22, tb); hipMemset(CV, 0, (size_t)T * 1280);
  printf("graphs = %d, algorithmic bytes per graph 25,508\n", T);
  char nm[128];
  const bool ingest = argc > 2 && !strcmp(argv[2], "ingest");   // only the ingest arms, next to the best existing arm of each direction
  const bool dxstore = argc > 2 && !strcmp(argv[2], "dxstore");
  const bool fwdpairs = argc > 2 && !strcmp(argv[2], "fwdpairs");
  if (fwdpairs) {
    constexpr int NA = 10, NR = 3;
    const char* names[NA] = {
        "F   512-thread workgroup, kernel order, nt loads and stores (reference)",
        "FP  pairs, roles on the same SIMD, reader 1 tile ahead",
        "FP  pairs, roles on adjacent waves, reader 1 tile ahead",
        "FP  pairs, roles on the same SIMD, reader 2 tiles ahead",
        "FP  pairs, roles on adjacent waves, reader 2 tiles ahead",
        "F   + 48 MFMAs + 400 FMAs per wave and graph (reference)",
        "FP  + 48 MFMAs (reader) + 400 FMAs (writer), same SIMD, 1 ahead",
        "FP  + 48 MFMAs (reader) + 400 FMAs (writer), adjacent waves, 1 ahead",
        "FP  + 48 MFMAs (reader) + 400 FMAs (writer), same SIMD, 2 ahead",
        "FP  + 48 MFMAs (reader) + 400 FMAs (writer), adjacent waves, 2 ahead"};
    float ms[NA][NR];
    for (int rep = 0; rep < NR; ++rep) {
      int a = 0;
#define FR(A_) ms[a][rep] = timeit([&] { hipLaunchKernelGGL((skel_fi<0, 1, 1, A_>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }); \
    linef(names[a], ms[a][rep]); ++a
#define FP(P_, D_, A_) ms[a][rep] = timeit([&] { hipLaunchKernelGGL((skel_fp<P_, D_, A_>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }); \
    linef(names[a], ms[a][rep]); ++a
      FR(0); FP(0, 1, 0); FP(1, 1, 0); FP(0, 2, 0); FP(1, 2, 0);
      FR(1); FP(0, 1, 1); FP(1, 1, 1); FP(0, 2, 1); FP(1, 2, 1);
#undef FR
#undef FP
    }
    const hipError_t err = hipDeviceSynchronize();
    if (err != hipSuccess) { printf("HIP error: %s\n", hipGetErrorString(err)); return 1; }
    printf("median / min / max of the %d repetitions (ms)\n", NR);
    float med[NA], spread = 0.f;
    for (int a = 0; a < NA; ++a) {
      float lo = ms[a][0], hi = ms[a][0], sum = 0.f;
      for (int rep = 0; rep < NR; ++rep) { lo = ms[a][rep] < lo ? ms[a][rep] : lo; hi = ms[a][rep] > hi ? ms[a][rep] : hi; sum += ms[a][rep]; }
      med[a] = sum - lo - hi;
      if (a >= NA / 2 && hi - lo > spread) spread = hi - lo;
      printf("  %-72s %.4f  %.4f  %.4f\n", names[a], med[a], lo, hi);
    }
    int best = NA / 2 + 1;
    for (int a = NA / 2 + 1; a < NA; ++a) if (med[a] < med[best]) best = a;
    const float gain = med[NA / 2] - med[best];
    printf("gate: F beside the arithmetic %.4f ms, best pair arm %.4f ms (%s), difference %.4f ms, widest spread of the arms beside the\n"
           "      arithmetic %.4f ms: the gate (difference > 2 x spread) %s\n",
           med[NA / 2], med[best], names[best], gain, spread, gain > 2.f * spread ? "PASSES" : "FAILS");
  }
  else if (dxstore) for (int rep = 0; rep < 3; ++rep) {
#define HD(S_, A_, F_, name) \
    line(name, timeit([&] { hipLaunchKernelGGL((skel_hi<0, 0, S_, A_, F_>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }))
    HD(0, 0, 0, "HI pairs, S0 8 x dwordx4, 32-byte segments (shipped)");
    HD(1, 0, 0, "HI pairs, S0 nontemporal");
    HD(0, 0, 1, "HI pairs, S1 32 x dword, two 128-byte lines each");
    HD(1, 0, 1, "HI pairs, S1 nontemporal");
    HD(0, 0, 2, "HI pairs, S2 permlane32_swap, 32 x dword, one 256-byte row each");
    HD(1, 0, 2, "HI pairs, S2 nontemporal");
    HD(0, 1, 0, "HI + MFMAs + FMAs, S0 (shipped)");
    HD(1, 1, 0, "HI + MFMAs + FMAs, S0 nontemporal");
    HD(0, 1, 1, "HI + MFMAs + FMAs, S1");
    HD(1, 1, 1, "HI + MFMAs + FMAs, S1 nontemporal");
    HD(0, 1, 2, "HI + MFMAs + FMAs, S2");
    HD(1, 1, 2, "HI + MFMAs + FMAs, S2 nontemporal");
#undef HD
    lineb("W  write-only stream, 1 KiB per wave-instruction",
          timeit([&] { hipLaunchKernelGGL((skel_w<0>), dim3(256), dim3(512), 0, 0, DX, T); }), (double)T * 8192);
    lineb("W  write-only stream, nontemporal",
          timeit([&] { hipLaunchKernelGGL((skel_w<1>), dim3(256), dim3(512), 0, 0, DX, T); }), (double)T * 8192);
    lineb("R  read-only stream (two tensors), 1 KiB per wave-instruction",
          timeit([&] { hipLaunchKernelGGL((skel_r<0>), dim3(256), dim3(512), 0, 0, X, G, DX, T); }), (double)T * 16384);
    lineb("R  read-only stream (two tensors), nontemporal",
          timeit([&] { hipLaunchKernelGGL((skel_r<1>), dim3(256), dim3(512), 0, 0, X, G, DX, T); }), (double)T * 16384);
  }
  else if (ingest) for (int rep = 0; rep < 3; ++rep) {
#define FI(G_, L_, S_, A_, name) \
    linef(name, timeit([&] { hipLaunchKernelGGL((skel_fi<G_, L_, S_, A_>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }))
#define HI(G_, L_, S_, A_, name) \
    line(name, timeit([&] { hipLaunchKernelGGL((skel_hi<G_, L_, S_, A_>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }))
    linef("F  forward: persistent, 8 waves/CU (2 x 256-thread workgroups), no barrier",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 0, 256>), dim3(512), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("F  forward: persistent, 8 waves/CU (512-thread workgroup), no barrier",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 0, 512>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }));
    FI(0, 0, 0, 0, "FI forward, kernel order, registers + land_tile");
    FI(1, 0, 0, 0, "FI forward, kernel order, (a) LDS-DMA single buffer");
    FI(0, 0, 1, 0, "FI forward, kernel order, (b) nontemporal stores");
    FI(0, 1, 0, 0, "FI forward, kernel order, (c) nontemporal loads");
    FI(1, 1, 0, 0, "FI forward, kernel order, (a+c) LDS-DMA with the nt policy bit");
    FI(1, 0, 1, 0, "FI forward, kernel order, (d) LDS-DMA + nontemporal stores");
    FI(0, 1, 1, 0, "FI forward, kernel order, (b+c) nontemporal loads and stores");
    FI(0, 0, 0, 1, "FI + 48 MFMAs + 400 FMAs, registers + land_tile");
    FI(1, 0, 0, 1, "FI + 48 MFMAs + 400 FMAs, (a) LDS-DMA single buffer");
    FI(0, 0, 1, 1, "FI + 48 MFMAs + 400 FMAs, (b) nontemporal stores");
    FI(0, 1, 0, 1, "FI + 48 MFMAs + 400 FMAs, (c) nontemporal loads");
    FI(1, 1, 0, 1, "FI + 48 MFMAs + 400 FMAs, (a+c) LDS-DMA with the nt policy bit");
    FI(1, 0, 1, 1, "FI + 48 MFMAs + 400 FMAs, (d) LDS-DMA + nontemporal stores");
    FI(0, 1, 1, 1, "FI + 48 MFMAs + 400 FMAs, (b+c) nontemporal loads and stores");
    line("H  pairs (g+CSR+dX | x), depth 1, 8 waves/CU, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 48 bf16 MFMAs + 400 v_fma_f32 per wave and graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + MFMAs + FMAs, the next graph requested BEHIND the arithmetic",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2, 0, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    HI(0, 0, 0, 0, "HI pairs, role-A order agg | request | dX, g in registers");
    HI(1, 0, 0, 0, "HI pairs, role-A order agg | request | dX, (a) g by LDS-DMA");
    HI(0, 0, 1, 0, "HI pairs, (b) nontemporal dX stores");
    HI(0, 1, 0, 0, "HI pairs, (c) nontemporal loads");
    HI(1, 1, 0, 0, "HI pairs, (a+c) g by LDS-DMA with the nt policy bit");
    HI(0, 0, 0, 1, "HI + MFMAs + FMAs, g in registers");
    HI(1, 0, 0, 1, "HI + MFMAs + FMAs, (a) g by LDS-DMA");
    HI(0, 0, 1, 1, "HI + MFMAs + FMAs, (b) nontemporal dX stores");
    HI(0, 1, 0, 1, "HI + MFMAs + FMAs, (c) nontemporal loads");
    HI(1, 1, 0, 1, "HI + MFMAs + FMAs, (a+c) g by LDS-DMA with the nt policy bit");
    HI(1, 0, 1, 1, "HI + MFMAs + FMAs, (d) g by LDS-DMA + nontemporal dX stores");
#undef FI
#undef HI
  }
  else for (int rep = 0; rep < 2; ++rep) {
    for (int wpc : {4, 8, 12}) {
      const int blocks = 256 * wpc / 4;
      snprintf(nm, sizeof nm, "P  persistent, depth 2, %2d waves/CU", wpc);
      line(nm, timeit([&] { hipLaunchKernelGGL((skel_p<0, 2>), dim3(blocks), dim3(256), 0, 0, X, G, CV, DX, T); }));
      snprintf(nm, sizeof nm, "P  persistent, depth 1, %2d waves/CU", wpc);
      line(nm, timeit([&] { hipLaunchKernelGGL((skel_p<0, 1>), dim3(blocks), dim3(256), 0, 0, X, G, CV, DX, T); }));
      snprintf(nm, sizeof nm, "PX persistent, depth 1, x in fragment layout, %2d waves/CU", wpc);
      line(nm, timeit([&] { hipLaunchKernelGGL((skel_p<1, 1>), dim3(blocks), dim3(256), 0, 0, X, G, CV, DX, T); }));
    }
    line("H  pairs (g+CSR+dX | x), depth 1, 8 waves/CU, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs (g+CSR+dX | x), depth 2, 8 waves/CU, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<2>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, depth 2, 16 waves/CU",
         timeit([&] { hipLaunchKernelGGL((skel_h<2>), dim3(512), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, every pair a CONTIGUOUS range of graphs",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 0, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + MFMAs + FMAs, contiguous ranges",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + MFMAs + FMAs, the next graph requested BEHIND the arithmetic",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2, 0, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, the next graph requested just before the barrier (no arithmetic)",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 0, 0, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, nontemporal LOADS",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 0, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, nontemporal STORES",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 0, 2>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, nontemporal loads and stores",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 0, 3>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + MFMAs + FMAs, nontemporal loads",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 48 bf16 MFMAs per wave and graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 1>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 48 bf16 MFMAs + 400 v_fma_f32 per wave and graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 2>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 48 MFMAs and 400 v_fma_f32 INTERLEAVED (1 : 8)",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 4>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 96 bf16 MFMAs per wave and graph (twice the kernel's)",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 5>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs + 400 v_fma_f32 per wave and graph",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 1, 3>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("H  pairs, depth 1, 8 waves/CU, NO barrier",
         timeit([&] { hipLaunchKernelGGL((skel_h<1, 0>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("PB persistent, depth 1, 4 waves/CU, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_p<0, 1, 1, 256>), dim3(256), dim3(256), 0, 0, X, G, CV, DX, T); }));
    line("PB persistent, depth 1, x in fragment layout, 4 waves/CU, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_p<1, 1, 1, 256>), dim3(256), dim3(256), 0, 0, X, G, CV, DX, T); }));
    line("PB persistent, depth 1, 8 waves/CU as ONE 512-thread workgroup, barrier per graph",
         timeit([&] { hipLaunchKernelGGL((skel_p<0, 1, 1, 512>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    line("P  persistent, depth 1, 8 waves/CU as ONE 512-thread workgroup, no barrier",
         timeit([&] { hipLaunchKernelGGL((skel_p<0, 1, 0, 512>), dim3(256), dim3(512), 0, 0, X, G, CV, DX, T); }));
    linef("F  forward: persistent, 8 waves/CU (512-thread workgroup), no barrier",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 0, 512>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }));
    linef("F  forward: persistent, 8 waves/CU (2 x 256-thread workgroups), no barrier",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 0, 256>), dim3(512), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 1, 8 waves/CU (2 x 256)",
          timeit([&] { hipLaunchKernelGGL((skel_fd<1, 256>), dim3(512), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 2, 8 waves/CU (2 x 256)",
          timeit([&] { hipLaunchKernelGGL((skel_fd<2, 256>), dim3(512), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 3, 8 waves/CU (2 x 256)",
          timeit([&] { hipLaunchKernelGGL((skel_fd<3, 256>), dim3(512), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 1, 16 waves/CU",
          timeit([&] { hipLaunchKernelGGL((skel_fd<1, 256>), dim3(1024), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 1, 32 waves/CU",
          timeit([&] { hipLaunchKernelGGL((skel_fd<1, 256>), dim3(2048), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: persistent, depth 2, 16 waves/CU",
          timeit([&] { hipLaunchKernelGGL((skel_fd<2, 256>), dim3(1024), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FD forward: NON persistent, one wave per graph (64-thread workgroups)",
          timeit([&] { hipLaunchKernelGGL((skel_fd<1, 64>), dim3(T), dim3(64), 0, 0, X, CV, DX, T); }));
    linef("FB forward: persistent, 8 waves/CU (512-thread workgroup), barrier per graph",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 1, 512>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }));
    linef("FB forward: persistent, 4 waves/CU, barrier per graph",
          timeit([&] { hipLaunchKernelGGL((skel_f<0, 1, 256>), dim3(256), dim3(256), 0, 0, X, CV, DX, T); }));
    linef("FH forward: pairs (x + CSR in | tile out via LDS), 8 waves/CU",
          timeit([&] { hipLaunchKernelGGL((skel_f<1, 1, 512>), dim3(256), dim3(512), 0, 0, X, CV, DX, T); }));
    linef("FH forward: pairs, 16 waves/CU",
          timeit([&] { hipLaunchKernelGGL((skel_f<1, 1, 512>), dim3(512), dim3(512), 0, 0, X, CV, DX, T); }));
    line("N  one wave per graph, 64-thread workgroups",
         timeit([&] { hipLaunchKernelGGL((skel_n<1>), dim3(T), dim3(64), 0, 0, X, G, CV, DX, T); }));
    line("N  one wave per graph, 256-thread workgroups",
         timeit([&] { hipLaunchKernelGGL((skel_n<4>), dim3((T + 3) / 4), dim3(256), 0, 0, X, G, CV, DX, T); }));
  }
  return 0;
}
