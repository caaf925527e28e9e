// The 64 x 64 fp64 Gram tile of a 256-thread workgroup (graphkern.hip's count Gram, labelprop.hip's affinity).  The header is
// compiled under the including file's own -ffp-contract flag.
#pragma once

#include "kgcn_common.h"

namespace kgcn {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;            // tile edge of a workgroup
constexpr int kKc = 16;              // k values staged per step
constexpr int kLd = kKc + 1;

// acc += A . B^T over k in [0, kext): four waves, wave (wr, wc) = (wv >> 1, wv & 1) a 32 x 32 block = 2 x 2 MFMA blocks.
// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15], and result r of the lane is
// C[row (l >> 4) + 4 r][col l & 15]: acc[x][y][r] is entry (wr 32 + x 16 + (l >> 4) + 4 r, wc 32 + y 16 + (l & 15)) of the tile.
// stage_a / stage_b (row in tile, k0, kk) return element k = k0 + kk of the row of the A / B panel; kKc values of k are staged at a
// time in as / bs [kTile * kLd] of E, converted to double where a fragment is read, and fed to the MFMA 4 at a time.  k comes in
// two parts because a caller adds them to a 64-bit row offset one after the other: with k added up first in 32 bits the compiler
// forms other addresses, and the matrix-free kernels of labelprop.hip ran 4 to 7 % slower (profiles/classical_device_fold.txt).
// The caller initialises acc; the panels are free again on return.
template <typename E, typename StageA, typename StageB>
__device__ __forceinline__ void gram_tile_64(E* as, E* bs, int kext, StageA stage_a, StageB stage_b, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, hi = lane >> 4, wr = wv >> 1, wc = wv & 1;
  const int kk = tid & (kKc - 1);
  for (int k0 = 0; k0 < kext; k0 += kKc) {
    for (int r = tid >> 4; r < kTile; r += 16) {
      as[r * kLd + kk] = stage_a(r, k0, kk);
      bs[r * kLd + kk] = stage_b(r, k0, kk);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kKc; s += 4) {
      double a[2], b[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        a[q] = (double)as[(wr * 32 + q * 16 + li) * kLd + s + hi];
        b[q] = (double)bs[(wc * 32 + q * 16 + li) * kLd + s + hi];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b[q], acc[p][q], 0, 0, 0);
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace kgcn
