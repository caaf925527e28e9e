// Cross-file launchers and predicates of the dense-layer family: dense.hip routes a call (fwd_route / wgrad_route) to one of
// the kernels of gemm3 / gemmh / gemmb / gemmn / wgradn / wgradx / narrow / skinny, wtable.hip writes the weight tables they read.
// The defining file and every caller include this header, so a changed parameter list fails at compile time and not at dlopen
// (-shared accepts undefined symbols).  Default arguments live here only.
// Predicates take the alignment facts of an operand as plain values (x16: its base is 16-byte aligned) so that the reporting
// functions of the ABI can ask them without a pointer.
#pragma once

#include "kgcn_common.h"

namespace kgcn {

// ---- wtable.hip: W pre-split into MFMA fragment order (bf16 three-piece section, then the f16 two-piece section) ----------
int64_t wtable_bf16_bytes(int din, int dout);
int64_t wtable_bytes(int din, int dout);
void launch_wtable_split(const float* w, long w_ld, int trans_w, int din, int dout, void* workspace, hipStream_t s);

// ---- the backward operand of the wide kernels (gemm3 / gemmh / gemmb), passed by value in their arguments ---------------------
// The contraction's operand is dpre = (grad [+ d pooled of the row's graph]) (.) act'(act_out).  The staging threads address
// everything relative to the row they read (`base` = grad, or act_out where the read-out's gradient is all there is): the saved
// output lies `ydiff` and the d pre-activation to write `pdiff` elements away; act' = c0 + c1 a + c2 a^2 (sigmoid 0, 1, -1;
// tanh 1, 0, -1; relu is a template argument); bc != nullptr: row r adds bc[(r / bc_n) * bc_ld + .], bc_only: and has no grad.
// (G3Dact after its first user; the name is part of the kernels' symbols.  gemmh.h's GhDact adds `dot_part` behind it.)
struct G3Dact { long ydiff, pdiff; float c0, c1, c2; const float* bc; long bc_ld; int bc_n, bc_only; };
inline const float* dact_base(const float* grad, const float* act_out) { return grad ? grad : act_out; }
inline G3Dact dact_operands(const float* grad, const float* act_out, const float* dpre, const float* pooled_grad, long pooled_ld,
                            int n_nodes, int dact) {
  const float* base = dact_base(grad, act_out);
  G3Dact da{};
  da.ydiff = act_out ? act_out - base : 0;
  da.pdiff = dpre ? dpre - base : 0;
  da.c0 = dact == KGCN_ACT_TANH ? 1.f : 0.f;
  da.c1 = dact == KGCN_ACT_SIGMOID ? 1.f : 0.f;
  da.c2 = -1.f;
  da.bc = pooled_grad;
  da.bc_ld = pooled_ld;
  da.bc_n = n_nodes > 0 ? n_nodes : 1;
  da.bc_only = grad ? 0 : 1;
  return da;
}

// ---- gemm3.hip: bf16 three-piece GEMMs of the wide layers -----------------------------------------------------------------
// table == nullptr: W is split inside the kernel; else `table` is the fragment table of wtable.hip for (w, trans_w)
int launch_gemm3_fwd(const float* x, long m, int din, long x_ld, const float* w, long w_ld, int trans_w, const float* bias,
                     float* y, int dout, long y_ld, int act, const void* table, hipStream_t s);
int launch_gemm3_dx_dact(const float* grad, const float* act_out, float* dpre, long m, int k, long ld, const void* table,
                         float* dx, int n, long dx_ld, int dact, hipStream_t s, const float* pooled_grad = nullptr,
                         int n_nodes = 0, long pooled_ld = 0);
int launch_gemm3_wgrad(const float* x, long x_ld, const float* dy, long dy_ld, long m, int din, int dout, float* part_dw,
                       float* part_db, int nblocks, hipStream_t s, const float* yact = nullptr, int act = KGCN_ACT_NONE);

// ---- gemmh.hip: f16 two-piece GEMMs; `tabh` is the f16 section of the table (table + wtable_bf16_bytes) ---------------------
bool gemmh_fwd_ok(bool x16, long m, int din, long x_ld, int dout);
int launch_gemmh_fwd(const float* x, long m, int din, long x_ld, const void* tabh, const float* bias, float* y, int dout,
                     long y_ld, int act, hipStream_t s);
int launch_gemmh_dx_dact(const float* grad, const float* act_out, float* dpre, long m, int k, long ld, const void* tabh,
                         float* dx, int n, long dx_ld, int dact, hipStream_t s, const float* pooled_grad, int n_nodes,
                         long pooled_ld, float* dot_part);
int gemmh_dot_parts(long m, int dout);
bool gemmh_wgrad_ok(int din, int dout, long m);
int launch_gemmh_wgrad(const float* x, long x_ld, const float* dy, long dy_ld, long m, int din, int dout, float* part_dw,
                       float* part_db, int nblocks, hipStream_t s, const float* yact, int act);

// ---- gemmb.hip: one-pass backward (dX, dW, dbias) of a wide layer -------------------------------------------------------------
int launch_gemmb(const float* grad, const float* act_out, long m, int din, int dout, long ld, const float* x, long x_ld,
                 const void* tabh, float* dx, long dx_ld, float* part_dw, float* part_db, int dact, const float* pooled_grad,
                 int n_nodes, long pooled_ld, hipStream_t s, float* dot_part);

// ---- gemmn.hip / wgradn.hip: wide input, narrow output (256 -> 50) ------------------------------------------------------------
bool gemmn_pays(bool x16, int din, long x_ld, int dout);
int launch_gemmn_fwd(const float* x, long m, int din, long x_ld, const void* table, const float* bias, float* y, int dout,
                     long y_ld, int act, hipStream_t s);
bool wgradn_ok(bool x16, int din, long x_ld, int dout);
int launch_wgradn(const float* x, long x_ld, const float* dy, long dy_ld, long m, int din, int dout, float* part_dw,
                  float* part_db, int nblocks, hipStream_t s);

// ---- wgradx.hip: weight gradient of a narrow input, wide output (81 -> 256) ---------------------------------------------------
bool wgradx_ok(int din, int dout);
int launch_wgradx(const float* x, long x_ld, const float* dy, long dy_ld, long m, int din, int dout, float* part_dw,
                  float* part_db, int nparts, hipStream_t s, const float* yact, int act);

// ---- narrow.hip: 50-wide layers (contiguous rows, a width that is no multiple of 4) -------------------------------------------
bool narrow_fwd_ok(bool x16, int din, long x_ld, bool y16, int dout, long y_ld);
int launch_narrow_fwd(const float* x, long m, int din, const float* w, long w_ld, int trans_w, const float* bias, float* y,
                      int dout, int act, hipStream_t s);
bool narrow_wgrad_ok(bool x16, int din, long x_ld, bool dy16, int dout, long dy_ld);
int launch_narrow_wgrad(const float* x, const float* dy, long m, int din, int dout, float* part_dw, float* part_db,
                        int nblocks, hipStream_t s);

// ---- skinny.hip: read-out layers (2..16 columns on one side) -----------------------------------------------------------------
bool skinny_n_ok(int din, int dout, int trans_w);
bool skinny_k_ok(int din, int dout);
int launch_skinny_n_fwd(const float* x, long m, int din, long x_ld, const float* w, long w_ld, const float* bias, float* y,
                        int dout, long y_ld, int act, hipStream_t s);
int launch_skinny_k_fwd(const float* x, long m, int din, long x_ld, const float* w, long w_ld, int trans_w, const float* bias,
                        float* y, int dout, long y_ld, int act, hipStream_t s);
int skinny_wgrad_parts(long m);
int launch_skinny_n_wgrad(const float* x, long m, int din, long x_ld, const float* g, long g_ld, int dout, float* part_dw,
                          float* part_db, int nparts, hipStream_t s);

}  // namespace kgcn
