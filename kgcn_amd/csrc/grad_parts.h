// The workspace of a layer's weight-gradient partials, as dense.hip and fused.hip carve it: nparts partials of dW [n_dw] | nparts
// of dbias [n_db] | nextra further floats.  The counts that sized the arrays are the ones the second stage is given.
#pragma once

#include "workspace.h"

namespace kgcn {

struct GradParts { int nparts; long n_dw, n_db; float *part_dw, *part_db, *extra; size_t bytes; };
inline GradParts grad_parts_layout(void* base, int nparts, long n_dw, long n_db, size_t nextra = 0) {
  Taker t(base, 4);
  GradParts w{nparts, n_dw, n_db, nullptr, nullptr, nullptr, 0};
  w.part_dw = t.take<float>((size_t)nparts * n_dw);
  w.part_db = t.take<float>((size_t)nparts * n_db);
  w.extra = t.take<float>(nextra);
  w.bytes = t.off;
  return w;
}
// nparts: how many partials the launch wrote (<= w.nparts)
inline int reduce_grad_parts(const GradParts& w, int nparts, float* dw, float* dbias, hipStream_t s) {
  return launch_reduce_pair(w.part_dw, w.n_dw, dw, w.part_db, w.n_db, dbias, nparts, s);
}

}  // namespace kgcn
