// Taker (kgcn_amd/csrc/workspace.h) on the host, at the alignments the library carves with (4, 16, 256) and at 4 with a switch to
// 16 before the last array (the batch-normalisation layout): for a few thousand tuples of four counts, 0 and counts whose byte
// size is no multiple of the alignment included, over element types of 1, 4 and 8 bytes,
//   the sizing pass (NULL base) and the carving pass end at the same offset;
//   every array starts on its alignment;
//   the arrays are disjoint, in order, and inside the total.
// A host program of its own:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=undefined,address -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/workspace_layout_check.cpp -o /tmp/workspace_layout_check && /tmp/workspace_layout_check
#include <vector>

#include "../../kgcn_amd/csrc/workspace.h"

namespace kgcn {                      // what workspace.h's refusals link against in the library
int fail(const char*, ...) { return 1; }
}  // namespace kgcn

static long bad = 0, checked = 0;

struct Array { size_t begin, bytes, align; };

// one layout: four arrays of the element sizes in `elem`, the last one carved at `last_align`
static size_t carve(unsigned char* base, size_t align, size_t last_align, const size_t count[4], const int elem[4], Array out[4]) {
  kgcn::Taker t(base, align);
  for (int i = 0; i < 4; ++i) {
    if (i == 3) t.align = last_align;
    unsigned char* p = elem[i] == 1 ? t.take<unsigned char>(count[i])
                     : elem[i] == 4 ? reinterpret_cast<unsigned char*>(t.take<float>(count[i]))
                                    : reinterpret_cast<unsigned char*>(t.take<long>(count[i]));
    out[i] = Array{base ? (size_t)(p - base) : 0, count[i] * (size_t)elem[i], t.align};
    if (!base && p) ++bad;            // a sizing pass hands out no pointer
  }
  return t.off;
}

static void check(size_t align, size_t last_align, const size_t count[4], const int elem[4]) {
  Array sized[4], got[4];
  const size_t total = carve(nullptr, align, last_align, count, elem, sized);
  std::vector<unsigned char> buffer(total + 1);                // + 1: a total of 0 still has a base
  const size_t end = carve(buffer.data(), align, last_align, count, elem, got);
  ++checked;
  bool ok = end == total;
  size_t cursor = 0;
  for (int i = 0; i < 4; ++i) {
    ok = ok && got[i].begin % got[i].align == 0 && got[i].begin >= cursor && got[i].begin + got[i].bytes <= total;
    cursor = got[i].begin + got[i].bytes;
    for (size_t b = 0; ok && b < got[i].bytes; b += got[i].bytes > 64 ? got[i].bytes - 1 : 1) buffer[got[i].begin + b] = (unsigned char)i;   // inside the buffer
  }
  if (!ok && bad++ < 10)
    printf("align %zu/%zu counts %zu %zu %zu %zu: sized %zu, carved %zu\n", align, last_align, count[0], count[1], count[2], count[3], total, end);
}

int main() {
  const size_t counts[] = {0, 1, 2, 3, 5, 63, 64, 65, 257, 1000};
  const int elems[][4] = {{4, 4, 4, 8}, {4, 4, 4, 4}, {1, 4, 8, 1}, {8, 1, 1, 4}};
  const size_t aligns[][2] = {{4, 4}, {16, 16}, {256, 256}, {4, 16}};
  for (const auto& al : aligns)
    for (const auto& el : elems) {
      bool narrower = false;                                                    // no layout carves a type at less than its size
      for (int i = 0; i < 4; ++i) narrower = narrower || (size_t)el[i] > al[i == 3];
      if (narrower) continue;
      for (size_t a : counts) for (size_t b : counts) for (size_t c : counts) for (size_t d : {(size_t)0, (size_t)1, (size_t)7, (size_t)129}) {
        const size_t count[4] = {a, b, c, d};
        check(al[0], al[1], count, el);
      }
    }
  printf("Taker: %ld layouts checked at alignments 4, 16, 256 and 4 -> 16, %ld wrong\n", checked, bad);
  return bad ? 1 : 0;
}
