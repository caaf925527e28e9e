// tile_of (kgcn_amd/csrc/kgcn_common.h) against its definition b = tj (tj + 1) / 2 + ti, 0 <= ti <= tj, on the host:
//   every b of a 726-tile grid (the graph Gram of 46,340 graphs launches 725 tiles a side), and
//   the first and last block of every column, and both neighbours of its start, up to the largest grid labelprop.hip and
//   pairrank.hip launch (KGCN_LP_MAX_ROWS = 131,072 rows -> 2,048 tiles; KGCN_PAIRRANK_MAX_NODES = 65,536 -> 1,024 tiles).
// A host program of its own:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=undefined,address -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/tile_of_check.cpp -o /tmp/tile_of_check && /tmp/tile_of_check
#include "../../kgcn_amd/csrc/kgcn_common.h"

static long bad = 0, checked = 0;

static void check(long b, long tiles) {
  int ti = -1, tj = -1;
  kgcn::tile_of(b, ti, tj);
  ++checked;
  if (!(0 <= ti && ti <= tj && tj < tiles && (long)tj * (tj + 1) / 2 + ti == b)) {
    if (bad++ < 10) printf("tile_of(%ld) = (%d, %d) in a grid of %ld tiles\n", b, ti, tj, tiles);
  }
}

int main() {
  const long gram = 726;
  for (long b = 0; b < gram * (gram + 1) / 2; ++b) check(b, gram);
  const long lp = (KGCN_LP_MAX_ROWS + 63) / 64, pr = (KGCN_PAIRRANK_MAX_NODES + 63) / 64, tiles = lp > pr ? lp : pr;
  const long blocks = tiles * (tiles + 1) / 2;
  for (long tj = 0; tj < tiles; ++tj) {
    const long start = tj * (tj + 1) / 2;
    for (long b : {start - 1, start, start + 1, start + tj})          // last of the column before, first, second, last of this one
      if (b >= 0 && b < blocks) check(b, tiles);
  }
  printf("tile_of: %ld blocks checked (%ld-tile grid in full, column edges of the %ld-tile grid), %ld wrong\n", checked, gram, tiles, bad);
  return bad ? 1 : 0;
}
