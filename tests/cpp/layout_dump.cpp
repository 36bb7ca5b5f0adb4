// Prints every array size of csrc/gs_layout.h for a grid of curves, types and shapes, one line per array:
//   <fq> <ty> <shared> <N> <m> <n> <array> <bytes>
// followed by one line "<fq> <ty> shape <xg> <yg> <kx> <ky> <sx> <sy> <st>" per (fq, ty).  tests/test_layout.py
// compares the lines with the Python binding's table.  Includes nothing but the layout header.
#include <stdio.h>

#include "gs_layout.h"

int main() {
  const size_t fqs[] = {48, 32};
  const struct {
    size_t N;
    int m, n;
  } shapes[] = {{1, 1, 1}, {3, 2, 1}, {5, 1, 3}, {(size_t)1 << 20, 4096, 1024}};  // the last one overflows an int product
  for (size_t fq : fqs)
    for (int ty = 0; ty < 4; ty++) {
      for (int shared = 0; shared < 2; shared++)
        for (const auto& s : shapes) {
          if (!gs_layout::shape_fits(s.m, s.n)) return 1;
          const gs_layout::Layout L(fq, ty, s.N, s.m, s.n, shared != 0);
          for (int a = 0; a < gs_layout::NARRAYS; a++)
            printf("%zu %d %d %zu %d %d %s %zu\n", fq, ty, shared, s.N, s.m, s.n, gs_layout::kArrayName[a], L.bytes[a]);
        }
      const gs_layout::Layout L = gs_layout::Layout::stride(fq, ty, 1, 1);
      printf("%zu %d shape %d %d %d %d %zu %zu %zu\n", fq, ty, (int)L.xg, (int)L.yg, L.kx, L.ky, L.sx, L.sy, L.st);
    }
  // the shape limit: m * n <= 2^22 with m, n <= 4096
  if (!gs_layout::shape_fits(4096, 1024) || gs_layout::shape_fits(4096, 1025) || gs_layout::shape_fits(4097, 1)) return 2;
  return 0;
}
