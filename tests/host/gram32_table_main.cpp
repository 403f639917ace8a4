// The host side of k_gram32.h alone: gram32_parts and gram32_tile_table for NTM = 1 .. 12 macro columns, printed for
// tests/test_fp32_gram_shapes_cpu.py.  No HIP runtime call is made; the header's kernels are compiled for the host side only.
//
//   consts <G32_NW> <G32_MAXT> <G32_SR> <G32_ROWS_WG>
//   ntm <NTM> parts <P>
//   <P * G32_NW lines>  part wave  code code ... (G32_MAXT codes: (J << 8) | I, or -1)
#include <cstdio>
#include <vector>

#include "k_gram32.h"

int main() {
  using namespace ovg::gram32;
  std::printf("consts %d %d %d %d\n", G32_NW, G32_MAXT, G32_SR, G32_ROWS_WG);
  for (int ntm = 1; ntm <= 12; ntm++) {
    const int P = gram32_parts(ntm);
    std::vector<int32_t> tab((size_t)P * G32_NW * G32_MAXT, 12345);
    gram32_tile_table(ntm, P, tab.data());
    std::printf("ntm %d parts %d\n", ntm, P);
    for (int part = 0; part < P; part++)
      for (int w = 0; w < G32_NW; w++) {
        std::printf("%d %d ", part, w);
        for (int s = 0; s < G32_MAXT; s++) std::printf(" %d", (int)tab[((size_t)part * G32_NW + w) * G32_MAXT + s]);
        std::printf("\n");
      }
  }
  std::printf("gram32 table ok\n");
  return 0;
}
