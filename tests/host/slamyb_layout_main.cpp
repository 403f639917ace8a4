// The carve of k_slam_y_big (k_slam_y_big.h) on the host alone, printed for tests/test_slam_big_shapes_cpu.py.  No HIP runtime call is made; the
// header's kernels are compiled for the host side only.
//
//   consts <SLY_MMAX_B> <SLY_NT_B> <SLY_TPW_B> <SLY_NW> <FB_PF>
//   carve <m> <proj> <tile rows> <total bytes> <holds at 163840>
//   parts <proj> yb vl wpart rhs inst hq misc total        (at SLY_MMAX_B)
//   ws <tile rows> <doubles per workgroup>
#include <cstdio>

#define OVG_TU_FEATY 1 // (the templates and the layout functions: the non-template kernels belong to the library's main translation unit)
#include <hip/hip_runtime.h>

#include "k_slam_y_big.h"

int main() {
  using namespace ovg::slamy;
  std::printf("consts %d %d %d %d %d\n", SLY_MMAX_B, SLY_NT_B, SLY_TPW_B, SLY_NW, ovg::feat::FB_PF);
  const int ms[] = {1, 126, 127, 128, 129, 168, 169, 200, 208, 209, 224, 225, SLY_MMAX_B, SLY_MMAX_B + 1};
  for (int m : ms)
    for (int proj = 0; proj < 2; proj++) {
      const int nt = (2 * m + 15) >> 4;
      std::printf("carve %d %d %d %zu %d\n", m, proj, nt, slamyb_lds_layout(nt, proj != 0).total, (int)slamyb_holds(m, proj != 0, 163840));
    }
  for (int proj = 0; proj < 2; proj++) {
    const SlamYBigLds L = slamyb_lds_layout(SLY_NT_B, proj != 0);
    std::printf("parts %d %zu %zu %zu %zu %zu %zu %zu %zu\n", proj, L.yb, L.vl, L.wpart, L.rhs, L.inst, L.hq, L.misc, L.total);
  }
  std::printf("ws %d %zu\n", SLY_NT_B, ovg::feat::featyb_ws_doubles(SLY_NT_B));
  std::printf("rows_lds %zu\n", slamyb_rows_lds(SLY_MMAX_B));
  std::printf("slamyb layout ok\n");
  return 0;
}
