// ovgpu_slamy_big_tu.hip — the library's THIRD translation unit: the block-row shape of the fused SLAM per-feature kernel, slamy::k_slam_y_big, and
// its records kernel slamy::k_slam_rows_big (k_slam_y_big.h), both instantiations.
//
// Why a translation unit of its own: the register allocation of a kernel in ovgpu_api.hip moves with what else that compilation holds (k_chol_fused's
// spills went from 11 to 10 registers with these four kernels next to it), and the kernels behind "slam_fused_big" are to leave every existing
// kernel's code as it is: ovgpu_api.o's and ovgpu_featy_tu.o's device code is the parent's, `make resource-usage` shows its figures.
// ovgpu_api.hip declares these instantiations `extern template`; the non-template kernels of the headers are compiled there only (OVG_TU_FEATY).
#define OVG_TU_FEATY 1
#define OVG_TU_SLAMY_BIG 1
#include <hip/hip_runtime.h>

#include "k_slam_y_big.h"

namespace ovg {
namespace slamy {
template __global__ void k_slam_rows_big<false>(SysParams, SlamYBigStore);
template __global__ void k_slam_rows_big<true>(SysParams, SlamYBigStore);
template __global__ void k_slam_y_big<false>(SysParams, int, SlamYBigStore, double *);
template __global__ void k_slam_y_big<true>(SysParams, int, SlamYBigStore, double *);
} // namespace slamy
} // namespace ovg
