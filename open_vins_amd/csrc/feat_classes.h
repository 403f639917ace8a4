// feat_classes.h — the length classes of an MSCKF batch (ovgpu_debug_option "feat_classes"): which per-feature kernel a track of m observations
// takes on its own, and the partition of a batch's slots (feature indices by descending track length) into at most four contiguous ranges, one
// per kernel.  Plain C++, no HIP: plan_feature_stage (api_state.inc) includes it, and tests/test_feat_classes_host.py compiles it into a
// stand-alone program under the address and undefined-behaviour sanitizers.
//
// The rule per track is the rule plan_feature_stage applies to the longest track of a batch (the tile budgets of the fused kernels):
//   the gate matrix of the one-pass kernels has 2 m + 4 rows in nta = ceil((2 m + 4) / 16) tile rows, nta (nta + 1) / 2 tiles of its upper triangle
//   k_feat_y<4, 9, 2>   4 x 9  = 36 tiles    m <= 62     code 1
//   k_feat_y<8, 17, 1>  8 x 17 = 136 tiles   m <= 126    code 2
//   k_feat_y_big        nt = ceil(2 m / 16) <= 29 tile rows   m <= 232    code 3
//   k_system_t          the rest                                           code 0
// Tracks of 0 or 1 observations take no kernel of their own (the kernels skip them by status): they go with the shortest class present.
// No class is merged into its neighbour for being small: DESIGN.md section 7 has the measurements that would have to justify such a rule.
#pragma once
#include <cstdint>

namespace ovg {
namespace featcls {

constexpr int FC_MAX = 4;                                // classes of a batch at most: one per code below
constexpr int FC_GENERAL = 0, FC_FEATY_4 = 1, FC_FEATY_8 = 2, FC_FEATY_BIG = 3; // the FeatKernel codes (api_context.inc) of the four
constexpr int FC_NT_BIG = 29;                            // tile rows the block-row kernel holds
constexpr int FC_NONE = -1;                              // a track of fewer than two observations

inline int tile_rows(int m) { return (2 * m + 15) / 16; }           // of the 2 m rows of a track
inline int gate_tile_rows(int m) { return (2 * m + 4 + 15) / 16; }  // of its gate matrix with the four augmented rows

// The kernel a batch whose longest track holds m observations is laid out for (every other eligibility term granted)
inline int kernel_of_length(int m) {
  if (m < 2) return FC_NONE;
  const int nta = gate_tile_rows(m), tiles = nta * (nta + 1) / 2;
  if (tiles <= 4 * 9) return FC_FEATY_4;
  if (tiles <= 8 * 17) return FC_FEATY_8;
  return tile_rows(m) <= FC_NT_BIG ? FC_FEATY_BIG : FC_GENERAL;
}

struct ClassRange {
  int kernel = FC_GENERAL;
  int begin = 0, end = 0; // slots begin .. end - 1 of the track order
  int m_max = 0;          // the longest track of the range: the one at slot `begin`
};
struct Partition {
  int n = 0; // classes, longest first; 0 for an empty batch
  ClassRange cls[FC_MAX];
};

// offsets[0 .. F]: the measurement offsets of the batch; order[0 .. F): its feature indices by descending track length.  A batch in which no
// track holds two observations is one class of the general kernel, as the single-kernel rule has it.
inline Partition partition(const int32_t *offsets, const int32_t *order, int F) {
  Partition pt;
  for (int slot = 0; slot < F; slot++) {
    const int f = order[slot], m = offsets[f + 1] - offsets[f];
    int k = kernel_of_length(m);
    if (k == FC_NONE) k = pt.n > 0 ? pt.cls[pt.n - 1].kernel : FC_GENERAL; // (descending lengths: every slot from here on is such a track)
    if (pt.n == 0 || pt.cls[pt.n - 1].kernel != k) {
      if (pt.n == FC_MAX) return Partition(); // (an order that is not descending: no partition)
      ClassRange &r = pt.cls[pt.n++];
      r.kernel = k, r.begin = slot, r.end = slot, r.m_max = m;
    }
    pt.cls[pt.n - 1].end = slot + 1;
  }
  return pt;
}

} // namespace featcls
} // namespace ovg
