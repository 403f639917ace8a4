// k_chol_wide.h — the Cholesky with carried columns beyond 256 columns, as TWO panels of chol::k_chol_fused (k_chol.h) around a Schur step.
//
// k_chol_fused holds the triangle of A in the registers of one workgroup: 16 tile rows, 256 columns.  Beyond that the factorisation used to be
// one launch of k_ekf_chol_step per 16 rows (k_ekf.h) — 17 to 32 dependent launches.  For 256 < D <= 512 the [D x LA] work matrix is split
//
//     [A | C] = [ A11  A12 | C1 ]        A11: 256 x 256
//               [  .   A22 | C2 ]        A22: D2 x D2,  D2 = D - 256
//
//   1. k_chol_fused on rows 0 .. 255 with everything right of A11 carried: Y rows 0 .. 255 = [U11 | W12 | Wc], final.
//   2. k_chol_schur   [A22 | C2] - W12^T [W12 | Wc]  ->  the COMPACT [D2 x LA2] matrix Ac (LA2 = LA - 256): one wavefront per 16 x 16 tile on or
//                     right of the diagonal tile, 64 v_mfma_f64_16x16x4_f64 each.  Both operands are row-contiguous pieces of Y's first 256 rows,
//                     streamed from L2 (k_initf_w's pattern; no LDS).  Thread 0 of the launch writes the GO word panel 2 is predicated on.
//   3. k_chol_fused on Ac -> Yc = [U22 | U22^-T (..)], compact as well: the kernel has no row stride, and it keeps its code object.
//   4. k_chol_place   Yc -> rows 256 .. D - 1 of Y from column 256 on; L = U^T for the caller that wants it.
//
// Four launches whatever D.  Ordering is by kernel boundaries only: neither kernel here waits for anything.  When panel 1 left a flag (pivot not
// positive / under tolerance: flags[0]; a follower's time-out: flags[2], which also raises flags[0]) the GO word is 0 and steps 2 - 4 do nothing:
// the flag words are what panel 1 left.  A time-out of panel 2 clears the GO word (it is that launch's predicate); k_chol_place then clears the
// CALLER's predicate, as k_chol_fused does itself when it is the caller's own launch.
#pragma once
#include "k_chol.h"

namespace ovg {
namespace chol {

constexpr int CW_D1 = 16 * CH_TMAX; // columns of the first panel

struct CholWideParams {
  int D, LA;                // the whole work matrix: CW_D1 < D <= 2 CW_D1
  const double *A;          // [D x LA] input
  double *Y;                // [D x LA] output; rows 0 .. CW_D1 - 1 are panel 1's
  double *Ac;               // [D2 x LA2] k_chol_schur's result, panel 2's input
  const double *Yc;         // [D2 x LA2] panel 2's result
  double *Lt;               // optional [D x D]: U^T with zeros above the diagonal (k_tf_lt's form)
  const int32_t *flags;     // [0] not positive definite, [2] a follower timed out
  int32_t *go;              // written by k_chol_schur, panel 2's predicate
  int32_t *pred;            // optional, the caller's: nothing happens when *pred == 0
  const int32_t *pred_not;  // optional, the caller's: nothing happens when *pred_not != 0
};

// Tile (ti, tj >= ti) of the compact matrix: rows 16 ti .. of A22's rows, columns 16 tj .. counted from column CW_D1 of the work matrix (the tiling
// runs straight through from A22 into the carried columns: a tile may hold both, both are the same row of Y to the B operand).
//   A operand, step u:  lane (g, cl) holds W12[4u + g][16 ti + cl] = Y[4u + g][CW_D1 + 16 ti + cl]
//   B operand, step u:  lane (g, cl) holds            Y[4u + g][CW_D1 + 16 tj + cl]
// Element (i, j) of the product depends on column i of A's tile and column j of B's only, so lanes beyond the matrix read a clamped address
// and their results are never stored: no masking of values.
__global__ void __launch_bounds__(256) k_chol_schur(CholWideParams p) {
  const int D = p.D, LA = p.LA, D2 = D - CW_D1, LA2 = LA - CW_D1;
  const bool go = !((p.pred && *p.pred == 0) || (p.pred_not && *p.pred_not != 0)) && p.flags[0] == 0 && p.flags[2] == 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) p.go[0] = go ? 1 : 0;
  if (!go) return;
  const int lane = threadIdx.x & 63, g = lane >> 4, cl = lane & 15;
  const int TR = (D2 + 15) >> 4, TC = (LA2 + 15) >> 4;
  int job = blockIdx.x * 4 + (threadIdx.x >> 6), ti = 0;
  while (ti < TR && job >= TC - ti) job -= TC - ti, ti++;
  if (ti >= TR) return;
  const int tj = ti + job;
  const int ca = min(CW_D1 + 16 * ti + cl, D - 1), cb = min(CW_D1 + 16 * tj + cl, LA - 1);
  d4 acc;
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = p.A[(size_t)min(CW_D1 + 16 * ti + g + 4 * q, D - 1) * LA + cb];
  const double *ya = p.Y + (size_t)g * LA + ca, *yb = p.Y + (size_t)g * LA + cb;
  // 32 rows of Y per trip: sixteen loads in flight per lane, then eight matrix instructions
#pragma unroll 1
  for (int k0 = 0; k0 < CW_D1; k0 += 32) {
    double a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] = ya[(size_t)(k0 + 4 * u) * LA], b[u] = yb[(size_t)(k0 + 4 * u) * LA];
#pragma unroll
    for (int u = 0; u < 8; u++) FEAT_MFMA(-a[u], b[u], acc);
  }
  const int col = 16 * tj + cl;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int row = 16 * ti + g + 4 * q;
    if (row < D2 && col < LA2) p.Ac[(size_t)row * LA2 + col] = acc[q];
  }
}

// One thread per element: first the D2 x LA2 elements of Yc (those panel 2 writes: from the row's diagonal TILE on), then, with Lt, the D x D
// elements of L = U^T, read from Y's first panel and from Yc.
__global__ void __launch_bounds__(256) k_chol_place(CholWideParams p) {
  const int D = p.D, LA = p.LA, D2 = D - CW_D1, LA2 = LA - CW_D1;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0 && p.pred && p.flags[2] != 0) p.pred[0] = 0; // whenever the time-out flag stands: panel 2's is the case that needs it (panel 1 cleared the word itself, a flag kept from earlier in a chain has the update dead already)
  if (p.go[0] == 0) return;
  const int64_t n_copy = (int64_t)D2 * LA2;
  if (e < n_copy) {
    const int r = (int)(e / LA2), c = (int)(e - (int64_t)r * LA2);
    if (c >= (r & ~15)) p.Y[(size_t)(CW_D1 + r) * LA + CW_D1 + c] = p.Yc[e];
    return;
  }
  e -= n_copy;
  if (!p.Lt || e >= (int64_t)D * D) return;
  const int s = (int)(e / D), c = (int)(e - (int64_t)s * D);
  double v = 0.0;
  if (c <= s) v = c < CW_D1 ? p.Y[(size_t)c * LA + s] : p.Yc[(size_t)(c - CW_D1) * LA2 + (s - CW_D1)];
  p.Lt[e] = v;
}

} // namespace chol
} // namespace ovg
