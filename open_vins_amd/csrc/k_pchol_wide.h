// k_pchol_wide.h — the diagonally pivoted Cholesky factor of the whitened Gram matrix for 25 .. 32 tile columns (mode A beyond 383 Jacobian columns,
// ovgpu_debug_option "mode_a_wide"), PANELLED in the manner of LAPACK's dpstrf.
//
// The contract is gram::k_gram_pchol's (k_gram.h) to the letter: step k eliminates the live column with the largest remaining diagonal entry, writes
// row k of R in the ORIGINAL column order with zeros in the columns eliminated before, never takes the carried column LD - 1 as a pivot and never masks
// it, stops at the first pivot not above tol x the first pivot, leaves the remaining rows of out [D x LD] zero and *n_dropped = D - rank.
//
// A 512 x 512 triangle does not fit the registers of one compute unit (k_gram_pchol holds twelve blocks of 32 columns), so the matrix stays in memory
// as the full symmetric square G [LG x LG] (k_gram_blk_reduce writes both triangles) and is worked on in place:
//
//   k_pchol_panel   ONE workgroup of 512 threads, PW_NB = 32 pivots per launch.  Thread j owns column j: its entries of the panel's rows in registers.
//                   Every wavefront keeps the whole running diagonal (dpstrf's `dots`: the starting diagonal minus the squares of the rows written so
//                   far — the very sequence of fused multiply-adds k_gram_pchol applies to its diagonal) and picks the pivot for itself, with
//                   k_gram_pchol's 32-bit key on the DPP network: all eight wavefronts hold the same numbers, so nobody is told.  Step i of the panel:
//                     row p of the trailing matrix, one contiguous read from L2      | the multipliers R[k0 + m][p], m < i: broadcast reads of the
//                     v = (row - sum_m R[k0 + m][p] R[k0 + m][j]) / sqrt(d), masked   | panel's rows in LDS
//                     -> registers, LDS (row i of the panel) and out
//                     ------------------------------------- workgroup barrier -------------------------------------
//                     every wavefront: its copy of the diagonal -= v^2 from the row in LDS, the pivot's column leaves the live set, next pivot
//                   ONE barrier per pivot: every row of the panel has an LDS row of its own, nothing is overwritten inside a launch.
//   k_pchol_schur   trailing matrix -= R_panel^T R_panel on v_mfma_f64_16x16x4_f64: one wavefront per 16 x 16 tile over the WHOLE square (both
//                   triangles, so that the panel kernel's row reads stay contiguous), eight matrix instructions per tile.  Eliminated columns hold zeros
//                   in R, so their rows and columns of G keep whatever they held: nobody reads them as live again (the mask on emit covers them).
//
// Why 32 pivots per launch and not 16: the launches are ordered by kernel boundaries only (as in k_chol_wide.h), and a boundary costs the stream a
// few microseconds — 32 of them at 511 columns against 64 —, while the correction grows by eight fused multiply-adds and eight broadcast LDS reads per
// step on average, a few hundred cycles next to the L2 round trip of the row.  The panel's rows take 128 KB of LDS (dynamic, through with_max_lds).
//
// Every launch of the largest panel count is enqueued up front.  The panel that stops — at a pivot not above the tolerance, or at row D — zeroes the
// rows it leaves unwritten, writes *n_dropped and raises ctl[PW_DONE]; every later launch reads that word first and returns.  Between launches the
// diagonal copy and the first pivot live in `dots` [LG + 1].  No kernel waits on another workgroup, every loop is bounded by D, LD or PW_NB, and every
// address is clamped to the matrix it reads.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "k_gram.h"

namespace ovg {
namespace gram {

constexpr int PW_NB = 32;    // pivots per launch of k_pchol_panel
constexpr int PW_LGMAX = 512; // columns of G at most: one thread each
constexpr int PW_NQ = PW_LGMAX / 64;
constexpr int PW_DONE = 1;    // ctl[0] is *n_dropped (the host reads it), ctl[PW_DONE] != 0: the factorisation has stopped
inline size_t pchol_wide_lds_bytes() { return (size_t)PW_NB * PW_LGMAX * sizeof(double); }
inline int pchol_wide_panels(int D) { return (D + PW_NB - 1) / PW_NB; }

struct PcholWideParams {
  int D, LD, LG;     // LD = D + 1 <= LG = 16 NT <= PW_LGMAX
  double *G;         // [LG x LG] the trailing matrix, in place
  double *out;       // [D x LD] R
  double *dots;      // [LG] the running diagonal (DEAD: eliminated or padding, CARRY: the carried column), [LG] the first pivot
  int32_t *ctl;      // [0] n_dropped, [PW_DONE]
  double tol;
  int k0;            // first pivot of this launch
};

__global__ void __launch_bounds__(PW_LGMAX) k_pchol_panel(PcholWideParams p) {
  extern __shared__ __attribute__((aligned(16))) double pw_rows[]; // [PW_NB][PW_LGMAX] the panel's rows of R (columns beyond LD: zero)
  constexpr double DEAD = -1.0e300, CARRY = -2.0e300;             // (both absorb every update: |R|^2 is far below their last bit)
  const int D = p.D, LD = p.LD, LG = p.LG, k0 = p.k0;
  const int tid = threadIdx.x, lane = tid & 63;
  if (k0 > 0 && p.ctl[PW_DONE] != 0) return; // (uniform: an earlier panel stopped)
  // the whole diagonal in every wavefront: column lane + 64 q
  double dg[PW_NQ];
  int colkey[PW_NQ];
#pragma unroll
  for (int q = 0; q < PW_NQ; q++) {
    const int j = lane + 64 * q;
    if (k0 == 0) dg[q] = j < D ? p.G[(size_t)j * LG + j] : (j < LD ? CARRY : DEAD);
    else dg[q] = j < LG ? p.dots[j] : DEAD;
    colkey[q] = 511 - j;
  }
  double dmax0 = k0 == 0 ? 0.0 : p.dots[LG], d = 0.0;
  int pv = -1;
  // the live column with the largest diagonal entry (ties: the lowest column): k_gram_pchol's 32-bit key — exponent and eleven mantissa bits with
  // the column in the low nine, as a signed integer (negative entries: negative keys) — reduced on the DPP network; the pivot's VALUE is read exactly
#define OVG_PW_NEXT_PIVOT(first)                                                                                                       \
  {                                                                                                                                    \
    int key = 0;                                                                                                                       \
    _Pragma("unroll") for (int q = 0; q < PW_NQ; q++) key = max(key, (__double2hiint(dg[q]) & ~0x1FF) | colkey[q]);                    \
    key = max(key, __builtin_amdgcn_update_dpp(0, key, 0x111, 0xF, 0xF, false));                                                       \
    key = max(key, __builtin_amdgcn_update_dpp(0, key, 0x112, 0xF, 0xF, false));                                                       \
    key = max(key, __builtin_amdgcn_update_dpp(0, key, 0x114, 0xF, 0xF, false));                                                       \
    key = max(key, __builtin_amdgcn_update_dpp(0, key, 0x118, 0xF, 0xF, false));                                                       \
    const int k01 = max(__builtin_amdgcn_readlane(key, 15), __builtin_amdgcn_readlane(key, 31));                                       \
    const int k23 = max(__builtin_amdgcn_readlane(key, 47), __builtin_amdgcn_readlane(key, 63));                                       \
    const int kmax = max(k01, k23);                                                                                                    \
    const int j = 511 - (kmax & 0x1FF), jq = j >> 6, jl = j & 63;                                                                      \
    double dsel = dg[0];                                                                                                               \
    _Pragma("unroll") for (int q = 1; q < PW_NQ; q++) dsel = jq == q ? dg[q] : dsel;                                                   \
    d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(dsel), jl), __builtin_amdgcn_readlane(__double2loint(dsel), jl));    \
    if (first) dmax0 = d;                                                                                                              \
    const bool go = kmax > 0 && d > p.tol * dmax0 && d > 0.0;                                                                          \
    pv = go ? j : -1;                                                                                                                  \
  }
  if (k0 == 0) OVG_PW_NEXT_PIVOT(true)
  else OVG_PW_NEXT_PIVOT(false)
  // this thread's column: alive while its entry of the diagonal is not DEAD (the carried column stays), its entries of the panel's rows
  const int mq = tid >> 6; // (wave-uniform: column tid is entry mq of lane `lane`)
  double mine[PW_NB];
#pragma unroll
  for (int i = 0; i < PW_NB; i++) mine[i] = 0.0;
  const int jc = min(tid, LG - 1); // clamped: the threads beyond LG read a value nobody uses
  int rank = -1;                  // >= 0: stopped in front of row `rank`
#pragma unroll
  for (int i = 0; i < PW_NB; i++) {
    const int k = k0 + i;
    if (k >= D) pv = -1;
    if (pv < 0) {
      rank = k;
      break;
    }
    const double g = p.G[(size_t)pv * LG + jc];
    double c = 0.0;
#pragma unroll
    for (int m = 0; m < i; m++) c = fma(pw_rows[m * PW_LGMAX + pv], mine[m], c);
    double my_dg = dg[0];
#pragma unroll
    for (int q = 1; q < PW_NQ; q++) my_dg = mq == q ? dg[q] : my_dg;
    double v = (g - c) * rsqrt_f64(d);
    v = (my_dg != DEAD && tid < LD) ? v : 0.0; // the columns eliminated before, and the padding
    mine[i] = v;
    pw_rows[i * PW_LGMAX + tid] = v;
    if (tid < LD) p.out[(size_t)k * LD + tid] = v;
    pchol_lds_barrier();
    const int pq = pv >> 6;
    const bool is_p = lane == (pv & 63);
#pragma unroll
    for (int q = 0; q < PW_NQ; q++) {
      const double r = pw_rows[i * PW_LGMAX + lane + 64 * q];
      dg[q] = fma(-r, r, dg[q]);
      dg[q] = (is_p && q == pq) ? DEAD : dg[q]; // the pivot's column leaves the live set: row k + 1 gets a zero there
    }
    OVG_PW_NEXT_PIVOT(false)
  }
#undef OVG_PW_NEXT_PIVOT
  if (rank < 0 && k0 + PW_NB >= D) rank = D; // the last panel ran through
  if (rank < 0) { // the next panel's start
    if (tid < 64) {
#pragma unroll
      for (int q = 0; q < PW_NQ; q++)
        if (lane + 64 * q < LG) p.dots[lane + 64 * q] = dg[q];
      if (lane == 0) p.dots[LG] = dmax0;
    }
    if (tid == 0 && k0 == 0) p.ctl[PW_DONE] = 0;
    return;
  }
  // stopped: zero rows behind the rank, the count, and the word every later launch reads first
  double *dst = p.out + (size_t)rank * LD;
  const int n_zero = (D - rank) * LD;
  for (int e = tid; e < n_zero; e += PW_LGMAX) dst[e] = 0.0;
  if (tid == 0) p.ctl[0] = D - rank, p.ctl[PW_DONE] = 1;
}

// G -= R[k0 .. k0 + PW_NB)^T R[k0 .. k0 + PW_NB): one wavefront per 16 x 16 tile of the whole square, four per workgroup.
//   A operand, step u:  lane (g, cl) holds R[k0 + 4 u + g][16 ti + cl]        B operand:  R[k0 + 4 u + g][16 tj + cl]
// Columns beyond LD - 1 read a clamped address: element (i, j) of the product depends on column i of A's tile and column j of B's only, and the
// rows and columns of G beyond LD are padding nobody reads as live.  The launch follows a panel whose PW_NB rows are all rows of the matrix
// (k0 + PW_NB < D), or does nothing.
__global__ void __launch_bounds__(256) k_pchol_schur(PcholWideParams p) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  if (p.ctl[PW_DONE] != 0) return;
  const int LD = p.LD, LG = p.LG, NT = LG >> 4, k0 = p.k0;
  if (k0 + PW_NB > p.D) return; // (never: the host enqueues no such launch)
  const int lane = threadIdx.x & 63, g = lane >> 4, cl = lane & 15;
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (job >= NT * NT) return;
  const int ti = job / NT, tj = job - ti * NT;
  const int ca = min(16 * ti + cl, LD - 1), cb = min(16 * tj + cl, LD - 1);
  const double *ra = p.out + (size_t)(k0 + g) * LD + ca, *rb = p.out + (size_t)(k0 + g) * LD + cb;
  double a[PW_NB / 4], b[PW_NB / 4];
#pragma unroll
  for (int u = 0; u < PW_NB / 4; u++) a[u] = ra[(size_t)(4 * u) * LD], b[u] = rb[(size_t)(4 * u) * LD];
  double *gt = p.G + (size_t)(16 * ti + g) * LG + 16 * tj + cl; // (16 NT = LG: every tile is inside the square)
  d4 acc;
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = gt[(size_t)(4 * q) * LG];
#pragma unroll
  for (int u = 0; u < PW_NB / 4; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[u], b[u], acc, 0, 0, 0);
#pragma unroll
  for (int q = 0; q < 4; q++) gt[(size_t)(4 * q) * LG] = acc[q];
}

// U_JJ^-1 of the diagonal tiles of U1 (the prior block's factor, rows of Y [D x LA]) -> uinv[J][256], row-major: what chol::k_chol_fused leaves for its
// followers, for a prior that was factored step-wise.  One wavefront per tile; lane c < 16 solves U v = e_c from the last row up (the tile's rows
// beyond D - 1 count as rows of the identity).  Nothing happens when the factorisation left its not-positive-definite flag.
__global__ void __launch_bounds__(64) k_uinv_tiles(int D, const double *__restrict__ Y, int LA, double *__restrict__ uinv, const int32_t *pred_not) {
  __shared__ double U[16 * 17];
  if (pred_not && *pred_not != 0) return;
  const int J = blockIdx.x, lane = threadIdx.x;
  if (16 * J >= D) return;
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15, r = 16 * J + i, cc = 16 * J + j;
    double x = i == j ? 1.0 : 0.0;
    if (r < D && cc < D && j >= i) x = Y[(size_t)r * LA + cc];
    U[i * 17 + j] = x;
  }
  __syncthreads();
  if (lane >= 16) return;
  double v[16];
#pragma unroll
  for (int i = 15; i >= 0; i--) {
    double s = i == lane ? 1.0 : 0.0;
#pragma unroll
    for (int j = i + 1; j < 16; j++) s = fma(-U[i * 17 + j], v[j], s);
    v[i] = s / U[i * 17 + i];
  }
#pragma unroll
  for (int i = 0; i < 16; i++) uinv[(size_t)J * 256 + i * 16 + lane] = i <= lane ? v[i] : 0.0;
}

} // namespace gram
} // namespace ovg
