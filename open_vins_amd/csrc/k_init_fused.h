// k_init_fused.h — one candidate of UpdaterSLAM::delayed_init (UpdaterSLAM.cpp:147-239: StateHelper::initialize = initialize_invertible
// followed by EKFUpdate, StateHelper.cpp:393-577) as a chain of FIVE launches without a memset (ovgpu_slam_delayed_init_fused):
//
//   k_system_t (init mode, k_system.h)   A1 = Q1^T [H_x | res] with R1 (init_out), A2 = Q2^T [H_x | res] (the stack's 2m - 3 rows), the gate flag
//   k_initf_w                            W = [G ; A2_x] P(cols, :),  G = R1^-1 A1           (3 + 2m - 3) x N, on the matrix cores
//   k_initf_s                            [S | -W2(:, cols) G^T | res2],  S = W2(:, cols) A2_x^T + sigma^2 I;  P_LL;  the Cholesky's step words
//   k_chol_fused (k_chol.h)              S = U^T U carried through [W2 | new columns | res2]  ->  Z, y
//   k_initf_tail                         P <- P_aug - Z^T Z, dx = Z^T y, box-plus, landmarks, the new landmark, counters, pose tables
//
// The algebra.  initialize_invertible appends the columns P(:, new) = -P(:, cols) G^T and P_LL = G P_DD G^T + sigma^2 R1^-1 R1^-T; the
// update that follows has H_f = 0 on the new variable, so its P_aug H^T is [W2^T ; -G W2(:, cols)^T]: BOTH need only G P(cols, :) and
// A2_x P(cols, :), i.e. ONE product of (2m) x D by D x N, and the appended columns need not be in memory before the update — the tail
// reads them from T = G P(cols, :) while it writes P_aug - Z^T Z.  The chain of single launches (k_init_invertible, k_ekf_mt, k_ekf_s, two
// clears, k_chol_fused, k_ekf_dx, k_ekf_pupdate, k_boxplus, k_build_tables, k_landmark_update) formed G P(cols, :) serially over D on one
// workgroup and the second product in a kernel of its own.
//
// Per-feature noise (ovgpu_set_feature_options): k_system_t scales A1, R1 and A2 by sigma / sigma_f, so sigma^2 below is the context's one
// value and sigma^2 R1^-1 R1^-T is sigma_f^2 (R1 / scale)^-1 (..)^-T.
//
// Everything is predicated on the gate flag ctr[2]: a rejected candidate writes nothing.  No workgroup waits for another one in the three kernels
// of this file: the tail's counters are advanced by the workgroup that finishes LAST (an atomic count of arrivals, reset by that workgroup).
// The only waits of the step are k_chol_fused's bounded ones.
//
// Bound: 2m - 3 + 3 <= 128 rows of W (eight 16-row tiles), m <= INITF_M_MAX = 64; a longer track takes the chain of single launches.
//
// ovgpu_debug_option "delayed_init_fused_long" = 1 moves the bound to INITF_M_MAX_LONG = 232, where the other fused per-feature kernels stop.  Nothing
// in the three kernels of this file is tied to 128 rows (a wavefront per 16 x 16 tile over global memory); what changes is around them: k_init_rows'
// carve goes beyond the 64 KB default (656 bytes per measurement + 512 at 72-double records, 152 704 bytes at 232: launched through with_max_lds),
// and r = 2m - 3 > 256 (m >= 130) is factored by the two panels of k_chol_wide.h, whose step words the host clears (p.prog = nullptr: k_initf_s leaves
// them alone).  k_chol_place puts the second panel's rows, the carried residual among them, where the tails read them.
//
// Level 2 of ovgpu_debug_option "delayed_init_fused": the gate is taken from the chain's own factor.  k_chol_fused carries res2 through
// S = U^T U to y = U^-T res2, and |y|^2 = res2^T (A2_x P_DD A2_x^T + sigma^2 I)^-1 res2 is the statistic StateHelper::initialize gates on
// (StateHelper.cpp:466; rows scaled by sigma / sigma_f scale S by its square and res2 by itself: the statistic does not see the scale).  So
//
//   k_init_rows                          A1, R1, A2 and the threshold as k_system_t's init mode leaves them, WITHOUT its gate: nothing of P is read
//   k_initf_w, k_initf_s, k_chol_fused   as above, predicated on ctr[2] = "the candidate was triangulated"
//   k_initf_tail_gate                    every workgroup forms chi2 = |y|^2 in one fixed order and decides alone; a rejected candidate writes
//                                        chi2 and its status (the last workgroup) and nothing else
#pragma once
#include "k_ekf.h"
#include "k_slam.h"
#include "k_system.h"
#include "k_triangulate.h"

namespace ovg {

constexpr int INITF_M_MAX = 64;
constexpr int INITF_M_MAX_LONG = 232; // "delayed_init_fused_long": r = 2m - 3 <= 461, two Cholesky panels from m = 130 on
constexpr int INIT_ROWS_CPW = 64;     // k_init_rows on a track beyond INITF_M_MAX: columns of phase (d) per workgroup (one wavefront's worth)

// k_init_rows' LDS carve in bytes for a launch whose candidate holds at most m_max measurements (host and device agree on this): the Jacobian
// records at the context's row stride, their bookkeeping, V of the three reflectors, the representation scratch.  64 measurements of 72 doubles:
// 42496 bytes.
struct InitRowsLds {
  size_t minfo, rows, V, hq, total;
};
__host__ __device__ constexpr InitRowsLds init_rows_lds_layout(int m_max, int row_stride) {
  InitRowsLds L{};
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15) & ~(size_t)15;
    return at;
  };
  L.minfo = take((size_t)m_max * 8 * sizeof(int));
  L.rows = take((size_t)m_max * row_stride * sizeof(double));
  L.V = take((size_t)2 * m_max * 3 * sizeof(double));
  L.hq = take(64 * sizeof(double)); // [0..2] tau, [3..8] T, [12..20] dpfg_dlambda, [21..38] H_anc, [39..56] H_calib, [58..60] diag(R1)
  L.total = o;
  return L;
}
static_assert(init_rows_lds_layout(INITF_M_MAX, 72).total == 42496, "the carve of the 64-measurement bound is what it was");
static_assert(init_rows_lds_layout(INITF_M_MAX_LONG, 72).total == 152704 && init_rows_lds_layout(INITF_M_MAX_LONG, 72).total <= 160 * 1024,
              "k_init_rows' carve at the long bound and 72-double records has to fit a compute unit's 160 KB of LDS");

// The system of ONE candidate (p.f_begin) of the delayed initialisation without the gate: phases (a0), (a), (b) and the unwhitened (d) of
// k_system_t for p.init = 1 (an MSCKF-style system: all three columns of H_f are projected), through the same device functions.  One workgroup;
// for a track beyond INITF_M_MAX a workgroup per INIT_ROWS_CPW columns of phase (d), each with the whole carve (see the kernel's head).
//   init_out[0 .. 3 LD) = oscale Q1^T [H_x | res],  init_out[3 LD .. + 9) = oscale R1,  the candidate's rows of Hbig = oscale Q2^T [H_x | res],
//   chi2_thresh[f],  init_flag[0] = the candidate arrived OVGPU_FEAT_USED.
// Neither chi2[f] nor status[f] is written, neither P nor the gate's workspaces are read.  p.m_max sizes the carve (the host passes the fused
// step's bound when the batch's longest track is beyond it).
__global__ void __launch_bounds__(SYS_NT) k_init_rows(SysParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int D = p.D, LD = p.LD, RS = p.row_stride;
  const InitRowsLds lo = init_rows_lds_layout(p.m_max, RS);
  int *minfo = reinterpret_cast<int *>(smem + lo.minfo);
  double *rows = reinterpret_cast<double *>(smem + lo.rows);
  double *V = reinterpret_cast<double *>(smem + lo.V);
  double *hq = reinterpret_cast<double *>(smem + lo.hq);

  const int f = p.f_begin;
  const int m0 = p.meas_offsets[f];
  const int m = p.meas_offsets[f + 1] - m0;
  const int64_t orow0 = p.row_off[f];
  const int n_out = (int)(p.row_off[f + 1] - orow0); // 2m - 3
  // The columns of phase (d) are dealt to the launch's workgroups in whole blocks of INIT_ROWS_CPW; every workgroup repeats (a0), (a) and (b),
  // which read nothing of P and write LDS only, and workgroup 0 alone writes what is not a column's.  One workgroup (a track of 64 measurements
  // at most): all columns, the launch as it was.  A column is one thread's, summed in one order whichever workgroup holds it: the same bits.
  const bool first_wg = blockIdx.x == 0;
  const int c_per_wg = ((LD + (int)gridDim.x - 1) / (int)gridDim.x + INIT_ROWS_CPW - 1) / INIT_ROWS_CPW * INIT_ROWS_CPW;
  const int c_begin = blockIdx.x * c_per_wg, c_end = min(LD, c_begin + c_per_wg);
  if (p.status[f] != OVGPU_FEAT_USED || m < 2 || m > p.m_max) { // failed before the gate (or a track the carve does not hold: the host never sends one)
    if (!first_wg) return;
    for (int64_t e = tid; e < (int64_t)n_out * LD; e += SYS_NT) p.Hbig[orow0 * LD + e] = 0.0;
    if (tid == 0) p.init_flag[0] = 0;
    return;
  }
  const int n = 2 * m;
  constexpr int nproj = 3;

  // (a0) representation Jacobian — UpdaterHelper.cpp:32-190
  const int rep_f = p.opt.feat_rep;
  const bool relative = rep_is_relative(rep_f);
  const double mult_f = p.feat_chi2mult ? p.feat_chi2mult[f] : p.opt.chi2_multipler;
  const double oscale = p.feat_sigma ? sqrt(p.opt.sigma_pix_sq) / p.feat_sigma[f] : 1.0; // (k_system_t: the stack keeps ONE isotropic noise level)
  V3 p_FinG = load_v3(p.p_FinG + 3 * f);
  int anchor_cam = -1, anchor_clone = -1;
  if (relative) { // the anchor of the triangulation
    const int ac = p.meas_cc[p.anchor_meas[f]];
    anchor_cam = ac >> 10, anchor_clone = ac & 1023;
    const V3 p_FinA = load_v3(p.p_FinA + 3 * f);
    const M3 R_ItoC = load_m3(p.tab_cam + 12 * anchor_cam);
    const V3 p_IinC = load_v3(p.tab_cam + 12 * anchor_cam + 9);
    const M3 R_GtoI = load_m3(p.tab_clone + 24 * anchor_clone);
    const V3 p_IinG = load_v3(p.tab_clone + 24 * anchor_clone + 9);
    p_FinG = mulT(R_GtoI, mulT(R_ItoC, p_FinA - p_IinC)) + p_IinG; // UpdaterHelper.cpp:274
  }
  const V3 p_FinG_fej = p_FinG; // fej == value for a feature that is not in the state yet (UpdaterMSCKF.cpp:186-194, UpdaterHelper.cpp:279-283)
  if (tid == 0) {
    double *dl = hq + 12;
    if (rep_f == OVGPU_REP_GLOBAL_3D) {
      dl[0] = 1, dl[1] = 0, dl[2] = 0, dl[3] = 0, dl[4] = 1, dl[5] = 0, dl[6] = 0, dl[7] = 0, dl[8] = 1;
    } else if (rep_f == OVGPU_REP_GLOBAL_FULL_INVERSE_DEPTH) {
      inv_depth_jac(p_FinG, dl); // UpdaterHelper.cpp:46
    } else {
      anchored_rep_jacobian(rep_f, p.opt.do_fej, p.tab_cam + 12 * anchor_cam, p.tab_clone + 24 * anchor_clone, load_v3(p.p_FinA + 3 * f), dl, hq + 21, hq + 39);
    }
    // StateHelper::initialize gates against the quantile of the res.rows() it was handed: 2m, or 2m - 2 when the bearing was projected out
    // before (StateHelper.cpp:466, UpdaterSLAM.cpp:181-196)
    if (first_wg) {
      p.chi2_thresh[f] = mult_f * p.chi2_table[min(n - p.init_dof_less, p.chi2_table_len - 1)];
      p.init_flag[0] = 1;
    }
  }
  __syncthreads();

  // (a) per-measurement sparse Jacobian rows — UpdaterHelper.cpp:314-421
  for (int i = tid; i < m; i += SYS_NT) sys_measurement_rows(p, m0 + i, p_FinG, p_FinG_fej, relative, hq, minfo + 8 * i, rows + (size_t)i * RS);
  __syncthreads();

  // (b) Householder QR of H_f (2m x 3) -> V, tau, T
  if (tid < 64) sys_hf_householder(rows, RS, V, hq, n, nproj, tid);
  __syncthreads();

  // (d) thread per column: rows 0..2 of Q^T [H_x | res] -> init_out, rows 3..n-1 -> Hbig (k_system_t's unwhitened stack, p.init)
  const double T00 = hq[3], T01 = hq[4], T02 = hq[5], T11 = hq[6], T12 = hq[7], T22 = hq[8];
  for (int c = c_begin + tid; c < c_end; c += SYS_NT) {
    int kind = COL_RESIDUAL, var = 0, sub = 0;
    if (c < D) kind = p.col_kind[c], var = p.col_var[c], sub = p.col_sub[c];
    const bool anc_hit_c = (kind == COL_CLONE && var == anchor_clone && relative);
    const bool anc_hit_p = (kind == COL_CALIB_POSE && var == anchor_cam && relative && p.opt.do_calib_pose);
    const int kclone = (kind == COL_CLONE) ? var : -1000;
    const int kcam = (kind == COL_CALIB_POSE || kind == COL_CALIB_INTR) ? var : -1000; // such a column exists only for a calibrated camera
    const bool whole = kind == COL_RESIDUAL; // (a landmark's column: no candidate touches a resident landmark)
    const int off0 = kind == COL_RESIDUAL ? RO_RES
                                          : (kind == COL_CLONE ? RO_CLONE + sub
                                                               : (kind == COL_CALIB_POSE ? RO_CPOSE + sub : (kind == COL_CALIB_INTR ? RO_CINTR + sub : RO_HF + sub)));
    const int astr = kind == COL_RESIDUAL ? 1 : (kind == COL_CALIB_INTR ? 8 : (kind == COL_LANDMARK ? 3 : 6));
    auto hval = [&](int i, int a) -> double {
      const int2 key = *reinterpret_cast<const int2 *>(minfo + 8 * i); // (camera, clone)
      const double *rd = rows + (size_t)i * RS;
      const double hv = rd[off0 + astr * a];
      double h = (whole || key.y == kclone || key.x == kcam) ? hv : 0.0;
      if (anc_hit_c) h += rd[RO_ANC + 6 * a + sub];
      if (anc_hit_p) h += rd[RO_ACAL + 6 * a + sub];
      return h;
    };
    double y0 = 0, y1 = 0, y2 = 0; // y = V^T h
#pragma unroll 4
    for (int i = 0; i < m; i++) {
      const double h0 = hval(i, 0), h1 = hval(i, 1);
      const double *v = V + (size_t)6 * i;
      y0 = fma(v[0], h0, y0), y1 = fma(v[1], h0, y1), y2 = fma(v[2], h0, y2);
      y0 = fma(v[3], h1, y0), y1 = fma(v[4], h1, y1), y2 = fma(v[5], h1, y2);
    }
    const double z0 = T00 * y0, z1 = T01 * y0 + T11 * y1, z2 = T02 * y0 + T12 * y1 + T22 * y2; // z = T^T y
    double *out = p.Hbig + orow0 * LD + c;
#pragma unroll 4
    for (int r = 0; r < n; r++) { // StateHelper.cpp:445-448: the first three rows determine the new variable, the others are gated and update
      const double h = hval(r >> 1, r & 1);
      const double *v = V + (size_t)3 * r;
      const double q = oscale * (h - (v[0] * z0 + v[1] * z1 + v[2] * z2));
      if (r < nproj) p.init_out[(size_t)r * LD + c] = q;
      else out[(size_t)(r - nproj) * LD] = q;
    }
  }
  if (first_wg && tid < 9) { // H_finit = R1 (3 x 3 upper triangular): Q^T H_f, diagonal = beta
    const int i = tid / 3, j = tid % 3;
    p.init_out[(size_t)3 * LD + tid] = oscale * (j < i ? 0.0 : (j == i ? hq[58 + i] : rows[(size_t)(i >> 1) * RS + RO_HF + 3 * (i & 1) + j]));
  }
}

// What the gated tail (level 2) reads and writes beyond InitFusedParams: the batch's gate arrays
struct InitGateParams {
  const double *chi2_thresh; // [F] written by k_init_rows
  double *chi2;              // [F]
  int32_t *status;           // [F]
};

struct InitFusedParams {
  int N;                    // leading dimension of P (the padded capacity) = carried covariance columns
  int D, LD;                // Jacobian columns, row stride of the system rows (residual in column D)
  int r, LA;                // 2m - 3 projected rows; LA = r + N + 1 columns of the factorisation's work matrix
  int rep, f, sz;           // representation, feature, dof of the new landmark (3; 1: only the third row of the 3-row system initialises it)
  const int32_t *col_cov;   // [D]
  const double *init_out;   // [3 LD + 9]: A1, R1
  const double *stack;      // [r x LD]: A2
  double *P;                // [N x N]
  double *A;                // [r x LA] = [S | W2 (new columns at id ..) | res2]
  const double *Y;          // [r x LA] the factorisation's result [U | Z | y]
  double *T;                // [3 x N] G P(cols, :)
  double *PLL;              // [9] G P_DD G^T + sigma^2 R1^-1 R1^-T
  double sigma2;
  int32_t *ctr;             // [0] covariance dimension, [1] landmark count, [2] this candidate passed the gate (level 2: was triangulated), [4] arrivals of the tail's workgroups
  int32_t *prog;            // [16] k_chol_fused's step words (cleared by k_initf_s); null: r > 256, both panels' words are cleared by the host
  double *dx;               // [N] row f of dx_seq
  int32_t *flags;           // [1] = 1: a negative diagonal of P after the update
  // the tail
  int C, K;
  const int32_t *clone_cov, *calib_cov, *intr_cov;
  double *clone_qp, *calib_qp, *intr;
  const double *clone_fej;
  double *tab_clone, *tab_cam, *tab_cc;
  const double *p_FinG, *p_FinA;
  const uint16_t *meas_cc;
  const int32_t *anchor_meas;
  LandmarkStore lm;
  int32_t *feat_slot;
};

// H_L^-1 of the upper-triangular 3 x 3 R1 (StateHelper.cpp:548) and a column of G = H_L^-1 [H_R | res]
struct InitHLinv {
  double i00, i01, i02, i11, i12, i22;
};
__device__ __forceinline__ InitHLinv initf_hlinv(const double *R1) {
  const double u00 = R1[0], u01 = R1[1], u02 = R1[2], u11 = R1[4], u12 = R1[5], u22 = R1[8];
  InitHLinv h;
  h.i00 = 1.0 / u00, h.i11 = 1.0 / u11, h.i22 = 1.0 / u22;
  h.i01 = -u01 * h.i00 * h.i11, h.i12 = -u12 * h.i11 * h.i22, h.i02 = (u01 * u12 - u02 * u11) * h.i00 * h.i11 * h.i22;
  return h;
}
__device__ __forceinline__ double initf_g(const InitHLinv &h, const double *top, int LD, int j, int c) {
  const double a = top[c], b = top[LD + c], d = top[2 * LD + c];
  return j == 0 ? h.i00 * a + h.i01 * b + h.i02 * d : (j == 1 ? h.i11 * b + h.i12 * d : h.i22 * d);
}

// W = [G ; A2_x] P(cols, :): one wavefront per 16 x 16 tile, W's rows tiled by 16 (G's three rows and A2's in one operand), the N columns
// across workgroups, P's rows gathered by col_cov.  Rows 0..2 -> T, rows 3.. -> the carried columns of A.
__global__ void __launch_bounds__(256) k_initf_w(InitFusedParams p) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int tn = (p.N + 15) / 16, tm = (p.r + 3 + 15) / 16;
  if (tile >= tn * tm || p.ctr[2] == 0) return;
  const int r0 = (tile / tn) * 16, c0 = (tile % tn) * 16;
  const InitHLinv h = initf_hlinv(p.init_out + (size_t)3 * p.LD);
  auto fa = [&](int i, int k) {
    const int row = r0 + i;
    if (row < 3) return initf_g(h, p.init_out, p.LD, row, k);
    return row < p.r + 3 ? p.stack[(size_t)(row - 3) * p.LD + k] : 0.0;
  };
  auto fb = [&](int k, int j) { const int c = c0 + j; return (c < p.N) ? p.P[(size_t)p.col_cov[k] * p.N + c] : 0.0; };
  const double4_t acc = mfma_tile(fa, fb, p.D, lane);
  const int col = c0 + (lane & 15);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int row = r0 + (lane >> 4) + 4 * q;
    if (col >= p.N || row >= p.r + 3) continue;
    if (row < 3) p.T[(size_t)row * p.N + col] = acc[q];
    else p.A[(size_t)(row - 3) * p.LA + p.r + col] = acc[q];
  }
}

// [S | new columns] = W2(:, cols) [A2_x ; G]^T (+ sigma^2 I on S): one wavefront per tile, the three rows of G ride behind A2's in the second
// operand.  The LAST workgroup: P_LL (wavefront 0), the residual column, the factorisation's step words.
__global__ void __launch_bounds__(256) k_initf_s(InitFusedParams p) {
  if (p.ctr[2] == 0) return;
  const int lane = threadIdx.x & 63;
  const int r = p.r, LD = p.LD, LA = p.LA, N = p.N, D = p.D;
  const InitHLinv h = initf_hlinv(p.init_out + (size_t)3 * LD);
  const int id = p.ctr[0], j0 = 3 - p.sz;
  if (blockIdx.x + 1 == gridDim.x) {
    for (int row = threadIdx.x; row < r; row += 256) p.A[(size_t)row * LA + r + N] = p.stack[(size_t)row * LD + D];
    if (p.prog && threadIdx.x < 16) p.prog[threadIdx.x] = 0; // (null: the two-panel factorisation, whose words the host clears)
    if (threadIdx.x < 64) {
      double s[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int c = lane; c < D; c += 64) {
        const int cc = p.col_cov[c];
        double g[3], t[3];
#pragma unroll
        for (int j = 0; j < 3; j++) g[j] = initf_g(h, p.init_out, LD, j, c), t[j] = p.T[(size_t)j * N + cc];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
          for (int k = 0; k < 3; k++) s[j][k] = fma(t[j], g[k], s[j][k]);
      }
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++)
          for (int off = 32; off > 0; off >>= 1) s[j][k] += __shfl_xor(s[j][k], off, 64);
      if (lane == 0) {
        const double inv[3][3] = {{h.i00, h.i01, h.i02}, {0.0, h.i11, h.i12}, {0.0, 0.0, h.i22}};
        for (int j = 0; j < 3; j++)
          for (int k = 0; k < 3; k++) {
            double w = 0.0;
            for (int q = 0; q < 3; q++) w = fma(inv[j][q], inv[k][q], w); // sigma^2 H_L^-1 H_L^-T (:549, R = sigma^2 I)
            p.PLL[3 * j + k] = fma(p.sigma2, w, s[j][k]);
          }
      }
    }
    return;
  }
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int tm = (r + 15) / 16, tc = (r + 3 + 15) / 16;
  if (tile >= tm * tc) return;
  const int r0 = (tile / tc) * 16, c0 = (tile % tc) * 16;
  auto fa = [&](int i, int k) { const int row = r0 + i; return (row < r) ? p.A[(size_t)row * LA + r + p.col_cov[k]] : 0.0; };
  auto fb = [&](int k, int j) {
    const int c = c0 + j;
    if (c < r) return p.stack[(size_t)c * LD + k];
    return c < r + 3 ? initf_g(h, p.init_out, LD, c - r, k) : 0.0;
  };
  const double4_t acc = mfma_tile(fa, fb, D, lane);
  const int col = c0 + (lane & 15);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int row = r0 + (lane >> 4) + 4 * q;
    if (row >= r) continue;
    if (col < r) p.A[(size_t)row * LA + col] = acc[q] + (row == col ? p.sigma2 : 0.0);
    else if (col >= r + j0 && col < r + 3) p.A[(size_t)row * LA + r + id + (col - r - j0)] = -acc[q]; // (id + sz <= N: the capacity counts every candidate)
  }
}

// The tail.  Workgroups 0 .. n - 2: one wavefront per 16 x 16 tile of P <- P_aug - Z^T Z over the current dimension id + sz, the appended rows /
// columns taken from T and P_LL (symmetric by construction: Z^T Z is, -T is mirrored, P_LL is averaged with its transpose).  The last workgroup:
// dx = Z^T y, Landmark::update of the resident landmarks, the new landmark, box-plus of clones / calibration / intrinsics, the pose tables.  The
// workgroup that arrives last advances the dimension and the landmark count.
//
// GATE (level 2): ctr[2] only says that the candidate was triangulated, and the decision is taken here.  Every workgroup sums y_k^2 over the r rows
// of the factorisation's carried residual column in ONE order — wavefront 0: lane-strided partial sums, a fixed butterfly, broadcast through LDS —
// so all of them hold the same bits and take the same branch without a word between them.  reject = chi2 > thr (k_system_t's comparison).  A
// rejected candidate: the last workgroup writes chi2 and the status, nobody writes anything else, the arrivals are counted and reset, the
// dimension and the landmark count stay.
template <bool GATE> __device__ __forceinline__ void initf_tail_body(const InitFusedParams &p, const InitGateParams &g) {
  if (p.ctr[2] == 0) return; // (every workgroup reads the same word: all of them leave, nobody counts)
  const int lane = threadIdx.x & 63, tid = threadIdx.x;
  const int r = p.r, LA = p.LA, N = p.N;
  const int id = p.ctr[0], slot = p.ctr[1], j0 = 3 - p.sz, n1 = id + p.sz;
  const double *Z = p.Y + r;
  bool reject = false;
  if constexpr (GATE) {
    __shared__ double chi2_s;
    if (tid < 64) {
      double s = 0.0;
      for (int k = lane; k < r; k += 64) {
        const double yk = p.Y[(size_t)k * LA + r + N];
        s = fma(yk, yk, s);
      }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) chi2_s = s;
    }
    __syncthreads();
    const double chi2 = chi2_s;
    reject = chi2 > g.chi2_thresh[p.f];
    if (blockIdx.x + 1 == gridDim.x && tid == 0) {
      g.chi2[p.f] = chi2;
      if (reject) g.status[p.f] = OVGPU_FEAT_CHI2_REJECTED;
    }
  }
  if (reject) {
    // (nothing of the state is written)
  } else if (blockIdx.x + 1 < gridDim.x) {
    const int tile = blockIdx.x * 4 + (tid >> 6);
    const int tn = (N + 15) / 16;
    const int r0 = (tile / tn) * 16, c0 = (tile % tn) * 16;
    if (tile < tn * tn && r0 < n1 && c0 < n1) {
      auto fa = [&](int i, int k) { const int row = r0 + i; return (row < n1) ? Z[(size_t)k * LA + row] : 0.0; };
      auto fb = [&](int k, int j) { const int c = c0 + j; return (c < n1) ? Z[(size_t)k * LA + c] : 0.0; };
      const double4_t acc = mfma_tile(fa, fb, r, lane);
      const int col = c0 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = r0 + (lane >> 4) + 4 * q;
        if (row >= n1 || col >= n1) continue;
        double base;
        if (row < id && col < id) base = p.P[(size_t)row * N + col];
        else if (row >= id && col >= id) base = 0.5 * (p.PLL[3 * (row - id + j0) + col - id + j0] + p.PLL[3 * (col - id + j0) + row - id + j0]); // :558
        else if (row >= id) base = -p.T[(size_t)(row - id + j0) * N + col]; // :556-557
        else base = -p.T[(size_t)(col - id + j0) * N + row];
        const double v = base - acc[q];
        p.P[(size_t)row * N + col] = v;
        if (row == col && v < 0.0) p.flags[1] = 1; // StateHelper.cpp:172-182
      }
    }
  } else {
    const double *y = p.Y + r + N;
    for (int i = tid; i < N; i += 256) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      if (i < n1) {
        int k = 0;
        for (; k + 4 <= r; k += 4) {
          s0 = fma(Z[(size_t)k * LA + i], y[(size_t)k * LA], s0);
          s1 = fma(Z[(size_t)(k + 1) * LA + i], y[(size_t)(k + 1) * LA], s1);
          s2 = fma(Z[(size_t)(k + 2) * LA + i], y[(size_t)(k + 2) * LA], s2);
          s3 = fma(Z[(size_t)(k + 3) * LA + i], y[(size_t)(k + 3) * LA], s3);
        }
        for (; k < r; k++) s0 = fma(Z[(size_t)k * LA + i], y[(size_t)k * LA], s0);
      }
      p.dx[i] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads(); // dx complete (this workgroup wrote all of it)
    for (int t = tid; t < 3 * slot; t += 256) { // Landmark::update of the resident landmarks, through P alone (k_landmark_update's rule)
      const int l = t / 3, k = t % 3, l0 = 3 - lm_rep_dof(p.lm.rep[l]);
      if (k >= l0) p.lm.value[3 * l + k] += p.dx[p.lm.cov[l] + k - l0];
    }
    if (tid < 3) { // the new landmark: UpdaterSLAM.cpp:213-221, new_variable->update(H_L^-1 res) (:569), then the update's own correction
      const bool relative = p.rep >= OVGPU_REP_ANCHORED_3D;
      const double *x = (relative ? p.p_FinA : p.p_FinG) + 3 * p.f;
      double v[3];
      lm_from_xyz(p.rep, V3{x[0], x[1], x[2]}, v);
      const int j = tid;
      const InitHLinv h = initf_hlinv(p.init_out + (size_t)3 * p.LD);
      p.lm.fej[3 * slot + j] = v[j];
      p.lm.value[3 * slot + j] = j >= j0 ? (v[j] + initf_g(h, p.init_out, p.LD, j, p.D)) + p.dx[id + j - j0] : v[j];
      if (j == 0) {
        p.lm.cov[slot] = id, p.lm.col[slot] = -1, p.lm.rep[slot] = p.rep;
        p.lm.anchor[slot] = relative ? (int32_t)p.meas_cc[p.anchor_meas[p.f]] : -1;
        p.feat_slot[p.f] = slot;
      }
    }
    const int nb = max(p.C, p.K);
    for (int t = tid; t < nb; t += 256) boxplus_item(t, p.C, p.K, p.dx, p.clone_cov, p.calib_cov, p.intr_cov, p.clone_qp, p.calib_qp, p.intr);
    __syncthreads(); // the poses the tables are built from
    const int nt = max(p.K * p.C, nb);
    for (int t = tid; t < nt; t += 256) build_tables_item(t, p.C, p.K, p.clone_qp, p.clone_fej, p.calib_qp, p.tab_clone, p.tab_cam, p.tab_cc);
  }
  // every workgroup has read the counters by now; the one that arrives last advances them (nobody waits)
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(p.ctr + 4, 1) == (int)gridDim.x - 1) {
      if (!reject) p.ctr[0] = n1, p.ctr[1] = slot + 1;
      p.ctr[4] = 0;
    }
  }
}
__global__ void __launch_bounds__(256) k_initf_tail(InitFusedParams p) { initf_tail_body<false>(p, InitGateParams{nullptr, nullptr, nullptr}); }
__global__ void __launch_bounds__(256) k_initf_tail_gate(InitFusedParams p, InitGateParams g) { initf_tail_body<true>(p, g); }

} // namespace ovg
