// k_slam_y.h — the fused per-feature kernel of UpdaterSLAM::update: ONE sweep Y = H L on the matrix cores per feature feeds the stack and the
// chi2 gate (the form k_featy.h gives MSCKF features, for features whose landmark lives in the state).
//
//   UpdaterHelper::get_feature_jacobian_full            UpdaterHelper.cpp:192-424   (sys_measurement_rows, k_system.h: the sparse records)
//   UpdaterHelper::get_feature_jacobian_representation  UpdaterHelper.cpp:32-190    (anchored_rep_jacobian / inv_depth_jac, k_system.h)
//   chi2 gate on all 2m rows                            UpdaterSLAM.cpp:390-409
//   stacking into Hx_big / res_big                      UpdaterSLAM.cpp:427-447
//
// A 3-dof SLAM landmark has no nullspace projection and no reflectors: the rows [H | r] go into the stack as they are and the statistic is
// r^T S0^-1 r with S0 = H P H^T + s_f^2 I.  On the whitened route P_DD = L L^T is at hand (the prior block's factor, k_ekf.h), so
//
//        S0 = Y Y^T + s_f^2 I,        Y = H L     (2m x D, dense up to the landmark's last column)
//
// and the rows the stack wants ARE Y (scaled by sigma / sigma_f, a feature with its own noise level).  The general kernel (k_system_t) forms
// T = H P thread-per-column from P in L2, S0 = T H^T by per-thread gathers, factors S0 in LDS eight columns at a time and sweeps H L again
// for the stack: 0.49 ms per 25-feature chunk.
//
// One workgroup of SLY_NW wavefronts per feature, no cross-workgroup traffic, no spin wait:
//   prologue   representation Jacobian (one thread), the 72-double records + 8-int minfo of sys_measurement_rows (thread per measurement) -> LDS,
//              the residual column of the stack, the instance lists of the tile rows
//   per block of 64 columns:
//     sweep    wavefront w takes tile rows w, w + NW, .. (16 rows = 8 measurements): per instance — a column block some row of the tile row
//              touches: clone blocks (6), camera extrinsics (6) / intrinsics (8), the anchor clone / anchor extrinsics of an anchored landmark,
//              the landmark's own 3 columns — and per 16-column output tile   Y_tile += A B,  A[row][k] = H[row][fc + k] (the blocks of a row
//              that start at fc ADD: an anchor clone that is also the measurement's clone), B[k][col] = L[fc + k][col].  An instance whose
//              last column lies left of the output tile meets zeros of L only (lower triangular) and is skipped.             | barrier
//     store    rows 0 .. 2m-1 of oscale Y -> the stack (coalesced: a wavefront writes 512 contiguous bytes of a row)
//     SYRK     every wavefront: its tiles (i, j) of S0 += Y_i Y_j^T over the block's slabs of 8 columns                      | barrier
//   gate       M = [S0 + s_f^2 I, r; r^T, 0] (identity on the padding) eliminated by feat::gate_ldl_chi2<.., MODE 1>: chi2 = r^T S0^-1 r is the
//              corner entry alone — the three columns k_feat_y gives H_f stay zero and nothing is divided by them
//   outputs    k_system_t's for nproj == 0: chi2, chi2_thresh, status = CHI2_REJECTED / atomicAdd(rows_used, 2m) (an integer), and a rejected
//              feature — or one that did not arrive as USED — leaves its rows of the stack exactly zero.
// Every sum has a fixed order: two runs on the same inputs return the same bits.
// k_slam_y<true> adds the projection of single-depth landmarks, feature by feature (the comment at the kernel); k_slam_y<false> is the above.
// Two shapes (the template parameters at the kernel): tracks of up to 62 observations on 8 tile rows of the gate matrix and blocks of 64 columns, as described
// above; tracks of 63 .. 126 on 16 tile rows and blocks of 32 columns ("slam_fused" = 3), where a wavefront holds two rows of the block per pass of a store.
#pragma once
#include "k_featy.h"

namespace ovg {
namespace slamy {

using feat::d4;
using feat::lds_barrier;

constexpr int SLY_MMAX = 62; // the longest track the short shape holds: 2 m + 4 rows of the augmented gate matrix in 8 tile rows, 36 tiles of its upper triangle
constexpr int SLY_NW = 8;    // wavefronts per workgroup: one tile row of the sweep each at the bound
constexpr int SLY_TPW = 5;   // gate tiles per wavefront: 36 <= 8 x 5
constexpr int SLY_RS = 72;   // doubles per record (RO_* of k_system.h, anchor blocks included)
constexpr int SLY_CB = 64;   // columns per block
// the long shape, 63 .. 126 observations: 16 tile rows, 136 tiles of the upper triangle (feat::gate_ldl_chi2<8, 17, ..>, the template k_feat_y<8, 17, 1>
// instantiates), column blocks of 32 — the block of Y and the records of 126 measurements do not fit LDS side by side at 64
constexpr int SLY_MMAX_L = 126;
constexpr int SLY_TPW_L = 17; // 136 = 8 x 17
constexpr int SLY_CB_L = 32;
constexpr int SLY_INST = 27; // instances per tile row: <= 8 clone + 8 extrinsic + 8 intrinsic blocks, anchor clone, anchor extrinsics, landmark
constexpr int SLY_ISTR = 32; // ints per tile row in the instance table: [0] count, [1 ..] (width << 16) | first column

struct SlamYLds {
  size_t yb, rows, minfo, hq, stage, inst, misc, vq, hb1, zp, total;
};
// m_max: longest track of the batch (<= SLY_MMAX at cb = SLY_CB, <= SLY_MMAX_L at cb = SLY_CB_L); proj: the carve with the projection (the reflectors V, the
// saved second bearing column, the partial sums of z); cb: columns per block.  The single source of the carve for host and device.
__host__ __device__ inline SlamYLds slamy_lds_layout(int m_max, bool proj = false, int cb = SLY_CB) {
  SlamYLds L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15) & ~(size_t)15;
    return at;
  };
  const int nt = (2 * m_max + 15) >> 4, nta = (2 * m_max + 4 + 15) >> 4;
  const size_t blk = (size_t)16 * nt * (cb + 2) * sizeof(double), pan = (size_t)2 * nta * 256 * sizeof(double);
  L.yb = take(blk > pan ? blk : pan); // the block of Y; afterwards the gate's row panel, twice
  L.rows = take((size_t)m_max * SLY_RS * sizeof(double));
  L.minfo = take((size_t)m_max * 8 * sizeof(int));
  L.hq = take(64 * sizeof(double));
  L.stage = take((128 + 2 * 256) * sizeof(double)); // the gate's diagonal-tile stage: scratch, E, F
  L.inst = take((size_t)nt * SLY_ISTR * sizeof(int));
  L.misc = take(4 * sizeof(double));
  L.vq = L.hb1 = L.zp = o;
  if (proj) {
    L.vq = take((size_t)2 * m_max * 3 * sizeof(double));      // V of sys_hf_householder: [2 m][3], the third column the unit vector of a column that stays
    L.hb1 = take((size_t)2 * m_max * sizeof(double));          // H_f[:, 1] as the records gave it (the first reflector is applied to it in place)
    // V^T Y of the block: [quarter][k][column] in four row quarters at 64 columns; [wavefront][k][column] in eight segments of 32 rows at 32 columns — 4096 bytes
    // either way.  The long shape has no room for them next to the records (224 bytes over the limit at 126 observations): zp lives inside the column-block
    // loop only and the gate's stage behind it only, they share the stage's space.
    if (cb == SLY_CB) L.zp = take((size_t)SLY_NW * SLY_CB * sizeof(double));
    else L.zp = L.stage;
  }
  L.total = o;
  return L;
}

// ------------------------------------------------------------------ shared with the block-row shape (k_slam_y_big.h); each leaves its callers' code as it was
// representation Jacobian by ONE thread, as k_system_t (UpdaterHelper.cpp:32-190): hq[12..20] dpfg_dlambda, [21..38] H_anc, [39..56] H_calib
// (k_slam_y, k_slam_rows_big)
__device__ __forceinline__ void slamy_rep_jacobian(const SysParams &p, int f, int rep_f, int anchor_cam, int anchor_clone, const V3 &p_FinG, const V3 &p_FinG_fej,
                                                   double *hq) {
  double *dl = hq + 12;
  if (rep_f == OVGPU_REP_GLOBAL_3D) {
    dl[0] = 1, dl[1] = 0, dl[2] = 0, dl[3] = 0, dl[4] = 1, dl[5] = 0, dl[6] = 0, dl[7] = 0, dl[8] = 1;
  } else if (rep_f == OVGPU_REP_GLOBAL_FULL_INVERSE_DEPTH) {
    inv_depth_jac(p.opt.do_fej ? p_FinG_fej : p_FinG, dl); // UpdaterHelper.cpp:46
  } else {
    anchored_rep_jacobian(rep_f, p.opt.do_fej, p.tab_cam + 12 * anchor_cam, p.tab_clone + 24 * anchor_clone, load_v3(p.p_FinA + 3 * f), dl, hq + 21, hq + 39);
  }
}
// the gate's verdict by ONE thread: k_system_t's outputs for the statistic chi2 of a feature of n rows that gives the stack n_out (k_slam_y, k_slam_y_big)
__device__ __forceinline__ void slamy_verdict(const SysParams &p, int f, double mult_f, bool single, int n, int n_out, double chi2, int *reject_slot) {
  const double thr = mult_f * p.chi2_table[min(single ? n - 2 : n, p.chi2_table_len - 1)]; // UpdaterSLAM.cpp:392-405: dof = 2m (2m - 2 behind the projection)
  p.chi2[f] = chi2;
  p.chi2_thresh[f] = thr;
  const bool reject = chi2 > thr;
  *reject_slot = reject ? 1 : 0;
  if (reject) p.status[f] = OVGPU_FEAT_CHI2_REJECTED;
  else if (p.rows_used) atomicAdd(p.rows_used, n_out);
}

#ifndef OVG_TU_FEATY
// PROJ ("with projection"): a feature whose landmark is ANCHORED_INVERSE_DEPTH_SINGLE has its two bearing columns H_b = H_f[:, 0:2] projected out
// (UpdaterSLAM.cpp:338-341, :371-379; k_system_t's nproj == 2): the records are those of ANCHORED_MSCKF_INVERSE_DEPTH, the landmark's instance is
// (lm_col, width 1) with the UNREFLECTED depth column H_f[:, 2] — the two reflectors of H_b act on whole rows of [Y | r] afterwards — and per block
// z = T^T V^T Y (2 x 64 dot products over the 2m rows, four row quarters summed in a fixed order) gives the stack its rows 2 .. 2m-1 of
// Y - V z as rows 0 .. 2m-3.  The SYRK keeps reading the unprojected block: with S0 = Y Y^T + s_f^2 I the statistic of the projected rows is
// r^T S0^-1 r - g^T G^-1 g, g = H_b^T S0^-1 r, G = H_b^T S0^-1 H_b — the Schur complement gate_ldl_chi2 returns for R = [r | H_b | 0] with the identity
// entry at the corner's G22 — against the threshold at dof 2m - 2.  A 3-dof feature of such a batch does what it does in k_slam_y<false>.
// k_slam_y<false> is the kernel as it was: batches that observe no single-depth landmark take it and return the bits they returned.
// TPW / CB / MMAX: the shape — <.., 5, 64, 62> as it was, <.., 17, 32, 126> the long one (the same algebra and the same order of every sum a track of either
// shape takes, except z's partial sums, eight segments of 32 rows where the short shape has four quarters).  At 32 columns a wavefront holds two rows of a
// block at once in the per-column phases: lane = (row half hp, column), as k_feat_y does at its 32-column blocks.
template <bool PROJ, int TPW = SLY_TPW, int CB = SLY_CB, int MMAX = SLY_MMAX> __global__ void __launch_bounds__(64 * SLY_NW) k_slam_y(SysParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = SLY_NW, NTH = 64 * SLY_NW, RS = SLY_RS, LS = CB + 2;
  constexpr int NCTB = CB / 16; // column tiles per block
  constexpr int HP = 64 / CB;   // rows a wavefront holds at once in the per-column phases
  static_assert(CB == 64 || CB == 32, "column blocks of 64 or 32");
  static_assert(((2 * MMAX + 4 + 15) >> 4) * (((2 * MMAX + 4 + 15) >> 4) + 1) / 2 <= NW * TPW, "the gate's upper triangle exceeds the wavefronts' tiles");
  static_assert(2 * MMAX <= 32 * NW, "z's row segments do not cover the track");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, cl = lane & 15;
  const int D = p.D, LD = p.LD;
  const int colb = lane & (CB - 1), hp = lane / CB;
  const SlamYLds lo = slamy_lds_layout(p.m_max, PROJ, CB);
  double *Yb = reinterpret_cast<double *>(smem + lo.yb);
  const int nta_max = (2 * p.m_max + 4 + 15) >> 4;
  double *panel = Yb, *panelx = Yb + (size_t)nta_max * 256;
  double *rows = reinterpret_cast<double *>(smem + lo.rows);
  int *minfo = reinterpret_cast<int *>(smem + lo.minfo);
  double *hq = reinterpret_cast<double *>(smem + lo.hq); // [12..20] dpfg_dlambda, [21..38] H_anc, [39..56] H_calib (sys_measurement_rows)
  double *st0 = reinterpret_cast<double *>(smem + lo.stage), *stE = st0 + 128, *stF = st0 + 384;
  int *inst = reinterpret_cast<int *>(smem + lo.inst);
  double *chi2_slot = reinterpret_cast<double *>(smem + lo.misc);
  int *reject_slot = reinterpret_cast<int *>(chi2_slot + 1);
  double *Vq = reinterpret_cast<double *>(smem + lo.vq), *hb1 = reinterpret_cast<double *>(smem + lo.hb1), *zp = reinterpret_cast<double *>(smem + lo.zp); // PROJ only
  const int nblk = (D + CB - 1) / CB;

  for (int slot = p.f_begin + blockIdx.x; slot < p.f_end; slot += gridDim.x) {
    const int f = p.order ? p.order[slot] : slot; // longest tracks first
    const int m0 = p.meas_offsets[f];
    const int m = p.meas_offsets[f + 1] - m0;
    const int64_t orow0 = p.row_off[f];
    const int n_out = (int)(p.row_off[f + 1] - orow0); // 2m
    __syncthreads(); // the previous feature's LDS is fully consumed
    double *out = p.Hbig + orow0 * LD;
    if (p.status[f] != OVGPU_FEAT_USED || m > MMAX) { // failed before the gate: its rows of the stack are zero (m > MMAX: the host never sends such a batch)
      for (int64_t e = tid; e < (int64_t)n_out * LD; e += NTH) out[e] = 0.0;
      continue;
    }
    const int n = 2 * m, NT = (n + 15) >> 4, NTA = (n + 4 + 15) >> 4, NTT = NTA * (NTA + 1) / 2;

    // ------------------------------------------------------------------ (a0) representation Jacobian, as k_system_t (UpdaterHelper.cpp:32-190)
    V3 p_FinG = load_v3(p.p_FinG + 3 * f);
    const int lm_id = p.feat_lm[f], lm_col = p.feat_lmcol[f];
    const int rep_l = p.lm_rep[lm_id]; // <false>: a 3-dof representation — the host keeps batches with a single-depth landmark off this instantiation
    const bool single = PROJ && rep_l == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
    const int rep_f = single ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : rep_l; // the single depth takes the Jacobians of the MSCKF inverse depth (UpdaterSLAM.cpp:338-341)
    if (PROJ && single && m < 2) continue; // (no row to give: n_out = 0; k_slam_gather flags such a track OVGPU_FEAT_TOO_FEW_MEAS and it never gets here)
    const bool relative = rep_is_relative(rep_f);
    const double sig2_f = p.feat_sigma ? p.feat_sigma[f] * p.feat_sigma[f] : p.opt.sigma_pix_sq;
    const double mult_f = p.feat_chi2mult ? p.feat_chi2mult[f] : p.opt.chi2_multipler;
    const double oscale = p.feat_sigma ? sqrt(p.opt.sigma_pix_sq) / p.feat_sigma[f] : 1.0; // one isotropic noise level in the stack
    V3 p_FinG_fej = load_v3(p.p_fej + 3 * f);
    int anchor_cam = -1, anchor_clone = -1;
    if (relative) { // the landmark's anchor (UpdaterSLAM.cpp:345-348)
      const int ac = p.feat_anchor[f];
      anchor_cam = ac >> 10, anchor_clone = ac & 1023;
      const V3 p_FinA = load_v3(p.p_FinA + 3 * f);
      const M3 R_ItoC = load_m3(p.tab_cam + 12 * anchor_cam);
      const V3 p_IinC = load_v3(p.tab_cam + 12 * anchor_cam + 9);
      const M3 R_GtoI = load_m3(p.tab_clone + 24 * anchor_clone);
      const V3 p_IinG = load_v3(p.tab_clone + 24 * anchor_clone + 9);
      p_FinG = mulT(R_GtoI, mulT(R_ItoC, p_FinA - p_IinC)) + p_IinG; // UpdaterHelper.cpp:274
      p_FinG_fej = p_FinG;                                           // :279-283: the "best" estimate
    }
    if (tid == 0) slamy_rep_jacobian(p, f, rep_f, anchor_cam, anchor_clone, p_FinG, p_FinG_fej, hq);
    __syncthreads();
    // ------------------------------------------------------------------ (a) the records (UpdaterHelper.cpp:314-421)
    for (int i = tid; i < m; i += NTH) sys_measurement_rows(p, m0 + i, p_FinG, p_FinG_fej, relative, hq, minfo + 8 * i, rows + (size_t)i * RS);
    __syncthreads();
    const int anc_ccol = relative ? p.clone_col[anchor_clone] : -1;
    const int anc_pcol = (relative && p.opt.do_calib_pose) ? p.calib_col[anchor_cam] : -1;
    if (PROJ && single) {
      // the two reflectors of H_b and their T by one wavefront, arithmetic as k_system_t's (sys_hf_householder, nproj = 2); it applies the first reflector
      // to H_f[:, 1] in the records: the column is saved and put back, the gate and nothing else reads H_b afterwards.  z_r = T^T V^T r -> hq[61], hq[62]
      if (wv == 0) {
        for (int r = lane; r < n; r += 64) hb1[r] = rows[(size_t)(r >> 1) * RS + RO_HF + 3 * (r & 1) + 1];
        sys_hf_householder(rows, RS, Vq, hq, n, 2, lane);
        double y0 = 0.0, y1 = 0.0;
        for (int r = lane; r < n; r += 64) {
          const double rr = rows[(size_t)(r >> 1) * RS + RO_RES + (r & 1)];
          y0 = fma(Vq[(size_t)3 * r], rr, y0), y1 = fma(Vq[(size_t)3 * r + 1], rr, y1);
        }
        y0 = wave_sum(y0), y1 = wave_sum(y1);
        if (lane == 0) hq[61] = hq[3] * y0, hq[62] = hq[4] * y0 + hq[6] * y1;
        for (int r = lane; r < n; r += 64) rows[(size_t)(r >> 1) * RS + RO_HF + 3 * (r & 1) + 1] = hb1[r];
      }
      __syncthreads();
      // the residual column of the stack: rows 2 .. n-1 of r - V z_r
      const double zr0 = hq[61], zr1 = hq[62];
      for (int a = 2 + tid; a < n; a += NTH)
        out[(int64_t)(a - 2) * LD + D] = oscale * (rows[(size_t)(a >> 1) * RS + RO_RES + (a & 1)] - (Vq[(size_t)3 * a] * zr0 + Vq[(size_t)3 * a + 1] * zr1));
    } else {
      // the residual column of the stack
      for (int a = tid; a < n; a += NTH) out[(int64_t)a * LD + D] = oscale * rows[(size_t)(a >> 1) * RS + RO_RES + (a & 1)];
    }
    // the instance list of every tile row: the distinct first columns of the blocks its rows touch (blocks are disjoint column ranges: the
    // first column identifies one), in registers; one thread per tile row
    if (tid < NT) {
      int cand[SLY_INST];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int i = 8 * tid + j;
        const bool on = i < m;
        const int *mi = minfo + 8 * min(i, m - 1);
        const int c0 = mi[2], c1 = mi[3], c2 = mi[4];
        cand[3 * j] = (on && c0 >= 0) ? (c0 | (6 << 16)) : -1;
        cand[3 * j + 1] = (on && c1 >= 0) ? (c1 | (6 << 16)) : -1;
        cand[3 * j + 2] = (on && c2 >= 0) ? (c2 | (8 << 16)) : -1;
      }
      cand[24] = anc_ccol >= 0 ? (anc_ccol | (6 << 16)) : -1;
      cand[25] = anc_pcol >= 0 ? (anc_pcol | (6 << 16)) : -1;
      cand[26] = lm_col >= 0 ? (lm_col | ((single ? 1 : 3) << 16)) : -1; // a single depth: its one column carries H_f[:, 2]
      int *il = inst + tid * SLY_ISTR;
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < SLY_INST; e++) {
        bool keep = cand[e] >= 0;
#pragma unroll
        for (int q = 0; q < e; q++) keep = keep && cand[q] != cand[e];
        if (keep) il[1 + cnt++] = cand[e];
      }
      il[0] = cnt;
    }
    // this wavefront's gate tiles: linear index t = s NW + wv over the upper triangle column by column
    int tij[TPW]; // (j << 8) | i, or -1
    d4 acc[TPW];
#pragma unroll
    for (int s = 0; s < TPW; s++) {
      const int t = s * NW + wv;
      int i = -1, j = 0;
      if (t < NTT) {
        while ((j + 1) * (j + 2) / 2 <= t) j++;
        i = t - j * (j + 1) / 2;
      }
      tij[s] = __builtin_amdgcn_readfirstlane(i < 0 ? -1 : ((j << 8) | i));
      acc[s] = d4{0.0, 0.0, 0.0, 0.0};
    }
#define TI(s) (tij[s] & 255)
#define TJ(s) (tij[s] >> 8)
    __syncthreads();

    // ------------------------------------------------------------------ the column blocks
    for (int kb = 0; kb < nblk; kb++) {
      const int c_lo = CB * kb;
      // ---- sweep on the matrix cores: this wavefront's tile rows of Y = H L, columns c_lo .. c_lo + 63 -> LDS
      for (int i = wv; i < NT; i += NW) {
        const int r = 16 * i + cl;
        const bool rv = r < n;
        const int mr = min(r >> 1, m - 1), par = r & 1;
        const int *mi = minfo + 8 * mr;
        const int myc = rv ? mi[2] : -2, myp = rv ? mi[3] : -2, myi = rv ? mi[4] : -2;
        const int mya = rv ? anc_ccol : -2, myq = rv ? anc_pcol : -2, myl = rv ? lm_col : -2;
        const double *rd = rows + (size_t)mr * RS;
        const int g1 = min(4 + g, 5); // (k = 6, 7 of a 6-wide block are masked by the width test below)
        const double hC0 = rd[RO_CLONE + 6 * par + g], hC1 = rd[RO_CLONE + 6 * par + g1];
        const double hP0 = rd[RO_CPOSE + 6 * par + g], hP1 = rd[RO_CPOSE + 6 * par + g1];
        const double hI0 = rd[RO_CINTR + 8 * par + g], hI1 = rd[RO_CINTR + 8 * par + 4 + g];
        const double hA0 = relative ? rd[RO_ANC + 6 * par + g] : 0.0, hA1 = relative ? rd[RO_ANC + 6 * par + g1] : 0.0;
        const double hQ0 = relative ? rd[RO_ACAL + 6 * par + g] : 0.0, hQ1 = relative ? rd[RO_ACAL + 6 * par + g1] : 0.0;
        const double hF0 = rd[RO_HF + 3 * par + (single ? 2 : min(g, 2))];
        d4 ay[NCTB];
        bool okc[NCTB];
        int cc[NCTB];
#pragma unroll
        for (int ct = 0; ct < NCTB; ct++) {
          ay[ct] = d4{0.0, 0.0, 0.0, 0.0};
          okc[ct] = c_lo + 16 * ct + cl < D;
          cc[ct] = min(c_lo + 16 * ct + cl, D - 1); // clamped address, masked value
        }
        const int *il = inst + i * SLY_ISTR;
        const int cnt = __builtin_amdgcn_readfirstlane(il[0]);
#pragma unroll 1
        for (int e = 0; e < cnt; e++) {
          const int code = __builtin_amdgcn_readfirstlane(il[1 + e]);
          const int fc = code & 0xffff, w = code >> 16;
          if (fc + w - 1 < c_lo) continue; // left of the block: zeros of L only
          // the blocks of this lane's row that start at fc add (an anchor clone that is the measurement's own clone; anchor extrinsics of its camera)
          double a0 = (myc == fc ? hC0 : 0.0) + (myp == fc ? hP0 : 0.0) + (myi == fc ? hI0 : 0.0) + (myl == fc ? hF0 : 0.0);
          a0 += mya == fc ? hA0 : 0.0;
          a0 += myq == fc ? hQ0 : 0.0;
          double a1 = (myc == fc ? hC1 : 0.0) + (myp == fc ? hP1 : 0.0) + (myi == fc ? hI1 : 0.0);
          a1 += mya == fc ? hA1 : 0.0;
          a1 += myq == fc ? hQ1 : 0.0;
          a0 = g < w ? a0 : 0.0;     // k >= w: rows of L that belong to the next block
          a1 = 4 + g < w ? a1 : 0.0;
          const double *L0 = p.Lw + (size_t)min(fc + g, D - 1) * D, *L1 = p.Lw + (size_t)min(fc + 4 + g, D - 1) * D;
#pragma unroll
          for (int ct = 0; ct < NCTB; ct++) {
            if (fc + w - 1 < c_lo + 16 * ct || c_lo + 16 * ct >= D) continue; // (wave-uniform)
            const double b0 = okc[ct] ? L0[cc[ct]] : 0.0;
            FEAT_MFMA(a0, b0, ay[ct]);
            if (w > 4) {
              const double b1 = okc[ct] ? L1[cc[ct]] : 0.0;
              FEAT_MFMA(a1, b1, ay[ct]);
            }
          }
        }
#pragma unroll
        for (int ct = 0; ct < NCTB; ct++)
#pragma unroll
          for (int q = 0; q < 4; q++) Yb[(size_t)(16 * i + g + 4 * q) * LS + 16 * ct + cl] = ay[ct][q];
      }
      lds_barrier();
      if (PROJ && single) {
        if constexpr (CB == 64) {
          // ---- V^T Y of the block: wavefront wv takes reflector wv & 1 over the row quarter wv >> 1 (32 rows), lane = column                  | barrier
          const int k = wv & 1, r0 = 32 * (wv >> 1), r1 = min(r0 + 32, n);
          double y = 0.0;
          for (int a = r0; a < r1; a++) y = fma(Vq[(size_t)3 * a + k], Yb[(size_t)a * LS + lane], y);
          zp[wv * CB + lane] = y;
          lds_barrier();
          // ---- rows 2 .. n-1 of oscale (Y - V z), z = T^T V^T Y -> rows 0 .. n-3 of the stack
          const double y0 = ((zp[lane] + zp[2 * CB + lane]) + zp[4 * CB + lane]) + zp[6 * CB + lane];
          const double y1 = ((zp[CB + lane] + zp[3 * CB + lane]) + zp[5 * CB + lane]) + zp[7 * CB + lane];
          const double z0 = hq[3] * y0, z1 = hq[4] * y0 + hq[6] * y1; // T00, T01, T11 (sys_hf_householder)
          const int c = c_lo + lane;
          if (c < D)
            for (int a = 2 + wv; a < n; a += NW) out[(int64_t)(a - 2) * LD + c] = oscale * (Yb[(size_t)a * LS + lane] - (Vq[(size_t)3 * a] * z0 + Vq[(size_t)3 * a + 1] * z1));
        } else {
          // ---- V^T Y of the block: wavefront wv takes the rows 32 wv .. 32 wv + 31, lane = (reflector hp, column): 8 x 32 rows hold n <= 252                | barrier
          const int r0 = 32 * wv, r1 = min(r0 + 32, n);
          double y = 0.0;
          for (int a = r0; a < r1; a++) y = fma(Vq[(size_t)3 * a + hp], Yb[(size_t)a * LS + colb], y);
          zp[wv * 2 * CB + lane] = y; // [wv][hp][colb]
          lds_barrier();
          // ---- rows 2 .. n-1 of oscale (Y - V z) -> rows 0 .. n-3 of the stack; the eight segments summed first to last
          double y0 = zp[colb], y1 = zp[CB + colb];
#pragma unroll
          for (int w8 = 1; w8 < NW; w8++) y0 += zp[w8 * 2 * CB + colb], y1 += zp[w8 * 2 * CB + CB + colb];
          const double z0 = hq[3] * y0, z1 = hq[4] * y0 + hq[6] * y1; // T00, T01, T11 (sys_hf_householder)
          const int c = c_lo + colb;
          if (c < D)
            for (int a = 2 + HP * wv + hp; a < n; a += HP * NW) out[(int64_t)(a - 2) * LD + c] = oscale * (Yb[(size_t)a * LS + colb] - (Vq[(size_t)3 * a] * z0 + Vq[(size_t)3 * a + 1] * z1));
        }
      } else {
        // ---- rows of oscale Y -> the stack
        if constexpr (CB == 64) {
          const int c = c_lo + lane;
          if (c < D)
            for (int a = wv; a < n; a += NW) out[(int64_t)a * LD + c] = oscale * Yb[(size_t)a * LS + lane];
        } else { // a wavefront writes two rows' 256 contiguous bytes
          const int c = c_lo + colb;
          if (c < D)
            for (int a = HP * wv + hp; a < n; a += HP * NW) out[(int64_t)a * LD + c] = oscale * Yb[(size_t)a * LS + colb];
        }
      }
      // ---- SYRK: S0 tiles += Y_i Y_j^T over the block's slabs of 8 columns (columns >= D of the block hold zeros)
      const int nsl = min(CB / 8, (D - 1 - c_lo) / 8 + 1);
#pragma unroll
      for (int s = 0; s < TPW; s++) {
        if (tij[s] >= 0 && TJ(s) < NT) {
          const double *ya = Yb + (size_t)(16 * TI(s) + cl) * LS + 2 * g, *yb = Yb + (size_t)(16 * TJ(s) + cl) * LS + 2 * g;
#pragma unroll 2
          for (int sl = 0; sl < nsl; sl++) {
            const double2 a = *reinterpret_cast<const double2 *>(ya + 8 * sl), b = *reinterpret_cast<const double2 *>(yb + 8 * sl);
            FEAT_MFMA(a.x, b.x, acc[s]);
            FEAT_MFMA(a.y, b.y, acc[s]);
          }
        }
      }
      lds_barrier(); // the block is free again
    }

    // ------------------------------------------------------------------ M = [Y Y^T + s_f^2 I, r; r^T, 0]: r in column n4 (identity on the padding; the columns n4+1 .. n4+3 stay zero)
    const int n4 = (n + 3) & ~3;
#pragma unroll
    for (int s = 0; s < TPW; s++) {
      if (tij[s] < 0) continue;
      if (16 * TJ(s) + 15 >= n) { // a tile that reaches the augmented columns / the padding
        const int b = 16 * TJ(s) + cl;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int a = 16 * TI(s) + g + 4 * q;
          double v = acc[s][q];
          if (a == b) v = a < n ? v + sig2_f : ((a >= n4 && a < n4 + 4) ? 0.0 : 1.0);
          else if (a < n && b == n4) v = rows[(size_t)(a >> 1) * RS + RO_RES + (a & 1)];
          else if (PROJ && single && a < n && (b == n4 + 1 || b == n4 + 2)) v = rows[(size_t)(a >> 1) * RS + RO_HF + 3 * (a & 1) + b - n4 - 1]; // H_b
          acc[s][q] = v;
        }
      } else if (TI(s) == TJ(s)) {
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (g + 4 * q == cl) acc[s][q] += sig2_f;
      }
    }
    const double chi2 = feat::gate_ldl_chi2<NW, TPW, PROJ ? 2 : 1>(acc, tij, NT, NTA, n, panel, panelx, st0, stE, stF, chi2_slot, lane, wv, single);
    if (tid == 0) slamy_verdict(p, f, mult_f, single, n, n_out, chi2, reject_slot);
    __syncthreads(); // (a full barrier: the other wavefronts' stores to the feature's rows have landed)
    if (*reject_slot)
      for (int64_t e = tid; e < (int64_t)n_out * LD; e += NTH) out[e] = 0.0;
#undef TI
#undef TJ
  }
}
#endif // OVG_TU_FEATY

} // namespace slamy
} // namespace ovg
