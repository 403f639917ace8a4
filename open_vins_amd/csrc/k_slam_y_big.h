// k_slam_y_big.h — k_slam_y (k_slam_y.h) for tracks whose gate matrix does not fit the registers of a compute unit: the algebra of k_slam_y on the
// pass structure of k_feat_y_big (k_featy_big.h).  Tracks of 127 .. SLY_MMAX_B observations under ovgpu_debug_option "slam_fused_big".
//
//   algebra   Y = H L on the matrix cores from the sparse 72-double records (clone, extrinsic, intrinsic blocks, the anchor clone / anchor extrinsics
//             of an anchored landmark — an anchor clone that is the measurement's own clone ADDS — and the landmark's own columns),
//             S0 = Y Y^T + s_f^2 I with per-feature sigma / multiplier; 3-dof: rows oscale [Y | r] to the stack, chi2 = r^T S0^-1 r at dof 2m;
//             single depth (PROJ): the two reflectors of the bearing columns act on whole rows on their way to the stack (rows 2 .. 2m-1 become
//             rows 0 .. 2m-3), chi2 = r^T S0^-1 r - g^T G^-1 g with the 2 x 2 G = H_b^T S0^-1 H_b at dof 2m - 2
//   passes    a pass owns tile rows [a, b) of the upper triangle, each from its diagonal tile to the right-hand-side tile column NT = [r | H_b | 0], as
//             many rows as fit SLY_NW x SLY_TPW_B = 136 accumulator tiles:
//             (A) sweep + SYRK per 32-column block (the first pass alone stores to the stack, later passes repeat the sweep of the rows >= a)
//             (B) S_ij -= sum_{k < a} W_ki^T W_kj, the earlier passes' row panels from a per-workgroup scratch in L2, double-buffered in LDS
//             (C) factor and solve of the rows a .. b-1; the solved right-hand sides stay in LDS across the passes, every pass ends with a full barrier
//             and the statistic comes from them after the last pass: chi2 = |y_r|^2 - g^T G^-1 g, y = U^-T [r | H_b].
//             With 136 tiles the number of passes changes at 168 | 169 observations (two to three) and 208 | 209 (three to four).
//   records   232 records are 133 632 bytes, next to a 126 208-byte block of Y: k_slam_y's prologue is a kernel of its own (k_slam_rows_big) in front
//             on the same stream — records and minfo (thread per measurement), the representation Jacobian and, PROJ, the reflectors (per feature),
//             the tile rows' instance lists — into workspaces in memory the big kernel reads.  The records keep H_b as sys_measurement_rows gave it
//             (the first reflector is applied to a copy), so nothing has to be saved and put back.
// One workgroup of 8 wavefronts per feature slot, longest tracks first; no cross-workgroup traffic, no spin wait, no float atomic (atomicAdd(rows_used, ..),
// an integer, is the only one); every sum has a fixed order: two runs on the same inputs return the same bits.  A rejected feature — or one that did
// not arrive as USED — leaves its rows of the stack exactly zero.  A short track of a big batch goes through its single pass.
//
// The upper bound SLY_MMAX_B = 232 observations (29 tile rows), MSCKF's: both carves fit the 163 840-byte limit there (149 440 / 156 864 bytes); 233
// observations are 30 tile rows, one more than a fetched row panel's prefetch registers hold (FB_PF), and keep k_system_t.
#pragma once
#include "k_featy_big.h"
#include "k_slam_y.h"

namespace ovg {
namespace slamy {

constexpr int SLY_MMAX_B = 232; // the longest track the big shape holds
constexpr int SLY_NT_B = 29;    // ... in tile rows: (2 x 232 + 15) / 16
constexpr int SLY_TPW_B = 17;   // accumulator tiles per wavefront: passes of up to 8 x 17 = 136 tiles, k_feat_y_big<8, 17>'s plan

struct SlamYBigLds {
  size_t yb, vl, wpart, rhs, inst, hq, misc, total;
};
// nt_max: tile rows of the batch's longest track (<= SLY_NT_B); proj: the carve with the projection (the two reflectors' columns of V).  The single
// source of the carve for host and device.
__host__ __device__ inline SlamYBigLds slamyb_lds_layout(int nt_max, bool proj) {
  SlamYBigLds L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15) & ~(size_t)15;
    return at;
  };
  const size_t blk = (size_t)16 * nt_max * feat::FB_LS * sizeof(double), pan = (size_t)2 * (nt_max + 1) * 256 * sizeof(double);
  L.yb = take(blk > pan ? blk : pan); // the block of Y; in phases (B), (C) two row panels of (nt_max + 1) tiles
  L.vl = o;
  if (proj) L.vl = take((size_t)16 * nt_max * 2 * sizeof(double)); // V[:, 0:2] of sys_hf_householder
  const size_t wp = (size_t)SLY_NW * 2 * feat::FB_CB * sizeof(double), stage = 2 * 256 * sizeof(double);
  L.wpart = take(wp > stage ? wp : stage); // V^T Y's partial sums per wavefront; in phase (C) the diagonal-tile stage
  L.rhs = take((size_t)16 * nt_max * 4 * sizeof(double)); // solved right-hand sides: they live across the passes
  L.inst = take((size_t)nt_max * SLY_ISTR * sizeof(int));
  L.hq = take(64 * sizeof(double));
  L.misc = take(8 * sizeof(double));
  L.total = o;
  return L;
}
// the batch's longest track fits the big shape: its tile rows within the bound (a fetched row panel is at most SLY_NT_B + 1 tiles) and its carve within `limit`
__host__ __device__ inline bool slamyb_holds(int m_max, bool proj, size_t limit) {
  const int nt = (2 * m_max + 15) >> 4;
  return m_max <= SLY_MMAX_B && nt <= SLY_NT_B && slamyb_lds_layout(nt > 0 ? nt : 1, proj).total <= limit;
}
// dynamic LDS of the records kernel: hq, a copy of H_f (6 m), V (6 m), the residuals (2 m), the three block columns of every measurement
__host__ __device__ inline size_t slamyb_rows_lds(int m_max) { return ((size_t)64 + 14 * m_max) * sizeof(double) + (((size_t)3 * m_max * sizeof(int)) + 15 & ~(size_t)15); }

// the workspaces the records kernel fills and the big kernel reads (plan: size_feature_stage)
struct SlamYBigStore {
  double *rows;   // [M][SLY_RS] the records of sys_measurement_rows
  int32_t *minfo; // [M][8]
  double *V;      // [2 M][3] PROJ: the reflectors of a single-depth feature
  double *hq;     // [F][64] [3], [4], [6]: T00, T01, T11; [61], [62]: z_r = T^T V^T r
  int32_t *inst;  // [F][SLY_NT_B][SLY_ISTR] the tile rows' instance lists: [0] count, [1 ..] (width << 16) | first column
};

#if !defined(OVG_TU_FEATY) || defined(OVG_TU_SLAMY_BIG) // (templates of a translation unit of their own: ovgpu_slamy_big_tu.hip)
// k_slam_y's prologue for one feature per workgroup (the slot blockIdx.x of the launch's range, as the big kernel orders them)
template <bool PROJ> __global__ void __launch_bounds__(256) k_slam_rows_big(SysParams p, SlamYBigStore st) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NTH = 256, RS = SLY_RS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int slot = p.f_begin + blockIdx.x;
  if (slot >= p.f_end) return;
  const int f = p.order ? p.order[slot] : slot;
  const int m0 = p.meas_offsets[f];
  const int m = p.meas_offsets[f + 1] - m0;
  if (p.status[f] != OVGPU_FEAT_USED || m > SLY_MMAX_B || m > p.m_max) return; // (the big kernel zeroes its rows)
  double *hq = reinterpret_cast<double *>(smem);
  double *hf = hq + 64, *V = hf + (size_t)6 * p.m_max, *res = V + (size_t)6 * p.m_max;
  int *mcol = reinterpret_cast<int *>(res + (size_t)2 * p.m_max);
  const int n = 2 * m, NT = (n + 15) >> 4;
  if (tid < 64) hq[tid] = 0.0;
  __syncthreads();
  // ------------------------------------------------------------------ representation Jacobian, as k_slam_y (UpdaterHelper.cpp:32-190)
  V3 p_FinG = load_v3(p.p_FinG + 3 * f);
  const int lm_id = p.feat_lm[f], lm_col = p.feat_lmcol[f];
  const int rep_l = p.lm_rep[lm_id];
  const bool single = PROJ && rep_l == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
  const int rep_f = single ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : rep_l;
  const bool relative = rep_is_relative(rep_f);
  V3 p_FinG_fej = load_v3(p.p_fej + 3 * f);
  int anchor_cam = -1, anchor_clone = -1;
  if (relative) {
    const int ac = p.feat_anchor[f];
    anchor_cam = ac >> 10, anchor_clone = ac & 1023;
    const V3 p_FinA = load_v3(p.p_FinA + 3 * f);
    const M3 R_ItoC = load_m3(p.tab_cam + 12 * anchor_cam);
    const V3 p_IinC = load_v3(p.tab_cam + 12 * anchor_cam + 9);
    const M3 R_GtoI = load_m3(p.tab_clone + 24 * anchor_clone);
    const V3 p_IinG = load_v3(p.tab_clone + 24 * anchor_clone + 9);
    p_FinG = mulT(R_GtoI, mulT(R_ItoC, p_FinA - p_IinC)) + p_IinG;
    p_FinG_fej = p_FinG;
  }
  if (tid == 0) slamy_rep_jacobian(p, f, rep_f, anchor_cam, anchor_clone, p_FinG, p_FinG_fej, hq);
  __syncthreads();
  // ------------------------------------------------------------------ the records (UpdaterHelper.cpp:314-421) -> memory; H_f, r and the block columns -> LDS
  for (int i = tid; i < m; i += NTH) {
    double *rd = st.rows + (size_t)(m0 + i) * RS;
    int32_t *mi = st.minfo + (size_t)8 * (m0 + i);
    sys_measurement_rows(p, m0 + i, p_FinG, p_FinG_fej, relative, hq, mi, rd);
#pragma unroll
    for (int q = 0; q < 6; q++) hf[6 * i + q] = rd[RO_HF + q];
    res[2 * i] = rd[RO_RES], res[2 * i + 1] = rd[RO_RES + 1];
    mcol[3 * i] = mi[2], mcol[3 * i + 1] = mi[3], mcol[3 * i + 2] = mi[4];
  }
  __syncthreads();
  if (PROJ && single && m >= 2 && wv == 0) {
    // the two reflectors of H_b and their T by one wavefront, arithmetic as k_system_t's (sys_hf_householder, nproj = 2), on the copy of H_f
    sys_hf_householder(hf - RO_HF, 6, V, hq, n, 2, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y0 = 0.0, y1 = 0.0;
    for (int r = lane; r < n; r += 64) {
      const double rr = res[r];
      y0 = fma(V[(size_t)3 * r], rr, y0), y1 = fma(V[(size_t)3 * r + 1], rr, y1);
      double *vo = st.V + ((size_t)2 * m0 + r) * 3;
      vo[0] = V[3 * r], vo[1] = V[3 * r + 1], vo[2] = V[3 * r + 2];
    }
    y0 = wave_sum(y0), y1 = wave_sum(y1);
    if (lane == 0) hq[61] = hq[3] * y0, hq[62] = hq[4] * y0 + hq[6] * y1; // z_r = T^T V^T r
  }
  __syncthreads();
  if (tid < 64) st.hq[(size_t)64 * f + tid] = hq[tid];
  // the instance list of every tile row: the distinct first columns of the blocks its rows touch, one thread per tile row (k_slam_y)
  const int anc_ccol = relative ? p.clone_col[anchor_clone] : -1;
  const int anc_pcol = (relative && p.opt.do_calib_pose) ? p.calib_col[anchor_cam] : -1;
  if (tid < NT) {
    int cand[SLY_INST];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int i = 8 * tid + j;
      const bool on = i < m;
      const int *mi = mcol + 3 * min(i, m - 1);
      const int c0 = mi[0], c1 = mi[1], c2 = mi[2];
      cand[3 * j] = (on && c0 >= 0) ? (c0 | (6 << 16)) : -1;
      cand[3 * j + 1] = (on && c1 >= 0) ? (c1 | (6 << 16)) : -1;
      cand[3 * j + 2] = (on && c2 >= 0) ? (c2 | (8 << 16)) : -1;
    }
    cand[24] = anc_ccol >= 0 ? (anc_ccol | (6 << 16)) : -1;
    cand[25] = anc_pcol >= 0 ? (anc_pcol | (6 << 16)) : -1;
    cand[26] = lm_col >= 0 ? (lm_col | ((single ? 1 : 3) << 16)) : -1; // a single depth: its one column carries H_f[:, 2]
    int32_t *il = st.inst + ((size_t)f * SLY_NT_B + tid) * SLY_ISTR;
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
}

// PROJ as k_slam_y's: a feature whose landmark is ANCHORED_INVERSE_DEPTH_SINGLE has its two bearing columns projected out; a 3-dof feature of such a
// batch does what it does in k_slam_y_big<false>.  nt_max: tile rows of the batch's longest track, the carve's and the scratch's parameter.
template <bool PROJ> __global__ void __launch_bounds__(64 * SLY_NW, 1) k_slam_y_big(SysParams p, int nt_max, SlamYBigStore st, double *wsG) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = SLY_NW, NTH = 64 * SLY_NW, TPW = SLY_TPW_B, RS = SLY_RS, CB = feat::FB_CB, LS = feat::FB_LS, PF = feat::FB_PF;
  static_assert(PF * NTH >= (SLY_NT_B + 1) * 256, "a fetched row panel must fit the prefetch registers");
  static_assert(SLY_NT_B + 1 <= NW * TPW, "a tile row with its right-hand sides exceeds a pass");
  static_assert(2 * SLY_MMAX_B <= 16 * SLY_NT_B, "the bound's rows exceed its tile rows");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, cl = lane & 15;
  const int D = p.D, LD = p.LD;
  const SlamYBigLds lo = slamyb_lds_layout(nt_max, PROJ);
  double *Yb = reinterpret_cast<double *>(smem + lo.yb);
  double *panel0 = Yb, *panel1 = Yb + (size_t)(nt_max + 1) * 256;
  double *Vl = reinterpret_cast<double *>(smem + lo.vl); // PROJ only
  double *wpart = reinterpret_cast<double *>(smem + lo.wpart);
  double *st0 = wpart, *st1 = wpart + 256;
  double *rhs = reinterpret_cast<double *>(smem + lo.rhs);
  int *inst = reinterpret_cast<int *>(smem + lo.inst);
  double *hq = reinterpret_cast<double *>(smem + lo.hq);
  int *reject_slot = reinterpret_cast<int *>(smem + lo.misc);
  double *ws = wsG + (size_t)blockIdx.x * feat::featyb_ws_doubles(nt_max);
  const int nblk = (D + CB - 1) / CB;
  const int col32 = lane & 31, hp = lane >> 5;
  // the scratch is read back by other wavefronts of this workgroup: past the vector cache (it may hold the previous track's panels)
  auto ld_l2 = [](const double *ptr) { return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

  for (int slot = p.f_begin + blockIdx.x; slot < p.f_end; slot += gridDim.x) {
    const int f = p.order ? p.order[slot] : slot; // longest tracks first
    const int m0 = p.meas_offsets[f];
    const int m = p.meas_offsets[f + 1] - m0;
    const int64_t orow0 = p.row_off[f];
    const int n_out = (int)(p.row_off[f + 1] - orow0);
    __syncthreads(); // the previous feature's LDS is fully consumed
    double *out = p.Hbig + orow0 * LD;
    const int n = 2 * m, NT = (n + 15) >> 4;
    if (p.status[f] != OVGPU_FEAT_USED || NT > nt_max || NT > SLY_NT_B) { // failed before the gate: its rows of the stack are zero (a track beyond the carve: the host never sends such a batch)
      for (int64_t e = tid; e < (int64_t)n_out * LD; e += NTH) out[e] = 0.0;
      continue;
    }
    const int lm_id = p.feat_lm[f], lm_col = p.feat_lmcol[f];
    const int rep_l = p.lm_rep[lm_id];
    const bool single = PROJ && rep_l == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
    const int rep_f = single ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : rep_l;
    if (PROJ && single && m < 2) continue; // (no row to give: n_out = 0)
    const bool relative = rep_is_relative(rep_f);
    const double sig2_f = p.feat_sigma ? p.feat_sigma[f] * p.feat_sigma[f] : p.opt.sigma_pix_sq;
    const double mult_f = p.feat_chi2mult ? p.feat_chi2mult[f] : p.opt.chi2_multipler;
    const double oscale = p.feat_sigma ? sqrt(p.opt.sigma_pix_sq) / p.feat_sigma[f] : 1.0; // one isotropic noise level in the stack
    int anchor_cam = -1, anchor_clone = -1;
    if (relative) {
      const int ac = p.feat_anchor[f];
      anchor_cam = ac >> 10, anchor_clone = ac & 1023;
    }
    const int anc_ccol = relative ? p.clone_col[anchor_clone] : -1;
    const int anc_pcol = (relative && p.opt.do_calib_pose) ? p.calib_col[anchor_cam] : -1;
    const double *frow = st.rows + (size_t)m0 * RS;
    const int32_t *finfo = st.minfo + (size_t)8 * m0;

    // ------------------------------------------------------------------ prologue: what k_slam_rows_big left for this feature
    if (tid < 64) hq[tid] = st.hq[(size_t)64 * f + tid];
    for (int e = tid; e < NT * SLY_ISTR; e += NTH) inst[e] = st.inst[(size_t)f * SLY_NT_B * SLY_ISTR + e];
    if (PROJ && single)
      for (int r = tid; r < n; r += NTH) {
        const double *vi = st.V + ((size_t)2 * m0 + r) * 3;
        Vl[2 * r] = vi[0], Vl[2 * r + 1] = vi[1];
      }
    __syncthreads();
    const double T00 = hq[3], T01 = hq[4], T11 = hq[6];
    if (PROJ && single) { // the residual column of the stack: rows 2 .. n-1 of r - V z_r
      const double zr0 = hq[61], zr1 = hq[62];
      for (int a = 2 + tid; a < n; a += NTH)
        out[(int64_t)(a - 2) * LD + D] = oscale * (frow[(size_t)(a >> 1) * RS + RO_RES + (a & 1)] - (Vl[2 * a] * zr0 + Vl[2 * a + 1] * zr1));
    } else {
      for (int a = tid; a < n; a += NTH) out[(int64_t)a * LD + D] = oscale * frow[(size_t)(a >> 1) * RS + RO_RES + (a & 1)];
    }

    // ------------------------------------------------------------------ the passes over block rows [a, b)
    int a = 0;
    while (a < NT) {
      int b = a, cnt = 0;
      while (b < NT && cnt + (NT + 1 - b) <= NW * TPW) cnt += NT + 1 - b, b++;
      // this wavefront's tiles: t = s NW + wv over the rows a .. b-1, each from its diagonal tile to the right-hand-side column NT
      int tij[TPW]; // (j << 8) | i, or -1
      d4 acc[TPW];
#pragma unroll
      for (int s = 0; s < TPW; s++) {
        const int t = s * NW + wv;
        int i = -1, j = 0;
        if (t < cnt) {
          int rem = t;
          i = a;
          while (rem >= NT + 1 - i) rem -= NT + 1 - i, i++;
          j = i + rem;
        }
        tij[s] = i < 0 ? -1 : ((j << 8) | i);
        acc[s] = d4{0.0, 0.0, 0.0, 0.0};
      }
#define TI(s) (tij[s] & 255)
#define TJ(s) (tij[s] >> 8)

      // ---------------------------------------------------------------- (A) the column blocks
      for (int kb = 0; kb < nblk; kb++) {
        const int c_lo = CB * kb;
        for (int i = a + wv; i < NT; i += NW) { // sweep on the matrix cores: tile rows >= a of Y = H L, columns c_lo .. c_lo + 31 -> LDS
          const int r = 16 * i + cl;
          const bool rv = r < n;
          const int mr = min(r >> 1, m - 1), par = r & 1;
          const int32_t *mi = finfo + 8 * mr;
          const int myc = rv ? mi[2] : -2, myp = rv ? mi[3] : -2, myi = rv ? mi[4] : -2;
          const int mya = rv ? anc_ccol : -2, myq = rv ? anc_pcol : -2, myl = rv ? lm_col : -2;
          const double *rd = frow + (size_t)mr * RS;
          const int g1 = min(4 + g, 5); // (k = 6, 7 of a 6-wide block are masked by the width test below)
          const double hC0 = rd[RO_CLONE + 6 * par + g], hC1 = rd[RO_CLONE + 6 * par + g1];
          const double hP0 = rd[RO_CPOSE + 6 * par + g], hP1 = rd[RO_CPOSE + 6 * par + g1];
          const double hI0 = rd[RO_CINTR + 8 * par + g], hI1 = rd[RO_CINTR + 8 * par + 4 + g];
          const double hA0 = relative ? rd[RO_ANC + 6 * par + g] : 0.0, hA1 = relative ? rd[RO_ANC + 6 * par + g1] : 0.0;
          const double hQ0 = relative ? rd[RO_ACAL + 6 * par + g] : 0.0, hQ1 = relative ? rd[RO_ACAL + 6 * par + g1] : 0.0;
          const double hF0 = rd[RO_HF + 3 * par + (single ? 2 : min(g, 2))];
          d4 ay[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
          const bool okc[2] = {c_lo + cl < D, c_lo + 16 + cl < D};
          const int cc[2] = {min(c_lo + cl, D - 1), min(c_lo + 16 + cl, D - 1)}; // clamped address, masked value
          const int *il = inst + i * SLY_ISTR;
          const int cnt_i = __builtin_amdgcn_readfirstlane(il[0]);
#pragma unroll 1
          for (int e = 0; e < cnt_i; e++) {
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
            a0 = g < w ? a0 : 0.0; // k >= w: rows of L that belong to the next block
            a1 = 4 + g < w ? a1 : 0.0;
            const double *L0 = p.Lw + (size_t)min(fc + g, D - 1) * D, *L1 = p.Lw + (size_t)min(fc + 4 + g, D - 1) * D;
#pragma unroll
            for (int ct = 0; ct < 2; ct++) {
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
          for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int q = 0; q < 4; q++) Yb[(size_t)(16 * i + g + 4 * q) * LS + 16 * ct + cl] = ay[ct][q];
        }
        lds_barrier();
        if (a == 0) { // first pass: the rows leave for the stack (half a wavefront per row: lane & 31 = column)
          const int c = c_lo + col32;
          if (PROJ && single) {
            // V^T Y of the block: wavefront wv takes the rows 2 wv + hp, + 16, ..; the halves by a shuffle, the wavefronts first to last      | barrier
            double w0 = 0.0, w1 = 0.0;
#pragma unroll 4
            for (int r = 2 * wv + hp; r < n; r += 2 * NW) {
              const double y = Yb[(size_t)r * LS + col32];
              w0 = fma(Vl[2 * r], y, w0), w1 = fma(Vl[2 * r + 1], y, w1);
            }
            w0 += __shfl_xor(w0, 32, 64), w1 += __shfl_xor(w1, 32, 64);
            if (hp == 0) wpart[(wv * 2 + 0) * CB + col32] = w0, wpart[(wv * 2 + 1) * CB + col32] = w1;
            lds_barrier();
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int w = 0; w < NW; w++) s0 += wpart[(w * 2 + 0) * CB + col32], s1 += wpart[(w * 2 + 1) * CB + col32];
            const double z0 = T00 * s0, z1 = T01 * s0 + T11 * s1; // z = T^T V^T Y
            // rows 2 .. n-1 of oscale (Y - V z) -> rows 0 .. n-3 of the stack
            if (c < D) {
#pragma unroll 4
              for (int r = 2 + 2 * wv + hp; r < n; r += 2 * NW)
                out[(int64_t)(r - 2) * LD + c] = oscale * (Yb[(size_t)r * LS + col32] - (Vl[2 * r] * z0 + Vl[2 * r + 1] * z1));
            }
          } else if (c < D) {
#pragma unroll 4
            for (int r = 2 * wv + hp; r < n; r += 2 * NW) out[(int64_t)r * LD + c] = oscale * Yb[(size_t)r * LS + col32];
          }
        }
        // SYRK: this pass's tiles += Y_i Y_j^T over the block's slabs of 8 columns (columns >= D of the block hold zeros)
        const int nsl = min(CB / 8, (D - 1 - c_lo) / 8 + 1);
#pragma unroll
        for (int s = 0; s < TPW; s++) {
          if (tij[s] >= 0 && TJ(s) < NT) {
            const double *ya = Yb + (size_t)(16 * TI(s) + cl) * LS + 2 * g, *yb = Yb + (size_t)(16 * TJ(s) + cl) * LS + 2 * g;
#pragma unroll 2
            for (int sl = 0; sl < nsl; sl++) {
              const double2 va = *reinterpret_cast<const double2 *>(ya + 8 * sl), vb = *reinterpret_cast<const double2 *>(yb + 8 * sl);
              FEAT_MFMA(va.x, vb.x, acc[s]);
              FEAT_MFMA(va.y, vb.y, acc[s]);
            }
          }
        }
        lds_barrier(); // the block is free again
      }

      // S0 = Y Y^T + s_f^2 I (identity on the padding); right-hand sides [r | H_b | 0]
#pragma unroll
      for (int s = 0; s < TPW; s++) {
        if (tij[s] < 0) continue;
        if (TJ(s) == NT) {
          int lane_o; // (opaque, and from the hardware: see k_featy.h)
          asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_o));
          const int go = lane_o >> 4, clo = lane_o & 15;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int r = 16 * TI(s) + go + 4 * q;
            double v = 0.0;
            if (r < n && (clo == 0 || (PROJ && single && clo < 3))) {
              const double *rd = frow + (size_t)(r >> 1) * RS;
              v = clo == 0 ? rd[RO_RES + (r & 1)] : rd[RO_HF + 3 * (r & 1) + clo - 1];
            }
            acc[s][q] = v;
          }
        } else if (TI(s) == TJ(s)) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int r = 16 * TI(s) + g + 4 * q;
            if (g + 4 * q == cl) acc[s][q] = r < n ? acc[s][q] + sig2_f : 1.0;
          }
        }
      }

      // ---------------------------------------------------------------- (B) the earlier passes' row panels: S_ij -= W_ki^T W_kj, k < a
      if (a > 0) {
        const int nfetch = (NT + 1 - a) * 256; // tiles a .. NT of a row panel, contiguous in the scratch
        double pf[PF];
        auto fetch = [&](int k) {
          const double *src = ws + ((size_t)k * (nt_max + 1) + a) * 256;
#pragma unroll
          for (int q = 0; q < PF; q++) {
            const int e = tid + NTH * q;
            pf[q] = ld_l2(src + (e < nfetch ? e : nfetch - 1));
          }
        };
        auto stash = [&](double *buf) {
          double *dst = buf + (size_t)a * 256;
#pragma unroll
          for (int q = 0; q < PF; q++) {
            const int e = tid + NTH * q;
            if (e < nfetch) dst[e] = pf[q];
          }
        };
        fetch(0);
        stash(panel0);
        for (int k = 0; k < a; k++) {
          const double *cur = (k & 1) ? panel1 : panel0;
          double *nxt = (k & 1) ? panel0 : panel1;
          lds_barrier(); // panel k is complete; panel k - 1 (= nxt) has been consumed by everybody
          const bool more = k + 1 < a;
          if (more) fetch(k + 1);
#pragma unroll
          for (int s = 0; s < TPW; s++) {
            if (tij[s] >= 0) {
              const double *pi = cur + (size_t)TI(s) * 256, *pj = cur + (size_t)TJ(s) * 256;
              double va[4], vb[4];
#pragma unroll
              for (int u = 0; u < 4; u++) va[u] = -pi[(4 * u + g) * 16 + cl], vb[u] = pj[(4 * u + g) * 16 + cl];
#pragma unroll
              for (int u = 0; u < 4; u++) FEAT_MFMA(va[u], vb[u], acc[s]);
            }
          }
          if (more) stash(nxt);
        }
        lds_barrier(); // the last fetched panel is consumed: (C) reuses panel0
      }

      // ---------------------------------------------------------------- (C) tile rows a .. b-1
      for (int k = a; k < b; k++) {
        {
          const int tkk = (k - a) * (NT + 1) - (k * (k - 1) - a * (a - 1)) / 2; // tiles of the rows a .. k-1 come first
          if (tkk % NW == wv) {
            const int slot_t = tkk / NW;
            d4 av = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < TPW; s++)
              if (s == slot_t) av = acc[s];
            d4 ev;
            (void)feat::diag_tile_factor_blk(av, ev, st0, lane, nullptr, 0.0, 16);
#pragma unroll
            for (int q = 0; q < 4; q++) st1[cl * 16 + g + 4 * q] = ev[q];
          }
        }
        lds_barrier();
        {
          double ua[4];
#pragma unroll
          for (int u = 0; u < 4; u++) ua[u] = st1[(4 * u + g) * 16 + cl];
#pragma unroll
          for (int s = 0; s < TPW; s++) {
            if (tij[s] >= 0 && TI(s) == k && TJ(s) > k) {
              d4 w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
              for (int u = 0; u < 4; u++) FEAT_MFMA(ua[u], acc[s][u], w);
              acc[s] = w;
              double *pt = panel0 + (size_t)TJ(s) * 256;
#pragma unroll
              for (int q = 0; q < 4; q++) pt[(g + 4 * q) * 16 + cl] = w[q];
              if (TJ(s) >= b) { // a later pass needs it
                double *wt = ws + ((size_t)k * (nt_max + 1) + TJ(s)) * 256;
#pragma unroll
                for (int q = 0; q < 4; q++) wt[(g + 4 * q) * 16 + cl] = w[q];
              }
            }
          }
        }
        lds_barrier();
#pragma unroll
        for (int s = 0; s < TPW; s++) {
          if (tij[s] >= 0 && TI(s) > k) {
            const double *pi = panel0 + (size_t)TI(s) * 256, *pj = panel0 + (size_t)TJ(s) * 256;
            double va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; u++) va[u] = -pi[(4 * u + g) * 16 + cl], vb[u] = pj[(4 * u + g) * 16 + cl];
#pragma unroll
            for (int u = 0; u < 4; u++) FEAT_MFMA(va[u], vb[u], acc[s]);
          }
        }
      }
      // the solved right-hand sides of this pass
#pragma unroll
      for (int s = 0; s < TPW; s++) {
        if (tij[s] >= 0 && TJ(s) == NT && cl < 4) {
#pragma unroll
          for (int q = 0; q < 4; q++) rhs[(size_t)(16 * TI(s) + g + 4 * q) * 4 + cl] = acc[s][q];
        }
      }
      __syncthreads(); // full barrier: the scratch stores have landed (vmcnt) before another wavefront fetches them; LDS is free
#undef TI
#undef TJ
      a = b;
    }

    // ------------------------------------------------------------------ chi2 = |y_r|^2 - g^T G^-1 g,  y_r = U^-T r, Y_b = U^-T H_b
    if (wv == 0) {
      double sa = 0, G00 = 0, G01 = 0, G11 = 0, g0 = 0, g1 = 0;
      for (int j = lane; j < n; j += 64) {
        const double yr = rhs[4 * j], y0 = rhs[4 * j + 1], y1 = rhs[4 * j + 2];
        sa = fma(yr, yr, sa);
        G00 = fma(y0, y0, G00), G01 = fma(y0, y1, G01), G11 = fma(y1, y1, G11);
        g0 = fma(y0, yr, g0), g1 = fma(y1, yr, g1);
      }
      sa = wave_sum(sa);
      double chi2 = sa;
      if (PROJ && single) { // the 2 x 2 G by its Cholesky factor
        G00 = wave_sum(G00), G01 = wave_sum(G01), G11 = wave_sum(G11), g0 = wave_sum(g0), g1 = wave_sum(g1);
        const double l10 = G01 / G00, d1 = G11 - l10 * G01, x1 = g1 - l10 * g0;
        chi2 = sa - (g0 * g0 / G00 + x1 * x1 / d1);
      }
      if (lane == 0) slamy_verdict(p, f, mult_f, single, n, n_out, chi2, reject_slot);
    }
    __syncthreads(); // (the pass loop ended with a full barrier: the rows' stores have landed)
    if (*reject_slot)
      for (int64_t e = tid; e < (int64_t)n_out * LD; e += NTH) out[e] = 0.0;
  }
}
#endif // OVG_TU_FEATY, OVG_TU_SLAMY_BIG

} // namespace slamy
} // namespace ovg
