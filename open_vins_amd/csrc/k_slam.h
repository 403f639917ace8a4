// k_slam.h — the small kernels around the SLAM landmarks that live in the state.
//
//   Landmark::get_xyz / set_from_xyz                   ov_core/src/types/Landmark.cpp:25-141
//   Landmark::update                                    ov_core/src/types/Landmark.h:80-89
//   UpdaterSLAM::update, landmark -> feature            UpdaterSLAM.cpp:333-353
//   StateHelper::initialize_invertible                  StateHelper.cpp:484-577
//
// The landmarks are resident in REPRESENTATION coordinates (what ov_type::Landmark stores): the additive
// correction of the EKF applies to those, the Jacobians need xyz.
#pragma once
#include "device_math.h"
#include "ovgpu_types.h"
#include "k_system.h"

namespace ovg {

// Landmark::get_xyz — Landmark.cpp:25-62 (3-dof representations)
__device__ __forceinline__ V3 lm_to_xyz(int rep, const double *v) {
  if (rep == OVGPU_REP_GLOBAL_FULL_INVERSE_DEPTH || rep == OVGPU_REP_ANCHORED_FULL_INVERSE_DEPTH) {
    const double ir = 1.0 / v[2];
    return V3{ir * cos(v[0]) * sin(v[1]), ir * sin(v[0]) * sin(v[1]), ir * cos(v[1])};
  }
  // ANCHORED_INVERSE_DEPTH_SINGLE is stored as (uv_norm_zero.x, uv_norm_zero.y, rho): only rho is a state variable, the bearing is
  // a constant of the landmark (Landmark.cpp:57-60, :124-140) — the same formulas as the MSCKF inverse depth
  if (rep == OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH || rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) {
    const double ir = 1.0 / v[2];
    return V3{ir * v[0], ir * v[1], ir};
  }
  return V3{v[0], v[1], v[2]};
}

// Landmark::set_from_xyz — Landmark.cpp:66-141
__device__ __forceinline__ void lm_from_xyz(int rep, const V3 &p, double *v) {
  if (rep == OVGPU_REP_GLOBAL_FULL_INVERSE_DEPTH || rep == OVGPU_REP_ANCHORED_FULL_INVERSE_DEPTH) {
    const double rho = 1.0 / norm(p);
    v[0] = atan2(p.y, p.x), v[1] = acos(rho * p.z), v[2] = rho;
    return;
  }
  if (rep == OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH || rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) {
    v[0] = p.x / p.z, v[1] = p.y / p.z, v[2] = 1.0 / p.z;
    return;
  }
  v[0] = p.x, v[1] = p.y, v[2] = p.z;
}

struct LandmarkStore {
  double *value, *fej;    // [3 * cap] representation coordinates
  int32_t *cov, *col;     // [cap] covariance id, first Jacobian column (-1: not in the column map yet)
  int32_t *anchor;        // [cap] packed (camera << 10 | clone) or -1
  int32_t *rep;           // [cap] ovgpu_feat_rep of the landmark (Landmark::_feat_representation; round 5: per landmark)
};
__host__ __device__ inline int lm_rep_dof(int rep) { return rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? 1 : 3; }

// per-feature inputs of the SLAM update from the landmark each feature observes (UpdaterSLAM.cpp:333-353)
// (the representation is the LANDMARK's, UpdaterSLAM.cpp:336-341: landmarks of several representations share one batch)
__global__ void k_slam_gather(int F, const int32_t *__restrict__ lm_index, const int32_t *__restrict__ meas_offsets, LandmarkStore lm,
                              double *p_FinG, double *p_FinA, double *p_fej, int32_t *feat_lm, int32_t *feat_lmcol, int32_t *feat_lmcov,
                              int32_t *feat_anchor, int32_t *status) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int l = lm_index[f];
  const int rep = lm.rep[l];
  const V3 x = lm_to_xyz(rep, lm.value + 3 * l), xf = lm_to_xyz(rep, lm.fej + 3 * l);
  double *dst = rep >= OVGPU_REP_ANCHORED_3D ? p_FinA : p_FinG; // position in the anchor camera / in the global frame
  dst[3 * f] = x.x, dst[3 * f + 1] = x.y, dst[3 * f + 2] = x.z;
  p_fej[3 * f] = xf.x, p_fej[3 * f + 1] = xf.y, p_fej[3 * f + 2] = xf.z;
  feat_lm[f] = l, feat_lmcol[f] = lm.col[l], feat_lmcov[f] = lm.cov[l], feat_anchor[f] = lm.anchor[l];
  // UpdaterSLAM.cpp:289-291; a single-depth landmark needs two measurements: one leaves no row after its bearing is projected out
  const int min_meas = lm_rep_dof(rep) == 1 ? 2 : 1;
  status[f] = (meas_offsets[f + 1] - meas_offsets[f] >= min_meas) ? OVGPU_FEAT_USED : OVGPU_FEAT_TOO_FEW_MEAS;
}

// ovgpu_set_active_landmarks: the column map of the calls that follow, from the resident variables sorted by covariance id (`vars`: covariance
// id, size, kind, index of each) and the landmarks the caller named (`active_idx`).  UpdaterSLAM::update gives columns to the variables its
// batch touches (UpdaterSLAM.cpp:300-340), delayed_init to no resident landmark at all (:147-239): a landmark outside the set keeps column
// -1 and is corrected through its covariance rows alone (k_landmark_update reads dx by covariance id).  Calibration and clones always have
// columns.  ONE wavefront: the set changes with every call and the map is a few hundred entries, so the launch is latency, not work — a
// wave-level inclusive scan of the block widths, 64 variables a step, gives every variable its first column; no LDS traffic and no barrier
// inside the scan loop (the two barriers in front of it separate the set's flags from their readers).
// The walk — which variables get columns, col_sub of a single-depth landmark — is layout_columns' (api_state.inc), kept in step with it by hand.
// Every store is bounded by the capacity the host reserved from its own mirror of the same walk (Dcap, L, C, K).
struct ActiveColsParams {
  int V, L, C, K, n_active, Dcap;
  const int32_t *vars;       // [4 V]
  const int32_t *active_idx; // [n_active], duplicates allowed
  int32_t *clone_col, *calib_col, *intr_col, *lm_col, *col_cov;
  uint8_t *col_kind, *col_sub;
  uint16_t *col_var;
};
__global__ void __launch_bounds__(64) k_active_columns(ActiveColsParams p) {
  extern __shared__ uint8_t act_lm[]; // [L]
  const int lane = threadIdx.x;
  for (int l = lane; l < p.L; l += 64) act_lm[l] = 0, p.lm_col[l] = -1;
  for (int i = lane; i < p.C; i += 64) p.clone_col[i] = -1;
  for (int k = lane; k < p.K; k += 64) p.calib_col[k] = -1, p.intr_col[k] = -1; // (a calibration that is not estimated has no column)
  __syncthreads();
  for (int i = lane; i < p.n_active; i += 64) {
    const int l = p.active_idx[i];
    if (l >= 0 && l < p.L) act_lm[l] = 1; // (a duplicate stores the same byte)
  }
  __syncthreads();
  int base = 0;
  for (int v0 = 0; v0 < p.V; v0 += 64) {
    const int v = v0 + lane;
    int cov = 0, size = 0, kind = COL_CLONE, index = 0, w = 0;
    if (v < p.V) {
      cov = p.vars[4 * v], size = p.vars[4 * v + 1], kind = p.vars[4 * v + 2], index = p.vars[4 * v + 3];
      const bool in_range = kind == COL_LANDMARK ? (index >= 0 && index < p.L) : (index >= 0 && index < (kind == COL_CLONE ? p.C : p.K));
      w = (in_range && (kind != COL_LANDMARK || act_lm[index])) ? size : 0;
    }
    int x = w;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    const int start = base + x - w;
    if (w > 0 && start + w <= p.Dcap) {
      if (kind == COL_CLONE) p.clone_col[index] = start;
      else if (kind == COL_CALIB_POSE) p.calib_col[index] = start;
      else if (kind == COL_CALIB_INTR) p.intr_col[index] = start;
      else p.lm_col[index] = start;
      for (int i = 0; i < w; i++) {
        p.col_cov[start + i] = cov + i, p.col_kind[start + i] = (uint8_t)kind, p.col_var[start + i] = (uint16_t)index;
        p.col_sub[start + i] = (uint8_t)((kind == COL_LANDMARK && size == 1) ? 2 : i); // the depth is column 2 of H_f
      }
    }
    base += __shfl(x, 63, 64);
  }
}

// Landmark::update: value += dx[id .. id+2]     (L from a device counter when the count changes inside a stream of launches)
// state dof of a landmark: 3, or 1 for a single-depth landmark whose state variable is the LAST of its three stored values
__global__ void k_landmark_update(int L, const int32_t *__restrict__ L_dev, const int32_t *__restrict__ lm_rep, const double *__restrict__ dx,
                                  const int32_t *__restrict__ lm_cov, double *lm_value, const int32_t *pred) {
  if (pred && *pred == 0) return;
  const int n = L_dev ? *L_dev : L;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const int l = t / 3, k = t % 3, j0 = 3 - lm_rep_dof(lm_rep[l]);
  if (k >= j0) lm_value[3 * l + k] += dx[lm_cov[l] + k - j0];
}

// dst (n x n, leading dimension ldd) <- src (leading dimension lds); the rest of dst's rows / columns up to nd is zeroed
__global__ void k_cov_copy(int n, int nd, const double *__restrict__ src, int lds, double *__restrict__ dst, int ldd) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i < nd && j < nd) dst[(size_t)i * ldd + j] = (i < n && j < n) ? src[(size_t)i * lds + j] : 0.0;
}

// ---------------------------------------------------------------------------------------------------
// window bookkeeping on the resident covariance (pure data movement: one thread per element)
// ---------------------------------------------------------------------------------------------------
// StateHelper::marginalize (StateHelper.cpp:271-339): dst = src without rows / columns [id, id + size).  The lower-left block is
// the transpose of the upper-right one, as in the reference (:303-304).
// StateHelper::get_marginal_covariance (StateHelper.cpp:226-258): out[i][j] = P[idx[i]][idx[j]]
__global__ void k_cov_gather(int N, int n, const int32_t *__restrict__ idx, const double *__restrict__ P, double *__restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n * n) out[t] = P[(size_t)idx[t / n] * N + idx[t % n]];
}

__global__ void k_cov_remove(int N, int id, int size, const double *__restrict__ src, double *__restrict__ dst) {
  const int Nn = N - size;
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= Nn || j >= Nn) return;
  int si = i < id ? i : i + size, sj = j < id ? j : j + size;
  if (i >= id && j < id) { // P(x2, x1) := P(x1, x2)^T
    const int t = si;
    si = sj, sj = t;
  }
  dst[(size_t)i * Nn + j] = src[(size_t)si * N + sj];
}

// ---------------------------------------------------------------------------------------------------
// ovgpu_state_marginalize_batched: n blocks leave in ONE pass (three launches whatever n is).  Marginalisation only SELECTS rows and
// columns of P, so the joint removal needs no order: k_marg_plan turns the block list into index lists, k_cov_remove_many gathers the
// covariance through them, k_records_compact the resident clone / landmark records.
// ---------------------------------------------------------------------------------------------------
// One integer table on the device.  The host fills blk / clone_keep / lm_keep (its checks ran before: blocks sorted by id, disjoint, inside
// [0, N)); k_marg_plan writes the rest.  Every list it writes has room for the UNCOMPACTED count, so no store depends on the flags' sum.
struct MargPlan {
  int N, C, L, n;
  const int32_t *blk;        // [2 n] (id, size), ascending ids
  const int32_t *clone_keep; // [C] 1: the clone stays
  const int32_t *lm_keep;    // [L]
  int32_t *keep;             // [N] old row / column of every new one
  int32_t *clone_src;        // [C] old index of every new clone
  int32_t *clone_new;        // [C] new index of every old clone, -1: it left
  int32_t *lm_src;           // [L] old index of every new landmark
};

// stream compaction by ONE wavefront, 64 flags a step: the ballot's bits below a lane are its exclusive prefix sum (no LDS, no barrier)
template <class Flag>
__device__ __forceinline__ void wave_compact(int lane, int count, Flag flag, int32_t *src_of_new, int32_t *new_of_old) {
  int run = 0;
  for (int i0 = 0; i0 < count; i0 += 64) {
    const int i = i0 + lane;
    const bool f = i < count && flag(i);
    const unsigned long long m = __ballot(f);
    const int pos = run + __popcll(m & ((1ull << lane) - 1ull));
    if (f) src_of_new[pos] = i; // pos <= i < count
    if (new_of_old && i < count) new_of_old[i] = f ? pos : -1;
    run += __popcll(m);
  }
}

__global__ void __launch_bounds__(64) k_marg_plan(MargPlan p) {
  const int lane = threadIdx.x;
  // a row stays when no block holds it: the last block that starts at or before it (binary search over the sorted list) ends before it
  wave_compact(lane, p.N, [&](int i) {
    int lo = 0, hi = p.n; // blocks [0, lo) start at or before i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.blk[2 * mid] <= i) lo = mid + 1;
      else hi = mid;
    }
    return lo == 0 || p.blk[2 * (lo - 1)] + p.blk[2 * (lo - 1) + 1] <= i;
  }, p.keep, nullptr);
  wave_compact(lane, p.C, [&](int i) { return p.clone_keep[i] != 0; }, p.clone_src, p.clone_new);
  wave_compact(lane, p.L, [&](int i) { return p.lm_keep[i] != 0; }, p.lm_src, nullptr);
}

// P'[i][j] = P[keep[i]][keep[j]]: one output row per grid row, consecutive lanes on consecutive j — the write is one contiguous row, the read
// the runs of the source row between the removed blocks.  A copy: no arithmetic touches a value.
__global__ void __launch_bounds__(256) k_cov_remove_many(int N, int Nn, const int32_t *__restrict__ keep, const double *__restrict__ src,
                                                         double *__restrict__ dst) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= Nn || j >= Nn) return;
  dst[(size_t)i * Nn + j] = src[(size_t)keep[i] * N + keep[j]];
}

// every resident record array through the index lists into its second buffer, in one launch: clone_qp / clone_fej (7 doubles a clone),
// lm_val / lm_fej (3 doubles a landmark), lm_anchor / lm_rep (one int).  An anchor names its clone by INDEX: it is rewritten to the
// clone's new one (the host has checked that no surviving landmark is anchored in a clone that leaves).
struct RecordsCompact {
  int Cn, Ln; // clones / landmarks that stay
  const int32_t *clone_src, *clone_new, *lm_src;
  const double *clone_qp, *clone_fej, *lm_val, *lm_fej;
  const int32_t *lm_anchor, *lm_rep;
  double *clone_qp_out, *clone_fej_out, *lm_val_out, *lm_fej_out;
  int32_t *lm_anchor_out, *lm_rep_out;
};
__global__ void __launch_bounds__(256) k_records_compact(RecordsCompact p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 7 * p.Cn) {
    const size_t s = (size_t)7 * p.clone_src[t / 7] + t % 7;
    p.clone_qp_out[t] = p.clone_qp[s], p.clone_fej_out[t] = p.clone_fej[s];
  }
  if (t < 3 * p.Ln) {
    const size_t s = (size_t)3 * p.lm_src[t / 3] + t % 3;
    p.lm_val_out[t] = p.lm_val[s], p.lm_fej_out[t] = p.lm_fej[s];
  }
  if (t < p.Ln) {
    const int s = p.lm_src[t];
    int32_t a = p.lm_anchor[s];
    if (a >= 0) {
      const int32_t cl = p.clone_new[a & 1023];
      a = cl >= 0 ? ((a >> 10) << 10) | cl : -1;
    }
    p.lm_anchor_out[t] = a, p.lm_rep_out[t] = p.lm_rep[s];
  }
}

// StateHelper::clone (StateHelper.cpp:341-391): rows / columns [nid, nid + n) := those of [sid, sid + n); P has leading dimension N
__global__ void k_cov_clone(int N, int n_old, int sid, int nid, int n, double *P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x; // index over the OLD rows, or n_old .. n_old + n*n - 1 for the corner
  if (i < n_old) {
    for (int a = 0; a < n; a++) {
      P[(size_t)i * N + nid + a] = P[(size_t)i * N + sid + a];
      P[(size_t)(nid + a) * N + i] = P[(size_t)(sid + a) * N + i];
    }
  } else if (i < n_old + n * n) {
    const int a = (i - n_old) / n, b = (i - n_old) % n;
    P[(size_t)(nid + a) * N + nid + b] = P[(size_t)(sid + a) * N + sid + b];
  }
}

// StateHelper::augment_clone, time-offset Jacobian (StateHelper.cpp:607-610), the two statements in the reference's order:
// pass 0: P(:, nid + j) += P(:, dt) dnc[j];   pass 1: P(nid + i, :) += dnc[i] P(dt, :)
__global__ void k_cov_dt(int N, int nid, int dt, const double *__restrict__ dnc, double *P, int pass) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N) return;
  if (pass == 0) {
    const double pd = P[(size_t)t * N + dt];
    for (int j = 0; j < 6; j++) P[(size_t)t * N + nid + j] += pd * dnc[j];
  } else {
    const double pd = P[(size_t)dt * N + t];
    for (int i = 0; i < 6; i++) P[(size_t)(nid + i) * N + t] += dnc[i] * pd;
  }
}

// StateHelper::EKFPropagation (StateHelper.cpp:36-114)
//   pass 0: W[i][a]   = sum_k P[i][old_k] Phi[a][k]                        (Cov_PhiT, :77-82)
//   pass 1: PCP[a][b] = Qsym[a][b] + sum_k Phi[a][k] W[old_k][b]           (:85-90)
//   pass 2: P(new, :) = W^T, P(:, new) = W, P(new, new) = PCP, a negative entry anywhere on the diagonal -> flags[1]   (:93-113)
__global__ void k_cov_propagate(int N, int nid, int n_new, int n_old, const int32_t *__restrict__ old_ids, const double *__restrict__ Phi,
                                const double *__restrict__ Q, double *P, double *W, double *PCP, int32_t *flags, int pass) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (pass == 0) {
    if (t >= N * n_new) return;
    const int i = t / n_new, a = t % n_new;
    double s = 0.0;
    for (int k = 0; k < n_old; k++) s = fma(P[(size_t)i * N + old_ids[k]], Phi[(size_t)a * n_old + k], s);
    W[t] = s;
  } else if (pass == 1) {
    if (t >= n_new * n_new) return;
    const int a = t / n_new, b = t % n_new;
    double s = a <= b ? Q[(size_t)a * n_new + b] : Q[(size_t)b * n_new + a]; // Q.selfadjointView<Upper>()
    for (int k = 0; k < n_old; k++) s = fma(Phi[(size_t)a * n_old + k], W[(size_t)old_ids[k] * n_new + b], s);
    PCP[t] = s;
  } else {
    if (t >= N * n_new) return;
    const int i = t / n_new, a = t % n_new;
    if (i >= nid && i < nid + n_new) {
      const double v = PCP[(size_t)(i - nid) * n_new + a];
      P[(size_t)i * N + nid + a] = v;
      if (i - nid == a && v < 0.0) flags[1] = 1;
    } else {
      const double v = W[t];
      P[(size_t)i * N + nid + a] = v;
      P[(size_t)(nid + a) * N + i] = v;
      // the reference scans the WHOLE diagonal (:101-113): a row outside the block keeps its diagonal entry (no thread of this pass writes it)
      if (a == 0 && P[(size_t)i * N + i] < 0.0) flags[1] = 1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// UpdaterSLAM::perform_anchor_change (UpdaterSLAM.cpp:506-647) for one anchored 3-dof landmark: the transition matrix of
// the landmark's error state into the new anchor frame, Phi = H_f_new^-1 [H_x_old | H_f_old | -H_x_new], goes to `phi`
// (3 x n_old, row-major) with the covariance index of every column in `ids`; the landmark's value / fej / anchor are
// rewritten.  The covariance itself is then propagated by k_cov_propagate (StateHelper::EKFPropagation, Q = 0).
// Column order: old anchor clone (6), old anchor camera extrinsics (6, if estimated), new anchor clone (6), new anchor
// camera extrinsics (6, if estimated and another camera), landmark (3) — the reference's phi_order_OLD (:592-610).
// One thread.
// ---------------------------------------------------------------------------------------------------
struct AnchorParams {
  int rep, do_fej, l, new_cam, new_clone;
  int sz; // landmark dof: 3, or 1 (single depth: H_f is the third column of the inverse-depth Jacobian, UpdaterHelper.cpp:178-189)
  const double *tab_clone, *tab_cam; // [C*24], [K*12]
  const int32_t *clone_cov, *calib_cov;
  LandmarkStore lm;
  double *phi;   // [3 * 27]
  int32_t *ids;  // [27]
  int32_t *n_old; // [1]
};

__global__ void k_anchor_change(AnchorParams p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int l = p.l;
  const int old_cam = p.lm.anchor[l] >> 10, old_clone = p.lm.anchor[l] & 1023;
  // Landmark::get_xyz(true) ignores its flag for ANCHORED_MSCKF_INVERSE_DEPTH and the single depth (Landmark.cpp:47-59 read value() /
  // uv_norm_zero in both cases): for these two the "first estimate" that moves to the new anchor is the CURRENT estimate
  const bool fej_reads_value = p.rep == OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH || p.rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
  const V3 pA_old = lm_to_xyz(p.rep, p.lm.value + 3 * l), pA_old_fej = lm_to_xyz(p.rep, (fej_reads_value ? p.lm.value : p.lm.fej) + 3 * l);
  double Hf_old[9], Ha_old[18], Hc_old[18], Hf_new[9], Ha_new[18], Hc_new[18];
  // the single-depth landmark uses the Jacobians of the MSCKF inverse depth (its third column is d p / d rho)
  const int jrep = p.rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : p.rep;
  anchored_rep_jacobian(jrep, p.do_fej, p.tab_cam + 12 * old_cam, p.tab_clone + 24 * old_clone, pA_old, Hf_old, Ha_old, Hc_old); // :523-526
  // current estimates (:536-551) and first estimates (:556-571) of the two anchor cameras
  V3 pA_new, pA_new_fej;
  for (int fej = 0; fej < 2; fej++) {
    const int o = fej ? 12 : 0;
    const M3 R_GtoOLD = mul(load_m3(p.tab_cam + 12 * old_cam), load_m3(p.tab_clone + 24 * old_clone + o));
    const V3 p_OLDinG = load_v3(p.tab_clone + 24 * old_clone + o + 9) - mulT(R_GtoOLD, load_v3(p.tab_cam + 12 * old_cam + 9));
    const M3 R_GtoNEW = mul(load_m3(p.tab_cam + 12 * p.new_cam), load_m3(p.tab_clone + 24 * p.new_clone + o));
    const V3 p_NEWinG = load_v3(p.tab_clone + 24 * p.new_clone + o + 9) - mulT(R_GtoNEW, load_v3(p.tab_cam + 12 * p.new_cam + 9));
    const M3 R_OLDtoNEW = mul(R_GtoNEW, transpose(R_GtoOLD));
    const V3 p_OLDinNEW = mul(R_GtoNEW, p_OLDinG - p_NEWinG);
    const V3 r = mul(R_OLDtoNEW, fej ? pA_old_fej : pA_old) + p_OLDinNEW;
    if (fej) pA_new_fej = r;
    else pA_new = r;
  }
  anchored_rep_jacobian(jrep, p.do_fej, p.tab_cam + 12 * p.new_cam, p.tab_clone + 24 * p.new_clone, pA_new, Hf_new, Ha_new, Hc_new); // :577-580
  // H_f_new^-1 by column-pivoted Householder QR of the 3 x 3 (:621); single depth: the pseudo-inverse h^T / |h|^2 of the 3 x 1 (:619)
  double inv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int j0 = 3 - p.sz; // rows of `inv` / columns of H_f that belong to the landmark's state
  if (p.sz == 3) {
    const M3 A{Hf_new[0], Hf_new[1], Hf_new[2], Hf_new[3], Hf_new[4], Hf_new[5], Hf_new[6], Hf_new[7], Hf_new[8]};
    const V3 c0 = colpiv_qr_solve3(A, V3{1, 0, 0}), c1 = colpiv_qr_solve3(A, V3{0, 1, 0}), c2 = colpiv_qr_solve3(A, V3{0, 0, 1});
    inv[0] = c0.x, inv[1] = c1.x, inv[2] = c2.x, inv[3] = c0.y, inv[4] = c1.y, inv[5] = c2.y, inv[6] = c0.z, inv[7] = c1.z, inv[8] = c2.z;
  } else {
    const double h0 = Hf_new[2], h1 = Hf_new[5], h2 = Hf_new[8], nn = 1.0 / (h0 * h0 + h1 * h1 + h2 * h2);
    inv[6] = nn * h0, inv[7] = nn * h1, inv[8] = nn * h2;
  }
  // ---- column layout
  int n = 0, col_oc, col_ok = -1, col_nc, col_nk = -1, col_lm;
  col_oc = n, n += 6;
  if (p.calib_cov[old_cam] >= 0) col_ok = n, n += 6;
  col_nc = n, n += 6;
  if (p.calib_cov[p.new_cam] >= 0) {
    if (p.new_cam == old_cam) col_nk = col_ok;
    else col_nk = n, n += 6;
  }
  col_lm = n, n += p.sz;
  for (int i = 0; i < p.sz * n; i++) p.phi[i] = 0.0;
  for (int j = 0; j < 6; j++) {
    p.ids[col_oc + j] = p.clone_cov[old_clone] + j, p.ids[col_nc + j] = p.clone_cov[p.new_clone] + j;
    if (col_ok >= 0) p.ids[col_ok + j] = p.calib_cov[old_cam] + j;
    if (col_nk >= 0) p.ids[col_nk + j] = p.calib_cov[p.new_cam] + j;
  }
  for (int j = 0; j < p.sz; j++) p.ids[col_lm + j] = p.lm.cov[l] + j;
  auto add_block = [&](int col, const double *H, int w, int b0, double sign) { // Phi(:, col ..) += sign * inv * H(:, b0 ..) (H is 3 x w)
    for (int a = j0; a < 3; a++)
      for (int b = b0; b < w; b++) {
        double sv = 0.0;
        for (int k = 0; k < 3; k++) sv = fma(inv[3 * a + k], H[w * k + b], sv);
        p.phi[(a - j0) * n + col + b - b0] += sign * sv;
      }
  };
  add_block(col_oc, Ha_old, 6, 0, 1.0);                  // :626-628
  if (col_ok >= 0) add_block(col_ok, Hc_old, 6, 0, 1.0);
  add_block(col_lm, Hf_old, 3, j0, 1.0);                 // :631 (single depth: H_f_old is the third column)
  add_block(col_nc, Ha_new, 6, 0, -1.0);                 // :634-636
  if (col_nk >= 0) add_block(col_nk, Hc_new, 6, 0, -1.0);
  *p.n_old = n;
  // ---- the landmark in its new anchor (:642-647)
  lm_from_xyz(p.rep, pA_new, p.lm.value + 3 * l);
  lm_from_xyz(p.rep, pA_new_fej, p.lm.fej + 3 * l);
  p.lm.anchor[l] = (p.new_cam << 10) | p.new_clone;
}

// ---------------------------------------------------------------------------------------------------
// UpdaterSLAM::change_anchors (UpdaterSLAM.cpp:481-504) for EVERY landmark that moves, in one launch: workgroup b (one wavefront) does for
// entry b of `tab` what k_anchor_change does for its landmark.  Phi is built from state VALUES alone (clone poses, extrinsics, the landmark's
// own value / first estimate) and an anchor change moves no clone and no calibration, so all of them can be formed at the entry state; the
// covariance follows in k_cov_propagate_multi.
// tab, 8 ints per entry: landmark, new camera, new clone, dof (3 / 1), n_old, first element of its Phi (dof x n_old, row-major) in `phi`,
// first of its n_old covariance ids in `ids`, the landmark's own covariance id (k_cov_propagate_multi).  The offsets are the host's prefix
// sums; n_old is the host's count of the same column walk (phi_order_OLD, :592-610) the kernel does.
// The lanes: the two Jacobian triples are the same few hundred flops for every lane (one lane's time); lane 0 parks them in LDS.  The three
// columns of H_f_new^-1 are three independent solves, lanes 0..2; the dof x n_old entries of Phi (3 x 3 by 3 x 6 / 3 x 3 products, one dot
// product of length 3 each) and the n_old ids go one per lane.  Entry for entry the arithmetic is k_anchor_change's.
// rewrite != 0: the resident landmark gets its new value / first estimate / anchor (mode B); 0: the store is only read (mode A export).
// ---------------------------------------------------------------------------------------------------
struct AnchorAllParams {
  int n, do_fej, rewrite;
  const int32_t *tab;                // [8 n]
  const double *tab_clone, *tab_cam; // [C*24], [K*12]
  const int32_t *clone_cov, *calib_cov;
  LandmarkStore lm;
  double *phi;       // the Phi of every entry, ragged
  int32_t *ids;      // the covariance ids of every entry's columns, ragged
  double *val, *fej; // [3 n] the landmarks in their new anchors
};

__global__ void __launch_bounds__(64) k_anchor_change_all(AnchorAllParams p) {
  __shared__ double sH[6][18]; // Ha_old, Hc_old, Ha_new, Hc_new (3 x 6), Hf_old, Hf_new (3 x 3)
  __shared__ double sInv[9];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= p.n) return;
  const int32_t *e = p.tab + 8 * b;
  const int l = e[0], new_cam = e[1], new_clone = e[2], sz = e[3], n_old = e[4];
  const int rep = p.lm.rep[l];
  const int old_cam = p.lm.anchor[l] >> 10, old_clone = p.lm.anchor[l] & 1023;
  // the "first estimate" of ANCHORED_MSCKF_INVERSE_DEPTH and of the single depth reads the current value (k_anchor_change; Landmark.cpp:47-59)
  const bool fej_reads_value = rep == OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH || rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
  const V3 pA_old = lm_to_xyz(rep, p.lm.value + 3 * l), pA_old_fej = lm_to_xyz(rep, (fej_reads_value ? p.lm.value : p.lm.fej) + 3 * l);
  double Hf_old[9], Ha_old[18], Hc_old[18], Hf_new[9], Ha_new[18], Hc_new[18];
  const int jrep = rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : rep;
  anchored_rep_jacobian(jrep, p.do_fej, p.tab_cam + 12 * old_cam, p.tab_clone + 24 * old_clone, pA_old, Hf_old, Ha_old, Hc_old); // :523-526
  V3 pA_new, pA_new_fej;
  for (int fej = 0; fej < 2; fej++) { // :536-551, :556-571
    const int o = fej ? 12 : 0;
    const M3 R_GtoOLD = mul(load_m3(p.tab_cam + 12 * old_cam), load_m3(p.tab_clone + 24 * old_clone + o));
    const V3 p_OLDinG = load_v3(p.tab_clone + 24 * old_clone + o + 9) - mulT(R_GtoOLD, load_v3(p.tab_cam + 12 * old_cam + 9));
    const M3 R_GtoNEW = mul(load_m3(p.tab_cam + 12 * new_cam), load_m3(p.tab_clone + 24 * new_clone + o));
    const V3 p_NEWinG = load_v3(p.tab_clone + 24 * new_clone + o + 9) - mulT(R_GtoNEW, load_v3(p.tab_cam + 12 * new_cam + 9));
    const M3 R_OLDtoNEW = mul(R_GtoNEW, transpose(R_GtoOLD));
    const V3 p_OLDinNEW = mul(R_GtoNEW, p_OLDinG - p_NEWinG);
    const V3 r = mul(R_OLDtoNEW, fej ? pA_old_fej : pA_old) + p_OLDinNEW;
    if (fej) pA_new_fej = r;
    else pA_new = r;
  }
  anchored_rep_jacobian(jrep, p.do_fej, p.tab_cam + 12 * new_cam, p.tab_clone + 24 * new_clone, pA_new, Hf_new, Ha_new, Hc_new); // :577-580
  const int j0 = 3 - sz; // rows of the inverse / columns of H_f that belong to the landmark's state
  // H_f_new^-1 (:621): column `lane` of the inverse is the solve for the unit vector e_lane; single depth: the pseudo-inverse of the 3 x 1 (:619)
  {
    const M3 A{Hf_new[0], Hf_new[1], Hf_new[2], Hf_new[3], Hf_new[4], Hf_new[5], Hf_new[6], Hf_new[7], Hf_new[8]};
    const int j = lane % 3;
    const V3 cj = colpiv_qr_solve3(A, V3{j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0});
    if (lane < 3) {
      if (sz == 3) {
        sInv[lane] = cj.x, sInv[3 + lane] = cj.y, sInv[6 + lane] = cj.z;
      } else {
        const double h0 = Hf_new[2], h1 = Hf_new[5], h2 = Hf_new[8], nn = 1.0 / (h0 * h0 + h1 * h1 + h2 * h2);
        sInv[lane] = 0.0, sInv[3 + lane] = 0.0, sInv[6 + lane] = nn * (lane == 0 ? h0 : lane == 1 ? h1 : h2);
      }
    }
  }
  if (lane == 0) {
    for (int i = 0; i < 18; i++) sH[0][i] = Ha_old[i], sH[1][i] = Hc_old[i], sH[2][i] = Ha_new[i], sH[3][i] = Hc_new[i];
    for (int i = 0; i < 9; i++) sH[4][i] = Hf_old[i], sH[5][i] = Hf_new[i];
  }
  __syncthreads(); // (also: every lane has read the landmark before lane 0 rewrites it below)
  // ---- column layout (phi_order_OLD)
  int n = 6, col_ok = -1, col_nc, col_nk = -1, col_lm; // the old anchor clone has columns 0 .. 5
  if (p.calib_cov[old_cam] >= 0) col_ok = n, n += 6;
  col_nc = n, n += 6;
  if (p.calib_cov[new_cam] >= 0) {
    if (new_cam == old_cam) col_nk = col_ok;
    else col_nk = n, n += 6;
  }
  col_lm = n, n += sz;
  if (n != n_old) return; // the host counted another layout: nothing is written (it cannot happen while the host mirrors of the ids hold)
  int32_t *ids = p.ids + e[6];
  for (int j = lane; j < n; j += 64) {
    int id;
    if (j >= col_lm) id = p.lm.cov[l] + j - col_lm;
    else if (col_nk >= 0 && col_nk != col_ok && j >= col_nk) id = p.calib_cov[new_cam] + j - col_nk;
    else if (j >= col_nc) id = p.clone_cov[new_clone] + j - col_nc;
    else if (col_ok >= 0 && j >= col_ok) id = p.calib_cov[old_cam] + j - col_ok;
    else id = p.clone_cov[old_clone] + j;
    ids[j] = id;
  }
  // Phi(a, col) = sum over the blocks that own the column of sign * (inv H)(a, .), accumulated in k_anchor_change's order
  auto prod = [&](int a, const double *H, int w, int bcol) {
    double sv = 0.0;
    for (int k = 0; k < 3; k++) sv = fma(sInv[3 * (a + j0) + k], H[w * k + bcol], sv);
    return sv;
  };
  double *phi = p.phi + e[5];
  for (int t = lane; t < sz * n; t += 64) {
    const int a = t / n, j = t - a * n;
    double v = 0.0;
    if (j < 6) v += prod(a, sH[0], 6, j);                                                  // :626-628
    if (col_ok >= 0 && j >= col_ok && j < col_ok + 6) v += prod(a, sH[1], 6, j - col_ok);
    if (j >= col_lm) v += prod(a, sH[4], 3, j - col_lm + j0);                              // :631
    if (j >= col_nc && j < col_nc + 6) v += -1.0 * prod(a, sH[2], 6, j - col_nc);          // :634-636
    if (col_nk >= 0 && j >= col_nk && j < col_nk + 6) v += -1.0 * prod(a, sH[3], 6, j - col_nk);
    phi[t] = v;
  }
  // ---- the landmark in its new anchor (:642-647)
  if (lane == 0) {
    double v[3], vf[3];
    lm_from_xyz(rep, pA_new, v);
    lm_from_xyz(rep, pA_new_fej, vf);
    for (int i = 0; i < 3; i++) p.val[3 * b + i] = v[i], p.fej[3 * b + i] = vf[i];
    if (p.rewrite) {
      for (int i = 0; i < 3; i++) p.lm.value[3 * l + i] = v[i], p.lm.fej[3 * l + i] = vf[i];
      p.lm.anchor[l] = (new_cam << 10) | new_clone;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The joint StateHelper::EKFPropagation (StateHelper.cpp:36-114, Q = 0) of n anchor changes in THREE launches whatever n is.  No Phi_l has a
// column in another moving landmark, so the reference's sequence of propagations is one propagation whose transition matrix has the block
// rows Phi_l.  S = sum of the landmarks' dof; gmap[g] = (entry << 2 | row) of joint row g; rowg[i] = the joint row of covariance row i, -1 if
// i belongs to no moving landmark.  Kernel boundaries are the only ordering: pass 0 reads P, pass 1 reads W, pass 2 alone writes P.
//   pass 0: W[i][g]  = sum_k P[i][old_l[k]] Phi_l[a][k]              every row i < N, every joint row g = (l, a)    (k_cov_propagate's pass 0)
//   pass 1: G[g][h]  = sum_k Phi_l[a][k] W[old_l[k]][h]              g <= h, stored at [g][h] and [h][g]: Phi_l P(old_l, old_m) Phi_m^T
//   pass 2: P(i, new_g) = P(new_g, i) = W[i][g] for the rows of no moving landmark, P(new_g, new_h) = G[g][h]; negative diagonal -> flags[1]
// Every element of P' that has a mirror image gets the same value as it: P' is exactly symmetric.
// ---------------------------------------------------------------------------------------------------
struct PropMultiParams {
  int N, S;
  const int32_t *tab, *gmap, *rowg; // [8 n], [S], [N]
  const int32_t *ids;
  const double *phi;
  double *P, *W, *G; // [N * N], [N * S], [S * S]
  int32_t *flags;
};

__global__ void __launch_bounds__(256) k_cov_propagate_multi(PropMultiParams p, int pass) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = p.N, S = p.S;
  if (pass == 0) {
    if (t >= N * S) return;
    const int i = t / S, g = t - i * S;
    const int32_t *e = p.tab + 8 * (p.gmap[g] >> 2);
    const int a = p.gmap[g] & 3, n_old = e[4];
    const int32_t *ids = p.ids + e[6];
    const double *phi = p.phi + e[5] + (size_t)a * n_old;
    double s = 0.0;
    for (int k = 0; k < n_old; k++) s = fma(p.P[(size_t)i * N + ids[k]], phi[k], s);
    p.W[t] = s;
  } else if (pass == 1) {
    if (t >= S * S) return;
    const int g = t / S, h = t - g * S;
    if (g > h) return;
    const int32_t *e = p.tab + 8 * (p.gmap[g] >> 2);
    const int a = p.gmap[g] & 3, n_old = e[4];
    const int32_t *ids = p.ids + e[6];
    const double *phi = p.phi + e[5] + (size_t)a * n_old;
    double s = 0.0;
    for (int k = 0; k < n_old; k++) s = fma(phi[k], p.W[(size_t)ids[k] * S + h], s);
    p.G[(size_t)g * S + h] = s;
    p.G[(size_t)h * S + g] = s;
  } else {
    if (t >= N * S) return;
    const int i = t / S, g = t - i * S;
    const int32_t *e = p.tab + 8 * (p.gmap[g] >> 2);
    const int col = e[7] + (p.gmap[g] & 3); // covariance id of joint row g
    const int gi = p.rowg[i];
    if (gi >= 0) {
      const double v = p.G[(size_t)gi * S + g];
      p.P[(size_t)i * N + col] = v;
      if (gi == g && v < 0.0) p.flags[1] = 1;
    } else {
      const double v = p.W[t];
      p.P[(size_t)i * N + col] = v;
      p.P[(size_t)col * N + i] = v;
    }
  }
}

// ovgpu_slam_init_systems: feature f's system as StateHelper::initialize takes it (StateHelper.cpp:393-481), copied out of the
// separated form the chain has just built, before k_init_invertible / the EKF run: the three rows Q1^T [H_x | res] with H_f = R1
// (init_out) on top of the 2m - 3 projected rows Q2^T [H_x | res] with H_f = 0 (the feature's rows of the stack).  A single-depth
// feature keeps the third row only (its H_f = R1(2, 2)): 1 + 2m - 3 = 2m - 2 rows, the bearing projected out (UpdaterSLAM.cpp:181-196).
// H_x is compacted to the feature's Hx_order (cols: the context's column of each of its h columns); the per-feature noise scaling of the
// stack (sigma / sigma_f, k_system.h) is undone, so that R = sigma_f^2 I.  One thread per element of H_x, rows x h, row-major: the stores
// are consecutive, the loads one row of the source per h threads.
struct InitExportParams {
  int LD, D, h, rows, single, f;
  const double *init_out;    // [3 * LD + 9]
  const double *stack;       // the feature's first row of the stack, stride LD (rows - 3 + 2 single of them)
  const int32_t *cols;       // [h]
  const double *feat_sigma;  // [F] or nullptr
  double sigma;              // the context's sigma_pix
  double *Hx, *Hf, *res;     // [rows * h], [rows * (single ? 1 : 3)], [rows]
};

__global__ void __launch_bounds__(256) k_init_export(InitExportParams p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int top = p.single ? 1 : 3; // rows taken from init_out
  const double scale = p.feat_sigma ? p.feat_sigma[p.f] / p.sigma : 1.0;
  auto src_row = [&](int r) -> const double * { return r < top ? p.init_out + (size_t)(r + 3 - top) * p.LD : p.stack + (size_t)(r - top) * p.LD; };
  if (t < p.rows * p.h) {
    const int r = t / p.h, j = t - r * p.h;
    p.Hx[t] = scale * src_row(r)[p.cols[j]];
  }
  if (t < p.rows) p.res[t] = scale * src_row(t)[p.D];
  const int cf = p.single ? 1 : 3;
  if (t < p.rows * cf) {
    const int r = t / cf, j = t - r * cf;
    const double *R1 = p.init_out + (size_t)3 * p.LD; // upper triangular, row-major
    p.Hf[t] = r < top ? scale * R1[3 * (r + 3 - top) + j + 3 - cf] : 0.0;
  }
}

struct InitParams {
  int N, D, LD;             // N = leading dimension of P (the padded capacity)
  int rep, f;
  int sz;                   // dof of the new landmark: 3, or 1 (single depth: only the third row of the 3-row system initialises it)
  const int32_t *col_cov;   // [D]
  const double *init_out;   // [3 * LD + 9]: Q1^T [H_x | res], R1
  double *P;
  double sigma2;
  int32_t *ctr;             // [0] current covariance dimension, [1] current landmark count, [2] this feature passed the gate
  const double *p_FinG, *p_FinA;
  const uint16_t *meas_cc;
  const int32_t *anchor_meas;
  LandmarkStore lm;
  int32_t *feat_slot;       // [F] landmark slot given to feature f, -1 if not initialised
};

// StateHelper::initialize_invertible (StateHelper.cpp:484-577) for one 3-dof landmark.  One workgroup.
//   G = H_L^-1 H_R (3 x D),  new columns of P = -P(:, cols) G^T,  P_LL = G P_small G^T + sigma^2 H_L^-1 H_L^-T,
//   landmark value += H_L^-1 res.
__global__ void __launch_bounds__(256) k_init_invertible(InitParams p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, N = p.N, D = p.D, LD = p.LD;
  if (p.ctr[2] == 0) {
    if (tid == 0) p.feat_slot[p.f] = -1;
    return;
  }
  double *G = sm;          // [3][LD]
  double *t = G + 3 * LD;  // [3][N]
  double *PLL = t + 3 * N; // [9]
  const double *top = p.init_out, *R1 = p.init_out + (size_t)3 * LD;
  // H_L^-1 of the upper-triangular 3 x 3 (StateHelper.cpp:548)
  const double u00 = R1[0], u01 = R1[1], u02 = R1[2], u11 = R1[4], u12 = R1[5], u22 = R1[8];
  const double i00 = 1.0 / u00, i11 = 1.0 / u11, i22 = 1.0 / u22;
  const double i01 = -u01 * i00 * i11, i12 = -u12 * i11 * i22, i02 = (u01 * u12 - u02 * u11) * i00 * i11 * i22;
  for (int c = tid; c < LD; c += 256) {
    const double a = top[c], b = top[LD + c], d = top[2 * LD + c];
    G[c] = i00 * a + i01 * b + i02 * d;
    G[LD + c] = i11 * b + i12 * d;
    G[2 * LD + c] = i22 * d;
  }
  __syncthreads();
  for (int i = tid; i < N; i += 256) { // t = G P(cols, :)
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int c = 0; c < D; c++) {
      const double pv = p.P[(size_t)p.col_cov[c] * N + i];
      t0 = fma(G[c], pv, t0), t1 = fma(G[LD + c], pv, t1), t2 = fma(G[2 * LD + c], pv, t2);
    }
    t[i] = t0, t[N + i] = t1, t[2 * N + i] = t2;
  }
  __syncthreads();
  if (tid < 9) {
    const int j = tid / 3, k = tid % 3;
    double s = 0.0;
    for (int c = 0; c < D; c++) s = fma(t[(size_t)j * N + p.col_cov[c]], G[(size_t)k * LD + c], s);
    // sigma^2 H_L^-1 H_L^-T (:549, R = sigma^2 I)
    const double inv[3][3] = {{i00, i01, i02}, {0.0, i11, i12}, {0.0, 0.0, i22}};
    double w = 0.0;
    for (int q = 0; q < 3; q++) w = fma(inv[j][q], inv[k][q], w);
    PLL[tid] = fma(p.sigma2, w, s);
  }
  __syncthreads();
  const int id = p.ctr[0], slot = p.ctr[1];
  const int j0 = 3 - p.sz; // first row of the initialising system that belongs to the new variable
  for (int i = tid; i < N; i += 256) {
    if (i >= id && i < id + p.sz) continue;
    for (int j = j0; j < 3; j++) { // :556-557
      const double v = -t[(size_t)j * N + i];
      p.P[(size_t)i * N + id + j - j0] = v;
      p.P[(size_t)(id + j - j0) * N + i] = v;
    }
  }
  if (tid < 9) {
    const int j = tid / 3, k = tid % 3;
    if (j >= j0 && k >= j0) p.P[(size_t)(id + j - j0) * N + id + k - j0] = 0.5 * (PLL[3 * j + k] + PLL[3 * k + j]); // :558, symmetric by construction up to rounding
  }
  if (tid == 0) {
    const bool relative = p.rep >= OVGPU_REP_ANCHORED_3D;
    const double *x = (relative ? p.p_FinA : p.p_FinG) + 3 * p.f;
    double v[3];
    lm_from_xyz(p.rep, V3{x[0], x[1], x[2]}, v); // UpdaterSLAM.cpp:213-221
    for (int j = 0; j < 3; j++) {
      p.lm.fej[3 * slot + j] = v[j];
      p.lm.value[3 * slot + j] = v[j] + (j >= j0 ? G[(size_t)j * LD + D] : 0.0); // new_variable->update(H_Linv * res), :569
    }
    p.lm.cov[slot] = id, p.lm.col[slot] = -1, p.lm.rep[slot] = p.rep;
    p.lm.anchor[slot] = relative ? (int32_t)p.meas_cc[p.anchor_meas[p.f]] : -1;
    p.feat_slot[p.f] = slot;
  }
  __syncthreads();
  if (tid == 0) p.ctr[0] = id + p.sz, p.ctr[1] = slot + 1;
}

} // namespace ovg
