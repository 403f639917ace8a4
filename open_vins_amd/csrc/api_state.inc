// api_state.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): options, ovgpu_create / destroy, ovgpu_set_state / reset_state / set_camera_poses, ovgpu_set_features and the row layout of a feature batch.

const char *ovgpu_last_error(void) { return g_err.c_str(); }

void ovgpu_default_options(ovgpu_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->chi2_multipler = 5.0, o->sigma_pix = 1.0; // UpdaterOptions.h:35-41
  o->triangulate_1d = 0, o->refine_features = 1, o->max_runs = 5; // FeatureInitializerOptions.h:36-42
  o->init_lamda = 1e-3, o->max_lamda = 1e10, o->min_dx = 1e-6, o->min_dcost = 1e-6, o->lam_mult = 10;
  o->min_dist = 0.10, o->max_dist = 60, o->max_baseline = 40, o->max_cond_number = 10000;
  o->do_fej = 1, o->do_calib_camera_pose = 1, o->do_calib_camera_intrinsics = 1; // StateOptions.h:38-47 (true in shipped configs)
  o->feat_rep_msckf = OVGPU_REP_GLOBAL_3D;
}

double ovgpu_chi2_quantile_95(int dof) { return chi2_quantile_95(dof); }
int ovgpu_abi_version(void) { return OVGPU_ABI_VERSION; }

// what ovgpu_create does to a fresh context (the device is current); on an error the caller deletes it
static int init_context(ovgpu_ctx *c, const ovgpu_options *opts, int device) {
  c->device = device;
  c->opts = *opts;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->lds_limit = (int)std::min<size_t>(prop.sharedMemPerBlock, 160 * 1024);
  HIPCHK(hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking));
  c->up.stream = c->down.stream = c->stream;
  HIPCHK(c->ctrl.reserve(CTRL_INTS));
  HIPCHK(hipMemset(c->ctrl.p, 0, CTRL_INTS * sizeof(int32_t)));
  // the views into it, set here and nowhere else (DevView: nothing to reserve or release; they go with ctrl)
  c->flags.p = c->ctrl.p; // 4 words
  // words 24 .. 26 sit BETWEEN the two sets of Cholesky step flags (8 .. 23, 32 .. 47): together with either set they are one contiguous range
  // (enqueue_speculative_prior zeroes them and the set the update's own factorisation will use ahead of time, in one launch)
  c->rows_used.p = c->ctrl.p + 24; // [0] rows of accepted features, [1] features passed by the gate's residual bound
  c->feat_counter.p = c->ctrl.p + 26;
  c->chol_prog.p = c->ctrl.p + 8; // 40 words: set 0 at +0, set 1 at +24 (CHOL_PROG_STRIDE)
  c->ctrl_pre = 0;
  DevOptions &d = c->dopt;
  d.chi2_multipler = opts->chi2_multipler;
  d.sigma_pix_sq = opts->sigma_pix * opts->sigma_pix; // UpdaterMSCKF.cpp:45
  d.init_lamda = opts->init_lamda, d.max_lamda = opts->max_lamda, d.min_dx = opts->min_dx, d.min_dcost = opts->min_dcost;
  d.lam_mult = opts->lam_mult, d.min_dist = opts->min_dist, d.max_dist = opts->max_dist, d.max_baseline = opts->max_baseline;
  d.max_cond_number = opts->max_cond_number;
  d.triangulate_1d = opts->triangulate_1d, d.refine_features = opts->refine_features, d.max_runs = opts->max_runs;
  d.do_fej = opts->do_fej, d.do_calib_pose = opts->do_calib_camera_pose, d.do_calib_intr = opts->do_calib_camera_intrinsics;
  d.feat_rep = opts->feat_rep_msckf;
  d.gate_always_factor = opts->gate_always_factor != 0;
  if (d.feat_rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) d.feat_rep = OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH; // UpdaterMSCKF.cpp:180-183
  c->row_stride = (d.feat_rep >= OVGPU_REP_ANCHORED_3D) ? 72 : 48;
  // library switches are options of the context, not of the environment (include/ovgpu.h)
  if (opts->compress_route < 0 || opts->compress_route > OVGPU_COMPRESS_PCHOLQR || opts->compress_route == 2 /* the retired unpivoted factor */ || opts->tsqr_overlap < 0 || opts->tsqr_overlap > 2 || opts->tsqr_workers < 0) {
    return set_err(OVGPU_ERR_INVALID, "bad library switch in ovgpu_options");
  }
  c->tree_pipelined = opts->tsqr_no_pipeline == 0;
  c->prior_overlap = opts->no_prior_overlap == 0;
  c->compress_gram = opts->compress_route == OVGPU_COMPRESS_TSQR ? 0 : 1;
  c->mode_a_factor = opts->compress_route == OVGPU_COMPRESS_TSQR ? 0 : 2;
  c->tree_overlap = opts->tsqr_overlap == 0 ? -1 : (opts->tsqr_overlap == 1 ? 1 : 0);
  c->whiten = opts->gram_no_whiten == 0;
  c->prior_pivot_tol = opts->prior_pivot_tol > 0.0 ? opts->prior_pivot_tol : 1e-13;
  c->tsqr_workers = opts->tsqr_workers;
  c->no_feat_kernel = opts->no_fast_feature_kernel != 0;
  c->no_chol_pipe = opts->no_single_launch_cholesky != 0;
  c->feat_shape = opts->feature_kernel_shape;
  c->gram_fp32 = opts->gram_fp32 != 0;
  if (c->ev_rows.create(hipEventDisableTiming) != hipSuccess) c->no_feat_kernel = true;
  // The side stream (the prior block's factorisation next to the triangulation) gets a PRIORITY of its own: the runtime deals its hardware queues
  // per priority level, so this stream never lands on the queue of the context's main stream.  Without it the SECOND context of a process
  // (bench.py's extras; the drop-in's UpdaterSLAM context beside UpdaterMSCKF's) had both streams on one hardware queue and ran its two
  // head chains one after the other: 0.827 instead of 0.762 ms per update (tools/dev_two_contexts.py, round 5).
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (hipStreamCreateWithPriority(&c->stream2.h, hipStreamNonBlocking, prio_hi) != hipSuccess || c->ev_fork.create(hipEventDisableTiming) != hipSuccess ||
      c->ev_join.create(hipEventDisableTiming) != hipSuccess)
    c->tree_overlap = 0;
  c->timing = opts->no_timing == 0;
  return OVGPU_OK;
}

int ovgpu_create(const ovgpu_options *opts, int device, ovgpu_ctx **out) {
  if (!opts || !out) return set_err(OVGPU_ERR_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return set_err(OVGPU_ERR_NO_DEVICE, std::string("no HIP device (") + hipGetErrorString(e) + "): this library has no CPU fallback");
  if (device < 0 || device >= ndev) return set_err(OVGPU_ERR_INVALID, "device index out of range");
  if (opts->feat_rep_msckf < 0 || opts->feat_rep_msckf > OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE)
    return set_err(OVGPU_ERR_INVALID, "unknown feature representation");
  HIPCHK(hipSetDevice(device));
  ovgpu_ctx *c = new ovgpu_ctx();
  const int rc = init_context(c, opts, device);
  if (rc != OVGPU_OK) {
    delete c; // (nothing has been enqueued yet: what exists by now goes with the struct)
    return rc;
  }
  *out = c;
  return OVGPU_OK;
}

void ovgpu_destroy(ovgpu_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)upload_sync(c, c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2); // a prior-block factorisation nobody joined
  // Every launch and asynchronous copy that touches a buffer of this context was enqueued on one of these two streams (the loop-back collective's
  // reads from other ranks' streams are ordered before this stream's tail by its `ready` events), and both are idle now: nothing is in flight, so
  // the members may go in any order — the buffers (OwnedBuf), the events and the two streams (Event, Stream) each free what they own.
  delete c;
}

// state dof of a resident landmark: the single-depth representation keeps its bearing as a constant (Landmark.cpp:124-140)
static int lm_dof(int rep) { return rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? 1 : 3; }
static bool lm_any_anchored(const ovgpu_ctx *c) {
  for (int l = 0; l < c->L; l++)
    if (c->h_lm_rep[l] >= OVGPU_REP_ANCHORED_3D) return true;
  return false;
}
// 3 or 1 when every resident landmark has that many dof, 0 for a mix (3 without landmarks)
static int lm_uniform_dof(const ovgpu_ctx *c) {
  int d = c->L > 0 ? lm_dof(c->h_lm_rep[0]) : 3;
  for (int l = 1; l < c->L; l++)
    if (lm_dof(c->h_lm_rep[l]) != d) return 0;
  return d;
}

// zero one of the control block's views, unless the block-wide memset at the start of this pipeline call already did (ctrl_clean)
static hipError_t ctrl_zero(ovgpu_ctx *c, unsigned bit, void *ptr, size_t bytes, hipStream_t s) {
  if (c->ctrl_clean & bit) {
    c->ctrl_clean &= ~bit;
    c->ctrl_pre &= ~bit;
    return hipSuccess;
  }
  if (c->ctrl_pre & bit) { // zeroed ahead of time by enqueue_speculative_prior (on the context's stream, before the fork), untouched since
    c->ctrl_pre &= ~bit;
    return hipSuccess;
  }
  return hipMemsetAsync(ptr, 0, bytes, s);
}

static int launch_build_tables(ovgpu_ctx *c) {
  const int n = std::max(c->K * c->C, std::max(c->C, c->K));
  hipLaunchKernelGGL(k_build_tables, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->C, c->K, c->clone_qp.p, c->clone_fej.p, c->calib_qp.p,
                     c->tab_clone.p, c->tab_cam.p, c->tab_cc.p);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// the resident state as it is now becomes what ovgpu_reset_state goes back to (P0 sized for the current N)
static int copy_reset_baseline(ovgpu_ctx *c) {
  const size_t N = (size_t)c->N, C = (size_t)c->C, K = (size_t)c->K;
  hipStream_t s = c->stream;
  HIPCHK(c->P0.reserve(N * N));
  HIPCHK(c->clone_qp0.reserve(7 * C));
  HIPCHK(hipMemcpyAsync(c->P0.p, c->P.p, sizeof(double) * N * N, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(c->clone_qp0.p, c->clone_qp.p, sizeof(double) * 7 * C, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(c->calib_qp0.p, c->calib_qp.p, sizeof(double) * 7 * K, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(c->intr0.p, c->intr.p, sizeof(double) * 8 * K, hipMemcpyDeviceToDevice, s));
  return OVGPU_OK;
}

// the covariance at dimension N_to: its leading n_copy x n_copy block (leading dimension ld_from) into Ppad, zero beyond, and Ppad becomes P
static int cov_resize(ovgpu_ctx *c, int n_copy, int N_to, int ld_from) {
  HIPCHK(c->Ppad.reserve((size_t)N_to * N_to));
  hipLaunchKernelGGL(k_cov_copy, dim3((N_to + 255) / 256, N_to), dim3(256), 0, c->stream, n_copy, N_to, c->P.p, ld_from, c->Ppad.p, N_to);
  HIPCHK(hipGetLastError());
  std::swap(c->P, c->Ppad);
  c->N = N_to;
  return OVGPU_OK;
}

// Canonical column order of the stacked Jacobian: calibrated camera variables, clones and (SLAM) landmarks sorted by
// covariance id.  build_columns sorts the resident variables (ovgpu_set_state, ovgpu_set_landmarks and every structural change of the
// state); layout_columns lays the columns out over that sorted list for the active landmark set (ovgpu_set_active_landmarks: a linear
// walk, no sort) or, without one, for every resident landmark.
static int layout_columns(ovgpu_ctx *c, bool defer_flush = false, const int32_t *resident_set = nullptr);
static int build_columns(ovgpu_ctx *c, bool defer_flush = false) {
  std::vector<ovgpu_ctx::HVar> vars = c->h_vars;
  for (int l = 0; l < c->L; l++) vars.push_back({c->h_lm_cov[l], lm_dof(c->h_lm_rep[l]), COL_LANDMARK, l});
  std::stable_sort(vars.begin(), vars.end(), [](const ovgpu_ctx::HVar &a, const ovgpu_ctx::HVar &b) { return a.cov < b.cov; });
  for (const auto &v : vars)
    if (v.cov < 0 || v.cov + v.size > c->N) return set_err(OVGPU_ERR_INVALID, "covariance id out of range");
  c->h_sorted.swap(vars);
  c->var_tab_ok = false;
  if (c->active_given) c->h_lm_active.resize(c->L, 0); // (landmarks the delayed initialisation appended are outside the set)
  return layout_columns(c, defer_flush);
}

// (the uploads are flushed HERE whatever the caller's defer_flush says: the kernel reads them; ovgpu_set_state, the one caller that defers, has no set)
// the device builds the tables of an active set itself, in one launch behind the two small uploads (k_active_columns, k_slam.h); the host's walk
// in layout_columns is the mirror that sizes the workspaces and nobody waits for the device
static int upload_var_tab(ovgpu_ctx *c) {
  const int V = (int)c->h_sorted.size();
  if (!c->var_tab_ok) {
    std::vector<int32_t> tab((size_t)4 * std::max(V, 1), 0);
    for (int v = 0; v < V; v++) tab[4 * v] = c->h_sorted[v].cov, tab[4 * v + 1] = c->h_sorted[v].size, tab[4 * v + 2] = c->h_sorted[v].kind, tab[4 * v + 3] = c->h_sorted[v].index;
    HIPCHK(c->var_tab.reserve(tab.size()));
    HIPCHK(c->up.put(c->var_tab.p, tab.data(), sizeof(int32_t) * tab.size()));
    c->var_tab_ok = true;
  }
  return OVGPU_OK;
}
// `resident`: the set is on the device already, n_active indices (ovgpu_slam_update_chunked uploads every chunk's set and the variable table in
// front of its first chunk); otherwise the set is uploaded here, behind the variable table if that is stale
static int enqueue_active_columns(ovgpu_ctx *c, const std::vector<int32_t> &active_idx, int D, const int32_t *resident = nullptr) {
  const int V = (int)c->h_sorted.size();
  if (!resident) {
    const int rcv = upload_var_tab(c);
    if (rcv != OVGPU_OK) return rcv;
    HIPCHK(c->active_idx.reserve(std::max<size_t>(active_idx.size(), 1)));
    HIPCHK(c->up.put(c->active_idx.p, active_idx.data(), sizeof(int32_t) * active_idx.size()));
  }
  HIPCHK(c->up.flush());
  HIPCHK(c->lm_col.reserve(std::max(c->L, 1)));
  ActiveColsParams ap;
  ap.V = V, ap.L = c->L, ap.C = c->C, ap.K = c->K, ap.n_active = (int)active_idx.size(), ap.Dcap = D;
  ap.vars = c->var_tab.p, ap.active_idx = resident ? resident : c->active_idx.p;
  ap.clone_col = c->clone_col.p, ap.calib_col = c->calib_col.p, ap.intr_col = c->intr_col.p, ap.lm_col = c->lm_col.p, ap.col_cov = c->col_cov.p;
  ap.col_kind = c->col_kind.p, ap.col_sub = c->col_sub.p, ap.col_var = c->col_var.p;
  hipLaunchKernelGGL(k_active_columns, dim3(1), dim3(64), (size_t)((c->L + 15) & ~15), c->stream, ap);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

static int layout_columns(ovgpu_ctx *c, bool defer_flush, const int32_t *resident_set) {
  const std::vector<ovgpu_ctx::HVar> &vars = c->h_sorted;
  const int C = c->C, K = c->K, N = c->N;
  const bool act = c->active_given;
  // More than 511 columns: no call can carry them (k_system's and the factorisations' tables).  The map falls back to calibration and clones,
  // which every other entry point can still use, and the SLAM entry points return OVGPU_ERR_CAPACITY with cols_over_msg until a set that fits is named.
  int D_want = 0, n_act = 0;
  for (const auto &v : vars) {
    const bool on = v.kind != COL_LANDMARK || !act || c->h_lm_active[v.index];
    D_want += on ? v.size : 0, n_act += (on && v.kind == COL_LANDMARK) ? 1 : 0;
  }
  c->cols_over = D_want + 1 > 512;
  c->lm_empty_set = c->L > 0 && act && n_act == 0; // no landmark has a column: the map below is a landmark-free state's (ovgpu_msckf_update_lm)
  if (c->cols_over)
    c->cols_over_msg = std::string("the active landmark set (") + (act ? std::to_string(n_act) + " landmarks named by ovgpu_set_active_landmarks" : "all " + std::to_string(c->L) + " resident landmarks: no set was named") +
                       ") gives " + std::to_string(D_want) + " Jacobian columns, more than 511: name the batch's landmarks with ovgpu_set_active_landmarks";
  // (with an active set only D, h_col_cov, h_lm_col, active_idx and the raw-stack classes of this walk are used: the tables themselves are k_active_columns',
  //  k_slam.h, which repeats the walk on the device — change the two together)
  std::vector<int32_t> clone_col(C, -1), calib_col(K, -1), intr_col(K, -1), col_cov, active_idx;
  std::vector<uint8_t> col_kind, col_sub;
  std::vector<uint16_t> col_var;
  c->h_lm_col.assign(c->L, -1);
  int D = 0;
  for (const auto &v : vars) {
    if (v.kind == COL_LANDMARK && (c->cols_over || (act && !c->h_lm_active[v.index]))) continue;
    if (v.kind == COL_CLONE) clone_col[v.index] = D;
    if (v.kind == COL_CALIB_POSE) calib_col[v.index] = D;
    if (v.kind == COL_CALIB_INTR) intr_col[v.index] = D;
    if (v.kind == COL_LANDMARK) c->h_lm_col[v.index] = D, active_idx.push_back(v.index);
    for (int i = 0; i < v.size; i++) {
      col_cov.push_back(v.cov + i);
      col_kind.push_back((uint8_t)v.kind);
      col_var.push_back((uint16_t)v.index);
      col_sub.push_back((uint8_t)((v.kind == COL_LANDMARK && v.size == 1) ? 2 : i)); // the depth is column 2 of H_f
    }
    D += v.size;
  }
  c->D = D, c->LD = D + 1;
  { // the regions of the unprojected stack (ovgpu_types.h: RawStack): classes of clones by the tile column their block ends in
    c->raw_cols_ok = false, c->raw_ncls = 0, c->raw_tables_ok = false;
    int calib_end = 0, clone_min = D;
    for (int k = 0; k < K; k++) calib_end = std::max(calib_end, std::max(calib_col[k] >= 0 ? calib_col[k] + 6 : 0, intr_col[k] >= 0 ? intr_col[k] + 8 : 0));
    for (int i = 0; i < C; i++)
      if (clone_col[i] >= 0) clone_min = std::min(clone_min, clone_col[i]);
    const int NTf = (D + 1 + 15) / 16;
    if ((c->L == 0 || c->lm_empty_set) && calib_end <= clone_min && NTf >= 6 && NTf <= 15) { // (with landmarks only the fused kernels of ovgpu_msckf_update_lm write this stack)
      const int top = NTf == 15 ? 15 : ((NTf + 1) & ~1); // (k_gram_il has the even counts and 15)
      int n = 0;
      for (int t = 4; t < top && n < RAW_MAXCLS - 1 && !c->raw_one_region; t += 2)
        // (row strides of 16 t - 3 doubles: ODD multiples of 8 bytes.  At 16 t the rows of a region start 512 .. 1792 bytes apart and the per-feature
        //  kernel's 512-byte row segments camp on a fraction of the memory channels: its store phase took 1.7 x the time of the 209-double stack's)
        if (16 * t - 4 >= calib_end + 6) c->raw_ntc[n] = t, c->raw_ld[n] = 16 * t - 3, c->raw_rcol[n] = 16 * t - 4, n++;
      c->raw_ntc[n] = top, c->raw_ld[n] = D + 1, c->raw_rcol[n] = D, n++;
      c->raw_ncls = n;
      c->raw_ntc[RAW_NEG] = top, c->raw_ld[RAW_NEG] = D + 1, c->raw_rcol[RAW_NEG] = D;
      c->h_cls_of_clone.assign(C, (uint8_t)(n - 1));
      for (int i = 0; i < C; i++) {
        int k = 0;
        while (k < n - 1 && clone_col[i] + 6 > c->raw_rcol[k]) k++;
        c->h_cls_of_clone[i] = (uint8_t)k;
      }
      HIPCHK(c->cls_of_clone.reserve(C));
      HIPCHK(c->up.put(c->cls_of_clone.p, c->h_cls_of_clone.data(), C));
      c->raw_j0 = clone_min + 6; // the oldest clone's block and the calibration columns left of it: the prior's common mode (ovgpu_types.h)
      c->raw_cols_ok = true;
    }
  }
  c->h_col_cov = col_cov;
  HIPCHK(c->col_cov.reserve(D));
  HIPCHK(c->col_kind.reserve(D));
  HIPCHK(c->col_sub.reserve(D));
  HIPCHK(c->col_var.reserve(D));
  HIPCHK(c->Mt.reserve((size_t)D * N));
  HIPCHK(c->Aaug.reserve((size_t)D * (D + N + 1)));
  HIPCHK(c->Yaug.reserve((size_t)D * (D + N + 1)));
  if (act) { // tables of an active set: built on the device (the uploads leave there)
    const int rca = enqueue_active_columns(c, active_idx, D, resident_set); // (resident_set lists the set in this walk's order)
    if (rca != OVGPU_OK) return rca;
  } else {
    HIPCHK(c->up.put(c->clone_col.p, clone_col.data(), sizeof(int32_t) * C));
    HIPCHK(c->up.put(c->calib_col.p, calib_col.data(), sizeof(int32_t) * K));
    HIPCHK(c->up.put(c->intr_col.p, intr_col.data(), sizeof(int32_t) * K));
    HIPCHK(c->up.put(c->col_cov.p, col_cov.data(), sizeof(int32_t) * D));
    HIPCHK(c->up.put(c->col_kind.p, col_kind.data(), D));
    HIPCHK(c->up.put(c->col_sub.p, col_sub.data(), D));
    HIPCHK(c->up.put(c->col_var.p, col_var.data(), sizeof(uint16_t) * D));
    if (c->L > 0) HIPCHK(c->up.put(c->lm_col.p, c->h_lm_col.data(), sizeof(int32_t) * c->L));
    // (the scatter launch that carries them may be the caller's — ovgpu_set_state adds its own arrays to it — and leaves here otherwise)
    if (!defer_flush) HIPCHK(c->up.flush());
  }
  c->have_feats = false;           // workspaces depend on D
  c->tri_readable = false;
  return OVGPU_OK;
}

int ovgpu_set_state(ovgpu_ctx *c, const ovgpu_state_view *st) {
  if (!c || !st) return set_err(OVGPU_ERR_INVALID, "null argument");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (st->N <= 0 || st->C <= 0 || st->K <= 0) return set_err(OVGPU_ERR_INVALID, "empty state");
  if (st->C > OVG_MAX_CLONES || st->K > OVG_MAX_CAMS) return set_err(OVGPU_ERR_CAPACITY, "too many clones / cameras");
  if (!st->P || !st->clone_q_p || !st->clone_q_p_fej || !st->clone_cov_id || !st->calib_q_p || !st->intrinsics || !st->cam_is_fisheye ||
      !st->calib_cov_id || !st->intr_cov_id)
    return set_err(OVGPU_ERR_INVALID, "null state array");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->up.begin());
  const int N = st->N, C = st->C, K = st->K;

  // ---- canonical column order: calibrated camera variables and clones sorted by covariance id
  c->h_vars.clear();
  for (int k = 0; k < K; k++) {
    if (c->dopt.do_calib_pose && st->calib_cov_id[k] >= 0) c->h_vars.push_back({st->calib_cov_id[k], 6, COL_CALIB_POSE, k});
    if (c->dopt.do_calib_intr && st->intr_cov_id[k] >= 0) c->h_vars.push_back({st->intr_cov_id[k], 8, COL_CALIB_INTR, k});
  }
  for (int i = 0; i < C; i++) c->h_vars.push_back({st->clone_cov_id[i], 6, COL_CLONE, i});
  c->N = N, c->C = C, c->K = K;
  c->gram_wide_on = c->gram_wide; // ("gram_wide": with the state and with the batch, end_feature_batch)
  c->mode_a_wide_on = c->mode_a_wide; // ("mode_a_wide": likewise)
  c->slam_mode_a_on = c->slam_mode_a; // ("slam_mode_a": likewise)
  c->mode_a_panel_on = c->mode_a_panel; // ("mode_a_panel": likewise)
  c->L = 0, c->h_lm_rep.clear(), c->h_lm_cov.clear(), c->h_lm_col.clear(), c->h_lm_anchor.clear();
  c->active_given = false, c->h_lm_active.clear(); // an active landmark set holds until the state or the landmarks are replaced
  c->row_stride = (c->dopt.feat_rep >= OVGPU_REP_ANCHORED_3D) ? 72 : 48;
  HIPCHK(c->clone_col.reserve(C));
  HIPCHK(c->calib_col.reserve(K));
  HIPCHK(c->intr_col.reserve(K));
  {
    const int rcb = build_columns(c, true);
    if (rcb != OVGPU_OK) return rcb;
  }
  const int D = c->D;

  HIPCHK(c->P.reserve((size_t)N * N));
  HIPCHK(c->P0.reserve((size_t)N * N));
  HIPCHK(c->clone_qp.reserve(7 * C));
  HIPCHK(c->clone_qp0.reserve(7 * C));
  HIPCHK(c->clone_fej.reserve(7 * C));
  HIPCHK(c->calib_qp.reserve(7 * K));
  HIPCHK(c->calib_qp0.reserve(7 * K));
  HIPCHK(c->intr.reserve(8 * K));
  HIPCHK(c->intr0.reserve(8 * K));
  HIPCHK(c->fisheye.reserve(K));
  HIPCHK(c->clone_cov.reserve(C));
  HIPCHK(c->calib_cov.reserve(K));
  HIPCHK(c->intr_cov.reserve(K));
  HIPCHK(c->tab_clone.reserve(24 * C));
  HIPCHK(c->tab_cam.reserve(12 * K));
  HIPCHK(c->tab_cc.reserve((size_t)12 * K * C));
  HIPCHK(c->Mt.reserve((size_t)D * N));
  HIPCHK(c->Aaug.reserve((size_t)D * (D + N + 1)));
  HIPCHK(c->Yaug.reserve((size_t)D * (D + N + 1)));
  HIPCHK(c->dx.reserve(N));

  // calibration ids the kernels see: -1 when that calibration is not being estimated
  std::vector<int32_t> calib_cov(K), intr_cov(K);
  for (int k = 0; k < K; k++) {
    calib_cov[k] = (c->dopt.do_calib_pose && st->calib_cov_id[k] >= 0) ? st->calib_cov_id[k] : -1;
    intr_cov[k] = (c->dopt.do_calib_intr && st->intr_cov_id[k] >= 0) ? st->intr_cov_id[k] : -1;
  }
  c->h_clone_cov.assign(st->clone_cov_id, st->clone_cov_id + C);
  c->h_calib_cov = calib_cov, c->h_intr_cov = intr_cov;
  // one scatter launch for the column map (build_columns above) and the state: the device-side copy of the prior that ovgpu_reset_state
  // restores is a second destination of the same arena bytes (round 5: four device-to-device copies behind nine uploads)
  bool twins = true;
  HIPCHK(c->up.put2(c->P.p, c->P0.p, st->P, sizeof(double) * N * N, twins));
  HIPCHK(c->up.put2(c->clone_qp.p, c->clone_qp0.p, st->clone_q_p, sizeof(double) * 7 * C, twins));
  HIPCHK(c->up.put2(c->calib_qp.p, c->calib_qp0.p, st->calib_q_p, sizeof(double) * 7 * K, twins));
  HIPCHK(c->up.put2(c->intr.p, c->intr0.p, st->intrinsics, sizeof(double) * 8 * K, twins));
  HIPCHK(c->up.put(c->clone_fej.p, st->clone_q_p_fej, sizeof(double) * 7 * C));
  HIPCHK(c->up.put(c->fisheye.p, st->cam_is_fisheye, K));
  HIPCHK(c->up.put(c->clone_cov.p, st->clone_cov_id, sizeof(int32_t) * C));
  HIPCHK(c->up.put(c->calib_cov.p, calib_cov.data(), sizeof(int32_t) * K));
  HIPCHK(c->up.put(c->intr_cov.p, intr_cov.data(), sizeof(int32_t) * K));
  // the caller's buffers may change when this returns: the bytes sit in the page-locked arena or on the device (Uplink::put)
  HIPCHK(c->up.flush());
  int rc = OVGPU_OK;
  if (!twins && (rc = copy_reset_baseline(c)) != OVGPU_OK) return rc; // (an array bypassed the arena, or the launch was split: the copies of rounds 4-5)
  rc = launch_build_tables(c);
  if (rc != OVGPU_OK) return rc;
  c->have_state = true, c->poses_only = false;
  c->have_feats = false; // workspaces depend on D
  c->tri_readable = false;
  return OVGPU_OK;
}

int ovgpu_reset_state(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  HIPCHK(hipSetDevice(c->device));
  RestoreParams r;
  r.N2 = c->N * c->N, r.nC = 7 * c->C, r.nK7 = 7 * c->K, r.nK8 = 8 * c->K, r.C = c->C, r.K = c->K;
  r.P = c->P.p, r.clone_qp = c->clone_qp.p, r.calib_qp = c->calib_qp.p, r.intr = c->intr.p;
  r.P0 = c->P0.p, r.clone_qp0 = c->clone_qp0.p, r.calib_qp0 = c->calib_qp0.p, r.intr0 = c->intr0.p, r.clone_fej = c->clone_fej.p;
  r.tab_clone = c->tab_clone.p, r.tab_cam = c->tab_cam.p, r.tab_cc = c->tab_cc.p;
  const int n = std::max(std::max(r.N2, r.nC), std::max(r.nK8, c->K * c->C));
  hipLaunchKernelGGL(k_restore_state, dim3((n + 255) / 256), dim3(256), 0, c->stream, r);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// Sizes the stacked-system buffer and the TSQR leaf layout for the batch's rows_total rows of c->LD columns:
// one leaf node per CU when there are enough rows, every node a whole number of 128-row appends.
static int configure_tsqr(ovgpu_ctx *c) {
  const int D = c->D, LD = c->LD;
  const int64_t rows_total = batch_of(c).rows_total;
  HIPCHK(c->Hbig.reserve((size_t)std::max<int64_t>(rows_total, 1) * LD));
  const int64_t blk = 4 * QR_LEAF_Q;
  const int64_t target = std::max<int64_t>(1, c->tsqr_workers > 0 ? c->tsqr_workers : c->num_cu);
  int64_t rpn = (rows_total + target - 1) / target;
  rpn = std::max<int64_t>(blk, ((rpn + blk - 1) / blk) * blk);
  if (rpn < 2 * blk && rows_total > 2 * blk) rpn = 2 * blk; // a leaf shorter than D rows compresses nothing
  c->rows_per_node = rpn;
  c->W = (int)std::max<int64_t>(1, (rows_total + rpn - 1) / rpn);
  HIPCHK(c->Rws.reserve((size_t)std::max(c->W, 16) * D * LD));
  return OVGPU_OK;
}

// FeatureInitializer's own input: the clone-camera poses, supplied directly
int ovgpu_set_camera_poses(ovgpu_ctx *c, int C, int K, const double *R_GtoC, const double *p_CinG) {
  if (!c || !R_GtoC || !p_CinG) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (C <= 0 || K <= 0 || C > OVG_MAX_CLONES || K > OVG_MAX_CAMS) return set_err(OVGPU_ERR_CAPACITY, "bad clone / camera count");
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> tab((size_t)12 * K * C);
  for (int i = 0; i < K * C; i++) {
    std::memcpy(&tab[(size_t)12 * i], R_GtoC + (size_t)9 * i, 9 * sizeof(double));
    std::memcpy(&tab[(size_t)12 * i + 9], p_CinG + (size_t)3 * i, 3 * sizeof(double));
  }
  HIPCHK(c->tab_cc.reserve(tab.size()));
  HIPCHK(upload(c->tab_cc.p, tab.data(), sizeof(double) * tab.size(), c->stream));
  HIPCHK(upload_sync(c, c->stream));
  c->C = C, c->K = K, c->N = 0, c->D = 0, c->LD = 1, c->L = 0;
  c->have_state = true, c->poses_only = true, c->have_feats = false, c->tri_readable = false;
  return OVGPU_OK;
}

// Whether the fused MSCKF kernel of the resident batch is the block-row one (k_featy_big.h: the batch was laid out for it, or ovgpu_debug_option
// "featy_big" forces it on a batch the one-pass kernels hold), and with it the columns per block of the sweep.  The batch's instance lists
// (k_feat_inst, k_featy.h) are built for that width when the batch is laid out; enqueue_system builds them again if the switch was thrown in between.
static bool featy_block_rows(const ovgpu_ctx *c) { return c->plan.msckf == FK_FEATY_BIG || c->featy_big; }
static int featy_block_cols(const ovgpu_ctx *c) { return featy_block_rows(c) ? 32 : feat::FY_CB; }
// The integer tables of a batch that depend on the batch and on the column map alone — with `anchors` the triangulation's anchor measurements
// (every path), on the fast path measurement -> feature, the clone-major positions and (fused kernels) the column-block lists of the tile rows
// for blocks of `cb` columns — (re)built by ONE launch on the context's stream (feat::k_batch_layout, k_featy.h; round 5: four launches).
// Called when the batch is laid out; ovgpu_debug_option "layout_every_update" = 1 calls it at the head of every update as well, so that a
// timing loop over a resident batch pays what a filter that hands over a new batch per frame pays inside ovgpu_set_features (bench.py's
// headline since round 6).
// second = true: the lists at 64 columns into fs_inst64 — the one-pass classes' of a batch whose longest fused track is the block-row kernel's
// ("feat_classes").  The pass runs over the whole batch (the lists are indexed by feature, a class is a slot range) and, since the kernel ranks a
// track's records on its way to the lists, writes measurement -> feature and the record positions again, the same values; the anchors and the
// unprojected stack's tables are left out
static int enqueue_batch_layout(ovgpu_ctx *c, bool anchors, int cb, bool second = false) {
  const Batch b = batch_of(c);
  const int F = b.F;
  const bool fast = c->plan.msckf != FK_GENERAL && b.M > 0; // (the instance lists go with the fast path's other tables)
  if (F > 0 && (anchors || fast)) {
    const int m_max = feat::batch_layout_m_pad(std::max(b.m_max, 1));
    // features per workgroup (k_featy.h: why eight); fewer where long tracks' tables would not fit 48 KB of LDS
    const size_t lds_one = feat::batch_layout_lds_ints(m_max) * sizeof(int32_t);
    int fpw_want = 1; // the fewest features per workgroup that keep the launch at 250 workgroups or fewer (measured: 800 features 0.4433 ms at four, 0.4477 at eight)
    while (fpw_want < std::min(c->layout_fpw, (int)feat::BL_FPW) && (F + fpw_want - 1) / fpw_want > 250) fpw_want *= 2;
    const int fpw = fast ? std::max(1, std::min<int>(fpw_want, (int)((48 * 1024) / lds_one))) : 1;
    const size_t lds = fast ? (size_t)fpw * lds_one : 0;
    const bool raw_tabs = fast && c->raw_tables_ok && !second;
    RawStack rw; // the regions' constants for the run table (raw_stack_layout has run)
    for (int k = 0; k <= RAW_NEG; k++) rw.base[k] = c->raw_base[k], rw.ld[k] = c->raw_ld[k], rw.rcol[k] = c->raw_rcol[k];
    hipLaunchKernelGGL(feat::k_batch_layout, dim3((F + fpw - 1) / fpw), dim3(fast ? feat::BL_NTH * fpw : 64), lds, c->stream, F, m_max, c->D, (const int32_t *)b.meas_offsets, (const uint16_t *)b.meas_cc,
                       (const int32_t *)c->clone_col.p, (const int32_t *)c->calib_col.p, (const int32_t *)c->intr_col.p, anchors ? c->anchor_pre.p : (int32_t *)nullptr,
                       fast ? c->fs_meas_feat.p : (int32_t *)nullptr, fast ? c->fs_pos.p : (int32_t *)nullptr, fast ? (second ? c->fs_inst64.p : c->fs_inst.p) : (int32_t *)nullptr, c->plan.nt, cb, c->C, c->K,
                       (const uint8_t *)c->cls_of_clone.p, (const int32_t *)c->raw_featbase.p, raw_tabs ? c->raw_dst.p : (int32_t *)nullptr,
                       raw_tabs ? c->raw_runs.p : (int32_t *)nullptr, rw);
    HIPCHK(hipGetLastError());
  }
  if (second) c->inst64_D = fast ? c->D : 0;
  else c->inst_cb = fast ? cb : 0, c->inst_D = c->D;
  return OVGPU_OK;
}
// the column-block lists again for another block width (enqueue_system: a switch that changes the sweep's block width was thrown after the layout)
static int enqueue_instance_lists(ovgpu_ctx *c, int cb) { return enqueue_batch_layout(c, false, cb); }
static int enqueue_instance_lists64(ovgpu_ctx *c) { return enqueue_batch_layout(c, false, feat::FY_CB, true); }
static int enqueue_batch_tables(ovgpu_ctx *c, bool anchors) {
  const int rc = enqueue_batch_layout(c, anchors, c->plan.msckf != FK_GENERAL ? featy_block_cols(c) : feat::FY_CB);
  c->inst64_D = 0;
  return rc == OVGPU_OK && c->plan.cls_mixed_width() ? enqueue_instance_lists64(c) : rc;
}

// The rows a feature of m measurements stacks.  MSCKF / delayed init: 2m - 3 after the nullspace projection (UpdaterHelper.cpp:449-450); SLAM
// update: all 2m (UpdaterSLAM.cpp:381-383) less the `proj` rows a single-depth landmark's bearing takes (UpdaterSLAM.cpp:371-379: 3 - dof).
static int feature_rows(bool slam_rows, int m, int proj) { return slam_rows ? std::max(2 * m - proj, 0) : (m >= 2 ? 2 * m - 3 : 0); }
// ... of every feature of b, as offsets: out[0 .. b.F].  A batch over landmarks of both sizes is laid out per feature once its landmarks are
// named (slam_prepare, a chunk); until then every feature gets the 2m rows of a 3-dof landmark
static void row_offsets_of(const ovgpu_ctx *c, const Batch &b, bool slam_rows, int64_t *out) {
  const int udof = lm_uniform_dof(c);
  out[0] = 0;
  for (int f = 0; f < b.F; f++) {
    int proj = udof == 1 ? 2 : 0;
    if (udof == 0 && (int)b.h_feat_lm.size() == b.F) proj = 3 - lm_dof(c->h_lm_rep[b.h_feat_lm[f]]);
    out[f + 1] = out[f] + feature_rows(slam_rows, b.h_offsets[f + 1] - b.h_offsets[f], proj);
  }
}
// The track order: feature indices by descending length, equal lengths in batch order — a counting sort (round 6; a comparison sort of 2000
// tracks was ~30 us of every frame).  offsets[0 .. F], order[0 .. F)
static void track_order(const int32_t *offsets, int F, int m_max, int32_t *order) {
  std::vector<int32_t> start(m_max + 2, 0);
  for (int f = 0; f < F; f++) start[m_max - (offsets[f + 1] - offsets[f]) + 1]++;
  for (int b = 0; b <= m_max; b++) start[b + 1] += start[b];
  for (int f = 0; f < F; f++) order[start[m_max - (offsets[f + 1] - offsets[f])]++] = f;
}

// Workgroups of a fused MSCKF kernel over `count` features: as many per CU as its registers (<4, 9, 2>: two; <8, 17, 1> and the block-row kernel:
// one) and its LDS block of `lds` bytes allow, the features dealt round-robin over them (select_feat_kernel and the length classes' plan)
static int fused_feat_grid(const ovgpu_ctx *c, FeatKernel k, size_t lds, int count) {
  const int per_cu = k == FK_FEATY_BIG ? 1 : std::max(1, std::min(k == FK_FEATY_4 ? 2 : 1, (int)((size_t)c->lds_limit / std::max<size_t>(lds, 1))));
  return std::max(1, std::min(count, c->num_cu * per_cu));
}

// The per-feature stage of batch b under the switches in force, as a value (FeatPlan, api_context.inc).  Pure: no HIP call, no reserve, nothing
// written to the context.
static FeatPlan plan_feature_stage(const ovgpu_ctx *c, const Batch &b) {
  FeatPlan pl;
  const int F = b.F, m_max = b.m_max, m1 = std::max(m_max, 1);
  const size_t limit = (size_t)c->lds_limit;
  // ---- the general kernel: LDS carve and (for long tracks) a global gate workspace
  size_t fixed = sys_lds_fixed_bytes(m1, c->row_stride, c->D);
  if (fixed >= limit) { // the records of the longest track do not fit LDS next to the T chunk: a global workspace holds them (k_system_t<true>)
    fixed = sys_lds_fixed_bytes(m1, c->row_stride, c->D, false);
    pl.rows_global = true;
  }
  if (fixed >= limit) {
    pl.error = "track too long for the per-feature kernel's LDS tables (block ids and reflectors of ~1900 observations at 208 columns)";
    return pl;
  }
  while (pl.m_lds_max < m_max && sys_gate_doubles(pl.m_lds_max + 1) * sizeof(double) <= limit - fixed) pl.m_lds_max++;
  pl.sys_lds = fixed + sys_gate_doubles(pl.m_lds_max) * sizeof(double);
  pl.sys_grid = std::max(1, std::min(F, c->num_cu * 4));
  pl.gate_ws_stride = pl.m_lds_max < m_max ? (int64_t)sys_gate_doubles(m_max) : 0;
  // (its panel routine, gate_chol_panel<8> of k_system.h, holds 512 rows of the gate's trapezoid in the registers of a wavefront's lanes and takes
  // longer trapezoids 512 rows at a time, round 5: a track's length is bounded by the block-id / reflector tables in LDS above, far beyond any
  // window; UpdaterMSCKF.cpp:216-222's dof >= 500 is reachable)
  // ---- MSCKF fast path (k_feat.h): the fused kernels, a block of 16 nt x 64 whitened rows in LDS instead of the row copies and the T chunk
  // (an anchored feat_rep_msckf takes it as well — k_feat_rows_anchored, k_featy.h: 48-double records whatever c->row_stride says, which stays the
  //  general kernel's; ovgpu_debug_option "anchored_fast" = 0 keeps such batches on the general kernel)
  // (resident landmarks under the empty active set have no column: the same batch, the same column map and the same kernels as without them.  The
  //  eligibility is recorded — lm_fast_ok — and only ovgpu_msckf_update_lm switches it on: enqueue_system, api_pipeline.inc)
  // (m: the longest track the fused kernels are to hold — the batch's; under "feat_classes" the longest of a fused class)
  auto fast_terms = [&](int m) {
    return !c->slam_rows && !c->no_feat_kernel && (c->dopt.feat_rep < OVGPU_REP_ANCHORED_3D || c->anchored_fast) && (c->L == 0 || c->lm_empty_set) && m >= 2 && c->K * c->C <= 8192 && c->D >= 16 &&
           (size_t)4 * (14 * std::max(m, 1) + 64) * sizeof(double) <= limit; // (the last: k_feat_vt's block, in front of every one of them)
  };
  if (fast_terms(m_max)) {
    // the gate matrix of the one-pass kernels: 2 m + 4 rows (the right-hand sides [r | H_f] are four augmented rows, k_featy.h), upper triangle
    const int nt = (2 * m_max + 15) / 16, nta = (2 * m_max + 4 + 15) / 16, tiles = nta * (nta + 1) / 2;
    // <4 wavefronts, 9 tiles each>, or <8, 17> (one workgroup per CU: 256 registers per lane) — options.feature_kernel_shape = 2 asks for it where
    // the first would do; beyond both the gate matrix does not fit the registers of a compute unit: block row by block row (k_featy_big.h)
    FeatKernel k = tiles <= 4 * 9 && c->feat_shape != 2 ? FK_FEATY_4 : (tiles <= 8 * 17 ? FK_FEATY_8 : FK_FEATY_BIG);
    const bool holds = k == FK_FEATY_BIG ? nt <= 29 && c->feat_shape == 0 && feat::featyb_lds_layout(nt, 8).total <= limit
                                         : feat::featy_lds_layout(nt, nta, k == FK_FEATY_4 ? 4 : 8, feat::FY_CB).total <= limit;
    if (holds) pl.msckf = k, pl.nt = nt, pl.nta = nta;
  }
  // ---- ovgpu_debug_option "feat_classes" = 1: a kernel per length class (feat_classes.h) — the rule above applied per track, every term that
  // reads no track length evaluated once, k_feat_vt's block sized by the longest FUSED track.  Only with the shape left to the library
  // (options.feature_kernel_shape = 0, "featy_big" = 0, the fast path not switched off) and the track lengths on the host: a batch of
  // ovgpu_set_features or ovgpu_tracks_to_features (begin_feature_batch), not a slice of one.  A batch of one class, and a batch one of whose
  // classes does not fit its LDS carve, keeps the single-kernel rule above.
  if (c->feat_classes >= 1 && c->feat_shape == 0 && !c->featy_big && !c->view && F > 0 && (int)b.h_order.size() == F && (int)b.h_offsets.size() == F + 1) {
    const featcls::Partition pt = featcls::partition(b.h_offsets.p, b.h_order.p, F);
    int first_fused = -1;
    for (int k = pt.n - 1; k >= 0; k--)
      if (pt.cls[k].kernel != featcls::FC_GENERAL) first_fused = k;
    bool ok = pt.n >= 2 && first_fused >= 0 && fast_terms(pt.cls[first_fused].m_max);
    // (the fast path's tables are built for EVERY track of such a batch, a general class's included: k_batch_layout keeps a track's keys in LDS,
    //  enqueue_batch_layout gives a workgroup 48 KB at the most — a batch whose longest track needs more keeps the single-kernel rule)
    ok = ok && feat::batch_layout_lds_ints(feat::batch_layout_m_pad(m1)) * sizeof(int32_t) <= (size_t)48 * 1024;
    FeatPlan::Class cl[featcls::FC_MAX];
    for (int k = 0; ok && k < pt.n; k++) {
      FeatPlan::Class &q = cl[k];
      q.kernel = (FeatKernel)pt.cls[k].kernel, q.begin = pt.cls[k].begin, q.end = pt.cls[k].end, q.m_max = pt.cls[k].m_max;
      const int count = q.end - q.begin;
      if (q.kernel == FK_GENERAL) { // the carve above: it was made for the batch's longest track, which is this class's
        q.lds = pl.sys_lds, q.grid = std::max(1, std::min(count, c->num_cu * 4));
        continue;
      }
      q.nt = featcls::tile_rows(q.m_max), q.nta = featcls::gate_tile_rows(q.m_max);
      q.lds = q.kernel == FK_FEATY_BIG ? feat::featyb_lds_layout(q.nt, 8).total : feat::featy_lds_layout(q.nt, q.nta, q.kernel == FK_FEATY_4 ? 4 : 8, feat::FY_CB).total;
      q.grid = fused_feat_grid(c, q.kernel, q.lds, count);
      ok = q.lds <= limit;
    }
    if (ok) {
      pl.n_classes = pt.n;
      for (int k = 0; k < pt.n; k++) pl.cls[k] = cl[k];
      pl.msckf = cl[first_fused].kernel, pl.nt = cl[first_fused].nt, pl.nta = cl[first_fused].nta, pl.m_fused = cl[first_fused].m_max;
    }
  }
  pl.lm_fast_ok = c->L > 0 && pl.msckf != FK_GENERAL;
  // ---- SLAM batches: the fused per-feature kernel k_slam_y (k_slam_y.h) behind ovgpu_debug_option "slam_fused", a level.  Eligible at level 1:
  // every landmark the batch observes is 3-dof (a batch that holds a single-depth landmark keeps the general kernel as a whole: its two
  // reflectors stay there), the longest track within the kernel's bound, and the fused kernels' limits on the state.  At level 2 a batch that
  // observes a single-depth landmark takes k_slam_y<true>, the instantiation with the projection, on the same terms and its own LDS carve; a
  // batch that observes none takes k_slam_y<false> as at level 1.  A batch of a mixed-dof state whose landmarks are not named yet is laid out
  // again once they are (slam_prepare).  Per-feature sigma / multiplier do not disqualify (ArUco corners).
  // Level 3 is level 2 with one addition: a batch whose longest track holds 63 .. 126 observations takes the long shape (16 tile rows, column
  // blocks of 32) on the same terms and its own carve; a batch of at most 62 takes the shapes of level 2.
  // "slam_fused_big" (a level of its own, acts at level 3 only): a batch whose longest track holds 127 .. SLY_MMAX_B observations takes the
  // block-row shape (k_slam_y_big.h) on the long shape's terms and its own carve; SLY_MMAX_B + 1 observations keep the general kernel.
  const bool big_on = c->slam_fused >= 3 && c->slam_fused_big;
  const int slamy_mmax = big_on ? slamy::SLY_MMAX_B : (c->slam_fused >= 3 ? slamy::SLY_MMAX_L : slamy::SLY_MMAX);
  if (c->slam_rows && c->slam_fused && !c->no_feat_kernel && c->L > 0 && m_max <= slamy_mmax && c->D >= 16 && c->K * c->C <= 8192) {
    const int udof = lm_uniform_dof(c);
    bool dof3 = udof == 3, named = udof != 0;
    if (udof == 0 && (int)b.h_feat_lm.size() == F) {
      dof3 = true, named = true;
      for (int f = 0; f < F; f++) dof3 = dof3 && lm_dof(c->h_lm_rep[b.h_feat_lm[f]]) == 3;
    }
    const bool proj = named && !dof3 && c->slam_fused >= 2;
    const bool lng = m_max > slamy::SLY_MMAX, big = m_max > slamy::SLY_MMAX_L;
    if (big) {
      const int nt = (2 * m_max + 15) / 16;
      if ((dof3 || proj) && slamy::slamyb_holds(m_max, proj, limit))
        pl.slam = proj ? FK_SLAMY_BIG_PROJ : FK_SLAMY_BIG, pl.slam_lds = slamy::slamyb_lds_layout(nt, proj).total, pl.slam_nt = nt;
    } else {
      const size_t lds = slamy::slamy_lds_layout(m1, proj, lng ? slamy::SLY_CB_L : slamy::SLY_CB).total;
      if ((dof3 || proj) && lds <= limit) pl.slam = FeatKernel((lng ? FK_SLAMY_LONG : FK_SLAMY) + (proj ? 1 : 0)), pl.slam_lds = lds;
    }
  }
  return pl;
}

// Sizes the per-feature stage for the batch in force and its row layout: the plan above, the workspaces it implies, the fused kernels' slot
// records, the stack and the TSQR leaf layout.  Reads the batch, writes none of it.
static int size_feature_stage(ovgpu_ctx *c) {
  const Batch b = batch_of(c);
  const int F = b.F, m1 = std::max(b.m_max, 1);
  const FeatPlan pl = plan_feature_stage(c, b);
  if (pl.error) return set_err(OVGPU_ERR_CAPACITY, pl.error);
  c->plan = pl;
  if (pl.rows_global) HIPCHK(c->sys_rows_ws.reserve((size_t)pl.sys_grid * m1 * c->row_stride));
  if (pl.gate_ws_stride) HIPCHK(c->gate_ws.reserve((size_t)pl.gate_ws_stride * pl.sys_grid));
  if (pl.msckf == FK_FEATY_BIG) HIPCHK(c->featyb_ws.reserve((size_t)std::max(1, std::min(F, c->num_cu)) * feat::featyb_ws_doubles(pl.nt))); // (a block-row CLASS: no more workgroups, the same tile rows)
  if (pl.slam >= FK_SLAMY_BIG) { // k_slam_y_big.h: the row panels' scratch and what its records kernel leaves for it
    const size_t M = std::max(b.M, 1), Fs = std::max(F, 1);
    HIPCHK(c->featyb_ws.reserve((size_t)std::max(1, std::min(F, c->num_cu)) * feat::featyb_ws_doubles(pl.slam_nt)));
    HIPCHK(c->slyb_rows.reserve(M * slamy::SLY_RS));
    HIPCHK(c->slyb_minfo.reserve(M * 8));
    HIPCHK(c->slyb_V.reserve(M * 6));
    HIPCHK(c->slyb_hq.reserve(Fs * 64));
    HIPCHK(c->slyb_inst.reserve(Fs * slamy::SLY_NT_B * slamy::SLY_ISTR));
  }
  if (pl.msckf != FK_GENERAL) { // row store of the fast path
    const int M = std::max(b.M, 1);
    HIPCHK(c->fs_tq.reserve((size_t)std::max(F, 1) * 8));
    HIPCHK(c->fs_inst.reserve((size_t)std::max(F, 1) * std::max(pl.nt, 1) * feat::FY_ISTR));
    if (pl.cls_mixed_width()) HIPCHK(c->fs_inst64.reserve((size_t)std::max(F, 1) * std::max(pl.nt, 1) * feat::FY_ISTR)); // (the same stride: one launch argument for both)
    HIPCHK(c->fs_rows.reserve((size_t)M * c->row_stride));
    HIPCHK(c->fs_minfo.reserve((size_t)M * 8));
    HIPCHK(c->fs_V.reserve((size_t)M * 6));
    HIPCHK(c->fs_meas_feat.reserve(M));
    HIPCHK(c->fs_pos.reserve(M));
    // the fused kernels' schedule: one record per slot, slots in the order of c->sys_order
    std::vector<int32_t> slots((size_t)8 * std::max(F, 1), 0);
    for (int sidx = 0; sidx < F; sidx++) {
      const int f = b.h_order[sidx];
      const HostSpan<int64_t> &row_off = b.h_row_off;
      int32_t *r = &slots[(size_t)8 * sidx];
      r[0] = f, r[1] = b.h_offsets[f], r[2] = b.h_offsets[f + 1] - b.h_offsets[f], r[3] = (int32_t)(row_off[f + 1] - row_off[f]);
      r[4] = (int32_t)(uint32_t)((uint64_t)row_off[f] & 0xffffffffu), r[5] = (int32_t)(uint32_t)((uint64_t)row_off[f] >> 32);
    }
    HIPCHK(c->fs_slots.reserve(slots.size()));
    HIPCHK(c->up.put(c->fs_slots.p, slots.data(), sizeof(int32_t) * slots.size()));
  }
  // ---- stacked system and TSQR accumulators
  return configure_tsqr(c);
}

// Row layout of the resident batch (the whole one: this writes its owners): the row offsets by the rule above, the stage sized for them, the
// offsets and the batch's integer tables on their way to the device.
static int set_row_layout(ovgpu_ctx *c, bool slam_rows, bool anchors = false) {
  if (c->view) return set_err(OVGPU_ERR_INVALID, "internal: the resident batch cannot be laid out while a part of it is in force");
  const int F = c->F;
  c->h_row_off.resize(F + 1);
  row_offsets_of(c, batch_of(c), slam_rows, c->h_row_off.data());
  c->rows_total = c->h_row_off[F];
  c->slam_rows = slam_rows;
  const int rcs = size_feature_stage(c);
  if (rcs != OVGPU_OK) return rcs;
  HIPCHK(c->row_off.reserve(F + 1));
  HIPCHK(c->up.put(c->row_off.p, c->h_row_off.data(), sizeof(int64_t) * (F + 1)));
  // everything ovgpu_set_features packed into the arena (offsets, packed codes, pixel coordinates, the slot records and row offsets above)
  // leaves by ONE scatter launch; behind it the batch's integer tables (one launch; `anchors`: a new batch, end_feature_batch)
  HIPCHK(c->up.flush());
  return enqueue_batch_tables(c, anchors);
}

// The regions of the unprojected stack for the batch whose packed (camera, clone) codes are `cc` (host): rows per region, every feature's first row
// in every region, the stack's size and the workgroups of k_gram_regions (dealt by rows x tiles of the region's triangle).
static int raw_stack_layout(ovgpu_ctx *c, const uint16_t *cc) {
  c->raw_tables_ok = false;
  const Batch b = batch_of(c);
  const int F = b.F, M = b.M, n = c->raw_ncls;
  if (!c->raw_enable || !c->raw_cols_ok || F <= 0 || M <= 0 || n <= 0) return OVGPU_OK;
  std::vector<int32_t> fb((size_t)F * RAW_MAXCLS, 0);
  int64_t run[RAW_MAXCLS + 1] = {0};
  for (int f = 0; f < F; f++) {
    int cnt[RAW_MAXCLS] = {0};
    for (int i = b.h_offsets[f]; i < b.h_offsets[f + 1]; i++) cnt[c->h_cls_of_clone[anchor_clone(cc[i])]]++;
    int below = 0;
    for (int k = 0; k < n; k++) {
      fb[(size_t)f * RAW_MAXCLS + k] = (int32_t)(run[k] - 2 * below);
      run[k] += 2 * cnt[k], below += cnt[k];
    }
  }
  run[RAW_NEG] = (int64_t)4 * F; // rows 4 f .. 4 f + 2: what the projection of feature f drops; row 4 f + 3: zero
  int64_t total = 0;
  double work[RAW_MAXCLS + 1] = {0}, work_sum = 0;
  int live = 0;
  for (int k = 0; k <= RAW_NEG; k++) {
    if (k >= n && k != RAW_NEG) {
      c->raw_rows[k] = 0, c->raw_base[k] = total;
      continue;
    }
    if (run[k] >= ((int64_t)1 << RAW_CLS_SHIFT)) return OVGPU_OK; // (a region beyond 134 M rows: the projected stack)
    c->raw_rows[k] = run[k], c->raw_base[k] = total;
    total += run[k] * c->raw_ld[k];
    // cycles of a 32-row stage of k_gram_il<ntc> ~ 128 T + 70 ntc + 1000 (T = ntc (ntc + 1) / 2 tiles, a quarter per wavefront at 64 cycles a product and 8 four-row
    // steps; staging of 2 ntc elements per thread; the stage barrier): in tiles per row
    work[k] = (double)run[k] * (0.5 * c->raw_ntc[k] * (c->raw_ntc[k] + 1) + (double)c->raw_work_const); // (measured: + 20 better than the + 8 + 0.55 ntc the cycle count above suggests — the narrow regions are staging bound)
    work_sum += work[k], live += run[k] > 0;
  }
  HIPCHK(c->Hraw.reserve((size_t)std::max<int64_t>(total, 1)));
  HIPCHK(c->raw_featbase.reserve(fb.size()));
  HIPCHK(c->raw_dst.reserve((size_t)M));
  HIPCHK(c->raw_runs.reserve((size_t)F * feat::FY_RUNREC * 4));
  HIPCHK(c->up.put(c->raw_featbase.p, fb.data(), sizeof(int32_t) * fb.size()));
  // workgroups: one per compute unit, every live region at least one, the rest by work
  const int G = std::max(c->num_cu, live);
  int wgs[RAW_MAXCLS + 1] = {0}, given = 0;
  for (int k = 0; k <= RAW_NEG; k++)
    if (c->raw_rows[k] > 0) wgs[k] = std::max(1, (int)std::floor(work[k] / work_sum * (G - live)) + 1), given += wgs[k];
  for (int k = RAW_NEG; given > G && k >= 0; k = k > 0 ? k - 1 : RAW_NEG) // (rounding: take from the regions that have several)
    if (wgs[k] > 1) wgs[k]--, given--;
  std::vector<gram::GramRegionWG> tab;
  int tiles = 0;
  c->raw_rs.n = 0;
  for (int k = 0; k <= RAW_NEG; k++) {
    if (wgs[k] == 0) continue;
    const int64_t nchunks = (c->raw_rows[k] + gram::GR_ROWS - 1) / gram::GR_ROWS;
    const int w = (int)std::min<int64_t>(wgs[k], nchunks);
    {
      const int q = c->raw_rs.n++;
      c->raw_rs.ntc[q] = c->raw_ntc[k], c->raw_rs.rcol[q] = c->raw_rcol[k];
    }
    for (int j = 0; j < w; j++) {
      gram::GramRegionWG r;
      r.ntc = c->raw_ntc[k], r.ld = c->raw_ld[k], r.rcol = c->raw_rcol[k], r.pad = 0;
      // (k_gram_regions zeroes the LDS columns ld .. 16 ntc - 1 only, the staging writes the rest: a row must fit its region's tile columns)
      if (r.ld > 16 * r.ntc) return set_err(OVGPU_ERR_INVALID, "raw_stack_layout: a region's row stride exceeds its tile columns");
      r.h_off = c->raw_base[k], r.rows = c->raw_rows[k];
      r.chunk_begin = (int)((nchunks * j) / w), r.chunk_end = (int)((nchunks * (j + 1)) / w);
      r.part_tile = tiles, r.region = (c->raw_rs.n - 1) | (k == RAW_NEG ? 16 : 0);
      tiles += r.ntc * (r.ntc + 1) / 2;
      tab.push_back(r);
    }
  }
  c->gram_wg_n = (int)tab.size(), c->gram_wg_tiles = tiles;
  HIPCHK(c->gram_wg.reserve(tab.size()));
  HIPCHK(c->up.put(c->gram_wg.p, tab.data(), sizeof(gram::GramRegionWG) * tab.size()));
  c->raw_tables_ok = true;
  return OVGPU_OK;
}

// Host bookkeeping, workspaces and the small per-batch tables of a feature batch of F tracks / M measurements whose
// meas_offsets are `offsets` (host); the measurement payload (uv, uvn, meas_cc) is written by the caller afterwards.
static int begin_feature_batch(ovgpu_ctx *c, int F, int M, const int32_t *offsets) {
  c->have_feats = false, c->tri_readable = false; // from here on the resident batch is neither the old one nor yet the new one
  c->raw_tables_ok = false;
  int m_max = 0;
  for (int f = 0; f < F; f++) {
    const int m = offsets[f + 1] - offsets[f];
    if (m < 0) return set_err(OVGPU_ERR_INVALID, "meas_offsets not monotone");
    m_max = std::max(m_max, m);
  }
  c->F = F, c->M = M, c->m_max = m_max;
  c->have_feat_sigma = c->have_feat_mult = false; // per-feature options belong to a batch
  c->h_feat_lm.clear(), c->h_feat_rep.clear();
  c->h_offsets.assign(offsets, offsets + (F > 0 ? F + 1 : 0));
  if (F == 0) c->h_offsets.assign(1, 0);

  // chi2 table for dof 1 .. max(499, 2 m_max)  (UpdaterMSCKF.cpp:52-55; dof >= 500 is computed on the fly there, :216-222)
  const int need = std::max(500, 2 * m_max + 1);
  if ((int)c->h_chi2_table.size() < need) {
    const int old = (int)c->h_chi2_table.size();
    c->h_chi2_table.resize(need, 0.0);
    for (int i = std::max(old, 1); i < need; i++) c->h_chi2_table[i] = chi2_quantile_95(i);
  }
  c->chi2_table_len = (int)c->h_chi2_table.size();
  HIPCHK(c->chi2_table.reserve(c->chi2_table_len));

  HIPCHK(c->meas_offsets.reserve(F + 1));
  HIPCHK(c->meas_cc.reserve(M));
  HIPCHK(c->uv.reserve((size_t)2 * M));
  HIPCHK(c->uvn.reserve((size_t)2 * M));
  HIPCHK(c->pA.reserve((size_t)3 * F));
  HIPCHK(c->pG.reserve((size_t)3 * F));
  HIPCHK(c->chi2.reserve(F));
  HIPCHK(c->chi2_thr.reserve(F));
  HIPCHK(c->anchor.reserve(F));
  HIPCHK(c->anchor_pre.reserve(F));
  HIPCHK(c->status.reserve(F));

  std::vector<int32_t> order(std::max(F, 1), 0);
  track_order(offsets, F, m_max, order.data()); // longest track first
  c->h_order.assign(order.begin(), order.begin() + F);
  HIPCHK(c->sys_order.reserve(std::max(F, 1)));
  HIPCHK(c->up.put(c->sys_order.p, order.data(), sizeof(int32_t) * F));
  HIPCHK(c->up.put(c->meas_offsets.p, c->h_offsets.data(), sizeof(int32_t) * (F + 1)));
  if (c->chi2_table_dev != c->chi2_table.p || c->chi2_table_dev_len != c->chi2_table_len) { // (the table only ever grows: uploaded when it did)
    HIPCHK(c->up.put(c->chi2_table.p, c->h_chi2_table.data(), sizeof(double) * c->chi2_table_len));
    c->chi2_table_dev = c->chi2_table.p, c->chi2_table_dev_len = c->chi2_table_len;
  }
  // (host staging vectors go out of scope: the arena keeps their bytes; the scatter launch is end_feature_batch's)
  return OVGPU_OK;
}

static int end_feature_batch(ovgpu_ctx *c) {
  // rows of the stacked system: SLAM layout when landmarks are resident (the batch is for ovgpu_slam_update), MSCKF otherwise;
  // an entry point that needs the other layout switches it (set_row_layout).  With it the batch's integer tables, the triangulation's
  // anchor measurements among them (a property of the batch: k_batch_layout)
  // (... and MSCKF again under the empty active set: no landmark has a column, the batch can only be UpdaterMSCKF's or the delayed initialisation's)
  const int rcl = set_row_layout(c, c->L > 0 && !c->lm_empty_set, true);
  if (rcl != OVGPU_OK) return rcl;
  c->gram_wide_on = c->gram_wide; // "gram_wide" takes effect with a batch handed over (here) and with ovgpu_set_state, nowhere else
  c->mode_a_wide_on = c->mode_a_wide; // ... and so does "mode_a_wide"
  c->slam_mode_a_on = c->slam_mode_a; // ... and "slam_mode_a"
  c->mode_a_panel_on = c->mode_a_panel; // ... and "mode_a_panel"
  c->have_feats = true;
  c->given_tri = false;
  return OVGPU_OK;
}

static int enqueue_speculative_prior(ovgpu_ctx *c); // api_pipeline.inc
int ovgpu_set_features(ovgpu_ctx *c, const ovgpu_features_view *fv) {
  if (!c || !fv) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state must precede ovgpu_set_features");
  if (fv->F < 0 || fv->M < 0) return set_err(OVGPU_ERR_INVALID, "negative sizes");
  if (fv->F > 0 && (!fv->meas_offsets)) return set_err(OVGPU_ERR_INVALID, "null feature arrays");
  if (fv->M > 0 && (!fv->uv || !fv->uvn || !fv->clone_idx || !fv->cam_idx)) return set_err(OVGPU_ERR_INVALID, "null measurement arrays");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->up.begin());
  const int F = fv->F, M = fv->M;
  if (F > 0 && (fv->meas_offsets[0] != 0 || fv->meas_offsets[F] != M)) return set_err(OVGPU_ERR_INVALID, "meas_offsets must span [0, M]");
  // The prior block's factorisation (75 us on a dozen compute units) needs the resident state alone: it starts HERE, on the second stream, while
  // this thread packs the measurement codes and the batch crosses the bus (api_pipeline.inc; the update joins it in front of the per-feature kernel)
  if (F > 0 && M > 0) {
    const int rsp = enqueue_speculative_prior(c);
    if (rsp != OVGPU_OK) return rsp;
  }
  // packed (camera, clone) codes; the range test as ONE accumulated flag (an early return inside the loop keeps it from vectorising:
  // 0.08 ms per 100 k measurements on the caller's thread)
  // (packed straight into the page-locked arena when the scatter path is on: one pass over the caller's indices instead of a pass and a copy;
  //  a batch that fails the range test leaves the resident one untouched)
  void *cc_arena = c->up.take(sizeof(uint16_t) * (size_t)M);
  if (!cc_arena) c->h_cc.resize((size_t)std::max(M, 1));
  uint16_t *cc = cc_arena ? static_cast<uint16_t *>(cc_arena) : c->h_cc.data();
  {
    const int32_t *ci = fv->clone_idx, *ki = fv->cam_idx;
    const uint32_t nC = (uint32_t)c->C, nK = (uint32_t)c->K;
    uint32_t bad = 0;
    for (int i = 0; i < M; i++) {
      const uint32_t cl = (uint32_t)ci[i], cam = (uint32_t)ki[i]; // (a negative index is a huge unsigned one)
      bad |= (uint32_t)(cl >= nC) | (uint32_t)(cam >= nK);
      cc[i] = (uint16_t)anchor_pack(cam, cl);
    }
    if (bad) return set_err(OVGPU_ERR_INVALID, "measurement refers to an unknown clone / camera");
  }
  const int32_t zero = 0;
  int rc = begin_feature_batch(c, F, M, F > 0 ? fv->meas_offsets : &zero);
  if (rc != OVGPU_OK) return rc;
  if (cc_arena) HIPCHK(c->up.commit(c->meas_cc.p, cc_arena, sizeof(uint16_t) * (size_t)M));
  if ((rc = raw_stack_layout(c, cc)) != OVGPU_OK) return rc;
  // Order of departure (round 6): the small tables and the packed codes first — one scatter launch, then the batch's integer tables, which
  // need nothing else (end_feature_batch) —, the pixel coordinates behind them in two launches of 0.8 MB per 100 k measurements: the device
  // builds the tables and moves the first array while this thread still packs the second.
  if (!cc_arena) HIPCHK(c->up.put(c->meas_cc.p, cc, sizeof(uint16_t) * M));
  const int rce = end_feature_batch(c);
  if (rce != OVGPU_OK) return rce;
  HIPCHK(c->up.put(c->uv.p, fv->uv, sizeof(float) * 2 * M));
  HIPCHK(c->up.flush());
  HIPCHK(c->up.put(c->uvn.p, fv->uvn, sizeof(float) * 2 * M));
  // No synchronisation here (round 4): everything above left the page-locked arena asynchronously, the kernels of the update queue
  // behind the copies on the same stream, and the arena is not reused before a synchronisation has been seen (Uplink::begin appends).
  HIPCHK(c->up.flush());
  return OVGPU_OK;
}
