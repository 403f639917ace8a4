// api_slam.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): UpdaterSLAM: landmarks, ovgpu_slam_update / compress, ovgpu_slam_delayed_init, anchor changes, per-feature options.
// Shared host steps: enqueue_slam_step (one SLAM update on the stream: the single call and every chunk), state_segs / state_snapshot (the moving
// state set aside and put back: the chunked call and mode A), InitChain / begin_init_chain (the set-up of both delayed-initialisation entries).
// From api_state.inc: copy_reset_baseline, cov_resize; from api_pipeline.inc: launch_chol_fused, decode_update_flags.
// ---------------------------------------------------------------------------
// UpdaterSLAM::update (UpdaterSLAM.cpp:253-479), GLOBAL_3D landmarks
// ---------------------------------------------------------------------------
static LandmarkStore landmark_store(ovgpu_ctx *c) { return LandmarkStore{c->lm_val.p, c->lm_fej.p, c->lm_cov.p, c->lm_col.p, c->lm_anchor.p, c->lm_repd.p}; }

static int reserve_landmarks(ovgpu_ctx *c, int cap, int keep) {
  const size_t n = (size_t)std::max(cap, 1);
  HIPCHK(c->lm_val.reserve(3 * n, 3 * (size_t)keep));
  HIPCHK(c->lm_fej.reserve(3 * n, 3 * (size_t)keep));
  HIPCHK(c->lm_cov.reserve(n, keep));
  HIPCHK(c->lm_col.reserve(n, keep));
  HIPCHK(c->lm_anchor.reserve(n, keep));
  HIPCHK(c->lm_repd.reserve(n, keep));
  return OVGPU_OK;
}

int ovgpu_set_landmarks(ovgpu_ctx *c, const ovgpu_landmarks_view *lm) {
  if (!c || !lm) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state must precede ovgpu_set_landmarks");
  if (lm->L < 0 || lm->L > 4096) return set_err(OVGPU_ERR_INVALID, "bad landmark count");
  if (lm->L > 0 && (!lm->p_value || !lm->p_fej || !lm->cov_id)) return set_err(OVGPU_ERR_INVALID, "null landmark arrays");
  // the representation is the landmark's own (Landmark::_feat_representation; UpdaterSLAM.cpp:336-341), one for all without feat_rep_each
  std::vector<int32_t> reps(std::max(lm->L, 1), lm->feat_rep);
  if (lm->feat_rep_each) reps.assign(lm->feat_rep_each, lm->feat_rep_each + lm->L), reps.resize(std::max(lm->L, 1), lm->feat_rep);
  bool relative = false;
  for (int l = 0; l < std::max(lm->L, 1); l++) {
    if (reps[l] < OVGPU_REP_GLOBAL_3D || reps[l] > OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) return set_err(OVGPU_ERR_INVALID, "unknown landmark representation");
    relative = relative || (l < lm->L && reps[l] >= OVGPU_REP_ANCHORED_3D);
  }
  if (relative && (!lm->anchor_cam || !lm->anchor_clone)) return set_err(OVGPU_ERR_INVALID, "anchored landmarks need anchor_cam / anchor_clone");
  std::vector<int32_t> anc(std::max(lm->L, 1), -1);
  for (int l = 0; l < lm->L; l++) {
    if (reps[l] < OVGPU_REP_ANCHORED_3D) continue;
    if (lm->anchor_cam[l] < 0 || lm->anchor_cam[l] >= c->K || lm->anchor_clone[l] < 0 || lm->anchor_clone[l] >= c->C)
      return set_err(OVGPU_ERR_INVALID, "landmark anchor refers to an unknown clone / camera");
    anc[l] = anchor_pack(lm->anchor_cam[l], lm->anchor_clone[l]);
  }
  HIPCHK(hipSetDevice(c->device));
  c->L = lm->L;
  c->active_given = false, c->h_lm_active.clear(); // new landmarks: every one has a column block until a set is named
  c->h_lm_rep.assign(reps.begin(), reps.begin() + lm->L);
  c->row_stride = (relative || c->dopt.feat_rep >= OVGPU_REP_ANCHORED_3D) ? 72 : 48;
  c->h_lm_cov.assign(lm->cov_id, lm->cov_id + lm->L);
  c->h_lm_anchor.assign(anc.begin(), anc.begin() + lm->L);
  int rc = reserve_landmarks(c, lm->L, 0);
  if (rc != OVGPU_OK) return rc;
  if (lm->L > 0) {
    HIPCHK(upload(c->lm_val.p, lm->p_value, sizeof(double) * 3 * lm->L, c->stream));
    HIPCHK(upload(c->lm_fej.p, lm->p_fej, sizeof(double) * 3 * lm->L, c->stream));
    HIPCHK(upload(c->lm_cov.p, c->h_lm_cov.data(), sizeof(int32_t) * lm->L, c->stream));
    HIPCHK(upload(c->lm_anchor.p, anc.data(), sizeof(int32_t) * lm->L, c->stream));
    HIPCHK(upload(c->lm_repd.p, reps.data(), sizeof(int32_t) * lm->L, c->stream));
  }
  return build_columns(c); // synchronises; the feature batch has to be uploaded again (row counts and D changed)
}

// UpdaterSLAM::update's Hx_order holds the variables its batch touches (UpdaterSLAM.cpp:300-340); delayed_init's systems touch no resident
// landmark (:147-239).  The set narrows the column map to that; the other landmarks are corrected through P, as there.
int ovgpu_set_active_landmarks(ovgpu_ctx *c, int32_t n, const int32_t *lm_index) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state (and ovgpu_set_landmarks) must precede ovgpu_set_active_landmarks");
  if (n > 0 && c->L <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_landmarks must precede ovgpu_set_active_landmarks");
  if (n > 0 && !lm_index) return set_err(OVGPU_ERR_INVALID, "null lm_index");
  for (int i = 0; i < n; i++)
    if (lm_index[i] < 0 || lm_index[i] >= c->L) return set_err(OVGPU_ERR_INVALID, "active landmark index out of range");
  if (n < 0 && !c->active_given) return OVGPU_OK; // every landmark has its columns already: nothing changes, the resident batch stays
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; } // the column map changes: a prior-block factorisation started for the old one is stale
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->up.begin());
  c->active_given = n >= 0;
  c->h_lm_active.assign(n >= 0 ? c->L : 0, 0);
  for (int i = 0; i < n; i++) c->h_lm_active[lm_index[i]] = 1; // (a landmark named twice is in the set once)
  return layout_columns(c); // the feature batch has to be uploaded again (D and the LDS carve of the per-feature kernel changed)
}

int ovgpu_get_landmarks(ovgpu_ctx *c, int32_t *L_out, double *value, double *fej, int32_t *cov_id, int32_t *anchor_cam, int32_t *anchor_clone) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(c->device));
  const int L = c->L;
  if (L_out) *L_out = L;
  hipStream_t s = c->stream;
  std::vector<int32_t> anc(std::max(L, 1), -1);
  if (L > 0) {
    if (value) HIPCHK(hipMemcpyAsync(value, c->lm_val.p, sizeof(double) * 3 * L, hipMemcpyDeviceToHost, s));
    if (fej) HIPCHK(hipMemcpyAsync(fej, c->lm_fej.p, sizeof(double) * 3 * L, hipMemcpyDeviceToHost, s));
    if (cov_id) HIPCHK(hipMemcpyAsync(cov_id, c->lm_cov.p, sizeof(int32_t) * L, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(anc.data(), c->lm_anchor.p, sizeof(int32_t) * L, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(upload_sync(c, s));
  for (int l = 0; l < L; l++) {
    if (anchor_cam) anchor_cam[l] = ovg::anchor_cam(anc[l]);
    if (anchor_clone) anchor_clone[l] = ovg::anchor_clone(anc[l]);
  }
  return OVGPU_OK;
}

int ovgpu_get_landmark_reps(ovgpu_ctx *c, int32_t *L_out, int32_t *feat_rep) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (L_out) *L_out = c->L;
  for (int l = 0; l < c->L && feat_rep; l++) feat_rep[l] = c->h_lm_rep[l];
  return OVGPU_OK;
}

// One SLAM update on the stream for the F features whose landmarks lm_index_dev names: their per-feature landmark data gathered from the
// resident landmarks, the system and the EKF update, the resident landmarks' share of dx.  No upload, no wait.
static int enqueue_slam_gather(ovgpu_ctx *c, const int32_t *lm_index_dev) {
  const Batch b = batch_of(c);
  const int F = b.F;
  if (F <= 0) return OVGPU_OK;
  hipLaunchKernelGGL(k_slam_gather, dim3((F + 255) / 256), dim3(256), 0, c->stream, F, lm_index_dev, (const int32_t *)b.meas_offsets, landmark_store(c), b.pG,
                     b.pA, c->pFej.p, c->feat_lm.p, c->feat_lmcol.p, c->feat_lmcov.p, c->feat_anchor.p, c->given_status.p);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}
static int enqueue_slam_step(ovgpu_ctx *c, const int32_t *lm_index_dev) {
  int rc = enqueue_slam_gather(c, lm_index_dev);
  if (rc != OVGPU_OK || (rc = enqueue_pipeline(c, STAGE_LOCAL | STAGE_EKF, true)) != OVGPU_OK) return rc;
  hipLaunchKernelGGL(k_landmark_update, dim3((3 * c->L + 255) / 256), dim3(256), 0, c->stream, c->L, (const int32_t *)nullptr, (const int32_t *)c->lm_repd.p, c->dx.p,
                     c->lm_cov.p, c->lm_val.p, (const int32_t *)nullptr);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// per-feature landmark data of a SLAM batch, gathered on the device from the resident landmarks (`gather`; ovgpu_slam_update leaves it to
// enqueue_slam_step); the triangulation stage is replaced by the state's landmark estimates
static int slam_prepare(ovgpu_ctx *c, const int32_t *lm_index, ovgpu_update_stats *stats, bool gather = true) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (c->L <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_landmarks was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features must follow ovgpu_set_landmarks");
  if (c->F > 0 && !lm_index) return set_err(OVGPU_ERR_INVALID, "null lm_index");
  HIPCHK(hipSetDevice(c->device));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const int F = c->F;
  hipStream_t s = c->stream;
  if (c->cols_over) return set_err(OVGPU_ERR_CAPACITY, c->cols_over_msg);
  for (int f = 0; f < F; f++) {
    if (lm_index[f] < 0 || lm_index[f] >= c->L) return set_err(OVGPU_ERR_INVALID, "lm_index out of range");
    if (c->h_lm_col[lm_index[f]] < 0) return set_err(OVGPU_ERR_INVALID, "a feature of the batch observes a landmark outside the active landmark set (ovgpu_set_active_landmarks)");
  }
  const size_t n = (size_t)std::max(F, 1);
  HIPCHK(c->pFej.reserve(3 * n));
  HIPCHK(c->feat_lm.reserve(n));
  HIPCHK(c->feat_lmcol.reserve(n));
  HIPCHK(c->feat_lmcov.reserve(n));
  HIPCHK(c->feat_anchor.reserve(n));
  HIPCHK(c->lm_index.reserve(n));
  HIPCHK(c->given_status.reserve(n));
  c->h_feat_lm.assign(lm_index, lm_index + F);
  if (lm_uniform_dof(c) == 0) { // 3-dof and single-depth landmarks in one batch: the rows each feature stacks follow from its landmark
    const int rcl = set_row_layout(c, true);
    if (rcl != OVGPU_OK) return rcl;
  }
  if (F > 0) {
    HIPCHK(upload(c->lm_index.p, lm_index, sizeof(int32_t) * F, s));
    HIPCHK(upload_sync(c, s));
    const int rcg = gather ? enqueue_slam_gather(c, c->lm_index.p) : (int)OVGPU_OK;
    if (rcg != OVGPU_OK) return rcg;
  }
  c->given_tri = true; // positions come from the state: no triangulation stage
  return OVGPU_OK;
}

int ovgpu_slam_update(ovgpu_ctx *c, const int32_t *lm_index, int32_t *feat_status, double *chi2, double *chi2_thresh, double *dx, double *P_out,
                      double *lm_out, ovgpu_update_stats *stats) {
  int rc = slam_prepare(c, lm_index, stats, false);
  if (rc != OVGPU_OK) return rc;
  hipStream_t s = c->stream;
  return update_with_fallbacks(c, stats, [&]() {
    int rc2 = enqueue_slam_step(c, c->lm_index.p); // (a repeat gathers again: the failed attempt left the landmarks as they were)
    if (rc2 != OVGPU_OK) return rc2;
    PendingFeatOut pend; // one synchronisation for the per-feature outputs, the landmarks and dx / P'
    if ((rc2 = read_feature_outputs(c, feat_status, chi2, chi2_thresh, nullptr, stats, &pend, finish_update_bytes(c))) != OVGPU_OK) return rc2;
    if (lm_out) HIPCHK(hipMemcpyAsync(lm_out, c->lm_val.p, sizeof(double) * 3 * c->L, hipMemcpyDeviceToHost, s));
    return finish_update(c, dx, P_out, stats, &pend);
  });
}

int ovgpu_slam_compress(ovgpu_ctx *c, const int32_t *lm_index, int32_t *feat_status, double *chi2, double *chi2_thresh, int32_t *D_out,
                        int32_t *rows_out, int32_t *col_cov_id, double *H, double *r, ovgpu_update_stats *stats) {
  const int rc = slam_prepare(c, lm_index, stats);
  if (rc != OVGPU_OK) return rc;
  return compress_impl(c, true, feat_status, chi2, chi2_thresh, nullptr, D_out, rows_out, col_cov_id, H, r, stats);
}

// ---------------------------------------------------------------------------
// ovgpu_slam_update_chunked: the chunks of one frame's UpdaterSLAM::update (VioManager.cpp:529-547 calls it once per max_slam_in_update
// features, chunk k + 1 linearised at the state chunk k left) in ONE device pass.  The chain of ovgpu_set_active_landmarks /
// ovgpu_set_features / ovgpu_slam_update pays per chunk a host walk of the columns, the batch's uploads, a blocking upload of lm_index and a
// read-back with its synchronisation; none of it is needed between chunks: the batch, the indices and every chunk's column set are known up
// front, the host sizes follow from the integer structure, and nothing a gate decides changes what is enqueued next.  Here: one upload (the
// chunk table, every chunk's column set in column order, lm_index, the feature orders and row offsets), per chunk a Batch VALUE (sizes and
// host mirrors from the plan, the whole batch's device arrays at the chunk's offset — so a chunk's per-feature outputs land at its place in the
// whole-batch arrays — the rebased offsets of k_chunk_offsets) put in force for the chunk's launches (BatchScope), under which the single
// call's own enqueue functions run unchanged, k_chunk_collect behind each (k_slam_chunks.h), one gather and one synchronisation at the end.
// ---------------------------------------------------------------------------
namespace {
struct ChunkPlan {
  int n = 0, F = 0;
  std::vector<int32_t> first, act_off, act, D, order; // act: the chunks' column sets, concatenated, each in covariance order; order: by descending track length, per chunk
  std::vector<int32_t> h_offsets, m_max;              // the chunks' meas_offsets rebased to 0 (per chunk F_k + 1 entries, at first[k] + k) and longest tracks
  std::vector<int64_t> row_off;                       // per chunk F_k + 1 entries, at first[k] + k
  std::vector<int32_t> tab;                           // first | act | lm_index | order, as uploaded
  size_t o_act = 0, o_lm = 0, o_order = 0;
  int D_max = 0;
  int64_t rows_max = 0;
};
} // namespace

// Chunk k of the whole batch w as a value: the plan's arrays for the host mirrors, w's device arrays at the chunk's offsets
static Batch chunk_batch(const ovgpu_ctx *c, const ChunkPlan &pl, const Batch &w, int k) {
  const int f0 = pl.first[k], Fk = pl.first[k + 1] - f0, m0 = w.h_offsets[f0];
  const size_t at = (size_t)f0 + k;
  Batch b = w;
  b.F = Fk, b.M = w.h_offsets[f0 + Fk] - m0, b.m_max = pl.m_max[k], b.rows_total = pl.row_off[at + Fk];
  b.h_offsets = {pl.h_offsets.data() + at, (size_t)Fk + 1}, b.h_row_off = {pl.row_off.data() + at, (size_t)Fk + 1};
  b.h_order = {pl.order.data() + f0, (size_t)Fk}, b.h_feat_lm = {pl.tab.data() + pl.o_lm + f0, (size_t)Fk};
  b.meas_offsets = c->chk_offs.p + at, b.sys_order = c->chk_tab.p + pl.o_order + f0, b.row_off = c->chk_rowoff.p + at;
  b.meas_cc = w.meas_cc + m0, b.uv = w.uv + 2 * (size_t)m0, b.uvn = w.uvn + 2 * (size_t)m0;
  b.status = w.status + f0, b.chi2 = w.chi2 + f0, b.chi2_thr = w.chi2_thr + f0, b.pA = w.pA + 3 * (size_t)f0, b.pG = w.pG + 3 * (size_t)f0;
  if (w.have_sigma) b.feat_sigma = w.feat_sigma + f0;
  if (w.have_mult) b.feat_mult = w.feat_mult + f0;
  return b;
}

// Chunk k on the stream at the state the launches before it leave: the column map of its landmarks (k_active_columns on the resident set), its
// batch in force, the single call's gather / pipeline / landmark update, its results into slot k.  No upload, no wait.
static int enqueue_chunk(ovgpu_ctx *c, const ChunkPlan &pl, int k) {
  const int f0 = pl.first[k], Fk = pl.first[k + 1] - f0;
  if (Fk == 0) return OVGPU_OK; // an empty chunk does nothing (its dx row and flag words were zeroed with the others)
  hipStream_t s = c->stream;
  c->active_given = true;
  c->h_lm_active.assign(c->L, 0);
  for (int i = pl.act_off[k]; i < pl.act_off[k + 1]; i++) c->h_lm_active[pl.act[i]] = 1;
  int rc = layout_columns(c, false, c->chk_tab.p + pl.o_act + pl.act_off[k]);
  if (rc != OVGPU_OK) return rc;
  if (c->cols_over || c->D != pl.D[k]) return set_err(OVGPU_ERR_INVALID, "internal: a chunk's column count differs from the plan's");
  const Batch b = chunk_batch(c, pl, batch_of(c), k);
  const BatchScope in_force(c, &b);
  // the plan's rows (per landmark, from the whole batch's offsets) against the layout's rule on the batch the stages will see
  std::vector<int64_t> rows(Fk + 1);
  row_offsets_of(c, b, true, rows.data());
  for (int i = 0; i <= Fk; i++)
    if (rows[i] != b.h_row_off[i]) return set_err(OVGPU_ERR_INVALID, "internal: a chunk's row layout differs from the plan's");
  c->slam_rows = true; // (the row offsets are on the device already and the batch's tables stay: the stage's sizes alone)
  if ((rc = size_feature_stage(c)) != OVGPU_OK) return rc;
  c->have_feats = true, c->given_tri = true;
  // ---- the single call's launches
  if ((rc = enqueue_slam_step(c, c->chk_tab.p + pl.o_lm + f0)) != OVGPU_OK) return rc;
  ChunkCollect cc;
  cc.N = c->N, cc.dx = c->dx.p, cc.flags = c->flags.p, cc.gate = c->rows_used.p + 1;
  cc.dx_row = c->chk_dx.p + (size_t)k * c->N, cc.flags_out = c->chk_flags.p + 4 * k, cc.gate_out = c->chk_flags.p + 4 * pl.n + k;
  hipLaunchKernelGGL(k_chunk_collect, dim3((std::max(c->N, 5) + 255) / 256), dim3(256), 0, s, cc);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// The part of the resident state that an update moves, as k_chunk_copy's segments: P (with_P; mode A of the delayed initialisation keeps P in
// Ppad instead) | clone_qp | calib_qp | intr | lm_val.  The one place that knows this layout.
struct StateSegs {
  double *live[CHUNK_COPY_SEGS];
  size_t len[CHUNK_COPY_SEGS], total;
};
static StateSegs state_segs(const ovgpu_ctx *c, bool with_P) {
  const size_t N = (size_t)c->N, C = (size_t)c->C, K = (size_t)c->K, L = (size_t)c->L;
  StateSegs g{{c->P.p, c->clone_qp.p, c->calib_qp.p, c->intr.p, c->lm_val.p}, {with_P ? N * N : 0, 7 * C, 7 * K, 8 * K, 3 * L}, 0};
  for (size_t n : g.len) g.total += n;
  return g;
}
// those segments set aside in `save` (state_segs(..).total doubles) or, put_back, brought back from it: one launch
static int state_snapshot(ovgpu_ctx *c, double *save, bool with_P, bool put_back) {
  const StateSegs g = state_segs(c, with_P);
  ChunkCopy q;
  size_t off = 0;
  for (int i = 0; i < CHUNK_COPY_SEGS; i++) {
    q.dst[i] = put_back ? g.live[i] : save + off, q.src[i] = put_back ? save + off : g.live[i], q.n[i] = (uint32_t)g.len[i];
    off += g.len[i];
  }
  hipLaunchKernelGGL(k_chunk_copy, dim3(UP_BLOCKS, CHUNK_COPY_SEGS), dim3(256), 0, c->stream, q);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

int ovgpu_slam_update_chunked(ovgpu_ctx *c, int32_t n_chunks, const int32_t *chunk_first, const int32_t *lm_index, int32_t *feat_status, double *chi2,
                              double *chi2_thresh, double *dx_seq, double *P_out, double *lm_out, ovgpu_update_stats *stats) {
  // ---- every check, before anything changes
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (c->L <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_landmarks was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features must follow ovgpu_set_landmarks");
  if (n_chunks < 1 || n_chunks > 4096 || !chunk_first) return set_err(OVGPU_ERR_INVALID, "null chunk_first or no chunk");
  const int F = batch_of(c).F, n = n_chunks, N = c->N, L = c->L;
  if (chunk_first[0] != 0 || chunk_first[n] != F) return set_err(OVGPU_ERR_INVALID, "chunk_first must span [0, F]");
  for (int k = 0; k < n; k++)
    if (chunk_first[k + 1] < chunk_first[k]) return set_err(OVGPU_ERR_INVALID, "chunk_first not monotone");
  if (F > 0 && !lm_index) return set_err(OVGPU_ERR_INVALID, "null lm_index");
  for (int f = 0; f < F; f++)
    if (lm_index[f] < 0 || lm_index[f] >= L) return set_err(OVGPU_ERR_INVALID, "lm_index out of range");
  ChunkPlan pl;
  pl.n = n, pl.F = F;
  pl.first.assign(chunk_first, chunk_first + n + 1);
  pl.act_off.assign(n + 1, 0), pl.D.assign(n, 0), pl.m_max.assign(n, 0), pl.order.assign(std::max(F, 1), 0);
  pl.h_offsets.assign((size_t)F + n, 0), pl.row_off.assign((size_t)F + n, 0);
  {
    const HostSpan<int32_t> offs = batch_of(c).h_offsets;
    int D_fixed = 0;
    for (const auto &v : c->h_sorted) D_fixed += v.kind != COL_LANDMARK ? v.size : 0;
    std::vector<uint8_t> on(L);
    for (int k = 0; k < n; k++) {
      const int f0 = pl.first[k], Fk = pl.first[k + 1] - f0;
      std::fill(on.begin(), on.end(), 0);
      for (int f = f0; f < f0 + Fk; f++) on[lm_index[f]] = 1;
      int D = D_fixed, n_act = 0; // layout_columns' walk: the set in covariance order
      for (const auto &v : c->h_sorted)
        if (v.kind == COL_LANDMARK && on[v.index]) pl.act.push_back(v.index), D += v.size, n_act++;
      pl.act_off[k + 1] = (int32_t)pl.act.size(), pl.D[k] = D;
      if (D + 1 > 512)
        return set_err(OVGPU_ERR_CAPACITY, "chunk " + std::to_string(k) + ": its " + std::to_string(n_act) + " landmarks give " + std::to_string(D) + " Jacobian columns, more than 511");
      pl.D_max = std::max(pl.D_max, D);
      // chunk-local: the offsets, the rows (feature_rows with the landmarks named) and the order of k_system's slots (track_order)
      int32_t *ho = pl.h_offsets.data() + f0 + k;
      int64_t *ro = pl.row_off.data() + f0 + k;
      for (int i = 0; i < Fk; i++) {
        const int m = offs[f0 + i + 1] - offs[f0 + i];
        ho[i + 1] = ho[i] + m, ro[i + 1] = ro[i] + feature_rows(true, m, 3 - lm_dof(c->h_lm_rep[lm_index[f0 + i]]));
        pl.m_max[k] = std::max(pl.m_max[k], m);
      }
      pl.rows_max = std::max(pl.rows_max, ro[Fk]);
      track_order(ho, Fk, pl.m_max[k], pl.order.data() + f0);
    }
  }
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }
  HIPCHK(hipSetDevice(c->device));
  if (stats) std::memset(stats, 0, sizeof(*stats) * n);
  hipStream_t s = c->stream;
  // ---- workspaces for the largest chunk, before the first launch (a buffer that grew between two chunks would be freed under the launches)
  {
    const size_t Dm = (size_t)pl.D_max, LDm = Dm + 1, Fm = (size_t)std::max(F, 1), NTm = (LDm + 15) / 16;
    HIPCHK(c->col_cov.reserve(511));
    HIPCHK(c->col_kind.reserve(511));
    HIPCHK(c->col_sub.reserve(511));
    HIPCHK(c->col_var.reserve(511));
    HIPCHK(c->Mt.reserve(Dm * N));
    HIPCHK(c->Aaug.reserve(Dm * (Dm + N + 1)));
    HIPCHK(c->Yaug.reserve(Dm * (Dm + N + 1)));
    HIPCHK(c->Yaug2.reserve(Dm * (Dm + N + 1)));
    {
      const double *before = c->Lw.p;
      HIPCHK(c->Lw.reserve(Dm * (Dm + 8)));
      if (c->Lw.p != before) c->Lw_D = -1; // (its zeroed upper triangle went with the old buffer)
    }
    HIPCHK(c->gram_rho.reserve(std::max((size_t)N, Dm)));
    HIPCHK(c->Hbig.reserve((size_t)std::max<int64_t>(pl.rows_max, 1) * LDm));
    HIPCHK(c->gram_G.reserve(256 * NTm * NTm));
    { // every chunk's Gram stage, whatever its column count (a chunk is narrower than the widest by its landmarks' columns only, but a narrower
      // count can take a kernel that leaves MORE partial tiles): the largest of what enqueue_compress_gram reserves for 1 .. NTm tile columns
      const int64_t chunks_max = (pl.rows_max + gram::GR_ROWS - 1) / gram::GR_ROWS;
      size_t need = 0;
      for (int nt = 1; nt <= (int)NTm; nt++) need = std::max(need, gram_part_doubles(c, nt, chunks_max));
      HIPCHK(c->gram_part.reserve(need));
    }
    HIPCHK(c->pFej.reserve(3 * Fm));
    HIPCHK(c->feat_lm.reserve(Fm));
    HIPCHK(c->feat_lmcol.reserve(Fm));
    HIPCHK(c->feat_lmcov.reserve(Fm));
    HIPCHK(c->feat_anchor.reserve(Fm));
    HIPCHK(c->given_status.reserve(Fm));
    HIPCHK(c->chk_offs.reserve((size_t)F + n));
    HIPCHK(c->chk_rowoff.reserve((size_t)F + n));
    HIPCHK(c->chk_flags.reserve((size_t)5 * n));
    HIPCHK(c->chk_dx.reserve((size_t)n * N));
    HIPCHK(c->chk_save.reserve(state_segs(c, true).total));
  }
  // ---- one upload
  pl.tab.assign(pl.first.begin(), pl.first.end());
  pl.o_act = pl.tab.size(), pl.tab.insert(pl.tab.end(), pl.act.begin(), pl.act.end());
  pl.o_lm = pl.tab.size(), pl.tab.insert(pl.tab.end(), lm_index, lm_index + F);
  pl.o_order = pl.tab.size(), pl.tab.insert(pl.tab.end(), pl.order.begin(), pl.order.begin() + F);
  HIPCHK(c->chk_tab.reserve(pl.tab.size()));
  HIPCHK(c->up.begin());
  { const int rcv = upload_var_tab(c); if (rcv != OVGPU_OK) return rcv; }
  HIPCHK(c->up.put(c->chk_tab.p, pl.tab.data(), sizeof(int32_t) * pl.tab.size()));
  HIPCHK(c->up.put(c->chk_rowoff.p, pl.row_off.data(), sizeof(int64_t) * pl.row_off.size()));
  HIPCHK(c->up.flush());
  hipLaunchKernelGGL(k_chunk_offsets, dim3((F + n + 255) / 256), dim3(256), 0, s, n, F, (const int32_t *)c->chk_tab.p, (const int32_t *)batch_of(c).meas_offsets, c->chk_offs.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(c->chk_flags.p, 0, sizeof(int32_t) * 5 * n, s));
  HIPCHK(hipMemsetAsync(c->chk_dx.p, 0, sizeof(double) * (size_t)n * N, s));
  int rc = state_snapshot(c, c->chk_save.p, true, false); // the entry state, for the restore-and-chain path
  if (rc != OVGPU_OK) return rc;
  // ---- every chunk, one after the other on the stream
  const NoStageTiming untimed(c); // (no stage events inside the pass: six marker packets per chunk; ovgpu_update_stats::ms_* stay 0)
  const int64_t fused0 = c->slam_fused_batches, wide0 = c->gram_wide_updates;
  for (int k = 0; k < n && rc == OVGPU_OK; k++) rc = enqueue_chunk(c, pl, k);
  // ---- one read-back
  std::vector<int32_t> flags((size_t)5 * n, 0);
  LandLayout land;
  const size_t o_fl = land.add(sizeof(int32_t) * 5 * n), o_st = land.add(sizeof(int32_t) * F), o_c2 = land.add(sizeof(double) * F), o_th = land.add(sizeof(double) * F);
  const size_t o_dx = land.add(sizeof(double) * (size_t)n * N), o_lm = land.add(sizeof(double) * 3 * L), o_P = land.add(sizeof(double) * (size_t)N * N);
  auto gather = [&]() -> int {
    HIPCHK(c->down.reserve(land.end));
    HIPCHK(c->down.get(o_fl, c->chk_flags.p, sizeof(int32_t) * 5 * n));
    if (F > 0) {
      const Batch w = batch_of(c);
      HIPCHK(c->down.get(o_st, w.status, sizeof(int32_t) * F));
      if (chi2) HIPCHK(c->down.get(o_c2, w.chi2, sizeof(double) * F));
      if (chi2_thresh) HIPCHK(c->down.get(o_th, w.chi2_thr, sizeof(double) * F));
    }
    if (dx_seq) HIPCHK(c->down.get(o_dx, c->chk_dx.p, sizeof(double) * (size_t)n * N));
    if (lm_out) HIPCHK(c->down.get(o_lm, c->lm_val.p, sizeof(double) * 3 * L));
    if (P_out) HIPCHK(c->down.get(o_P, c->P.p, sizeof(double) * (size_t)N * N));
    HIPCHK(upload_sync(c, s)); // the ONE synchronisation of the call
    std::memcpy(flags.data(), c->down.at(o_fl), sizeof(int32_t) * 5 * n);
    return OVGPU_OK;
  };
  // on return the active set in force is "all" (the all-landmarks map leaves with the gather's launch); the batch was never anything but the
  // whole batch as uploaded: no chunk's Batch outlives enqueue_chunk
  auto leave = [&]() -> int {
    c->h_feat_lm.assign(lm_index, lm_index + F);
    c->active_given = false, c->h_lm_active.clear();
    const int rcl = layout_columns(c); // (as ovgpu_set_active_landmarks(n < 0): the batch has to be handed over again before another update)
    c->tri_readable = rcl == OVGPU_OK;
    return rcl;
  };
  if (rc != OVGPU_OK) {
    c->gram_wide_updates = wide0; // (the pass does not stand)
    (void)leave();
    (void)upload_sync(c, s);
    return rc;
  }
  if ((rc = leave()) != OVGPU_OK) return rc;
  if ((rc = gather()) != OVGPU_OK) return rc;
  int k_done = n; // chunks whose results stand
  int status = OVGPU_OK;
  bool any = false;
  for (int k = 0; k < n; k++) any = any || flags[4 * k] || flags[4 * k + 1] || flags[4 * k + 2];
  if (c->chunk_fail_inject >= 0 && c->chunk_fail_inject < n) any = true;
  c->chunk_fail_inject = -1;
  if (any) {
    // A chunk's flag word is set: a prior block that failed its pivot test (the single call repeats through the Householder route), a follower of
    // the single-launch Cholesky that timed out (it repeats with the step-wise kernels), a negative diagonal (the chain stops there).  The chunks
    // behind it ran on a state the chain would not have produced: the entry state comes back and the chunks run as the chain of single calls
    // runs them, one synchronisation and update_with_fallbacks each.  Correct, slower and rare; counted.
    c->chunk_fallbacks++;
    c->slam_fused_batches = fused0, c->gram_wide_updates = wide0; // (the pass does not stand: the chain below counts its own pipelines)
    if ((rc = state_snapshot(c, c->chk_save.p, true, true)) != OVGPU_OK) return rc;
    if ((rc = launch_build_tables(c)) != OVGPU_OK) return rc;
    HIPCHK(hipMemsetAsync(c->chk_flags.p, 0, sizeof(int32_t) * 5 * n, s));
    HIPCHK(hipMemsetAsync(c->chk_dx.p, 0, sizeof(double) * (size_t)n * N, s));
    k_done = 0;
    for (int k = 0; k < n && status == OVGPU_OK; k++) {
      int32_t fl[4] = {0, 0, 0, 0};
      status = update_with_fallbacks(c, nullptr, [&]() {
        int rc2 = enqueue_chunk(c, pl, k);
        if (rc2 != OVGPU_OK) return rc2;
        if (hipMemcpyAsync(fl, c->chk_flags.p + 4 * k, sizeof(fl), hipMemcpyDeviceToHost, s) != hipSuccess || upload_sync(c, s) != hipSuccess)
          return set_err(OVGPU_ERR_HIP, "read-back of a chunk's flag words failed");
        const std::string chunk = "chunk " + std::to_string(k) + ": ";
        return decode_update_flags(c, fl, nullptr, {CHOL_TIMED_OUT "; the state was not modified", chunk + "innovation covariance not SPD", chunk + "negative covariance diagonal after the update"});
      });
      if (status == OVGPU_OK || status == OVGPU_ERR_NEGATIVE_DIAGONAL || status == OVGPU_ERR_NOT_SPD) k_done = k + 1;
      if (stats && pl.first[k + 1] > pl.first[k]) stats[k].status = status;
    }
    const std::string msg = g_err;
    if ((rc = leave()) != OVGPU_OK) return rc;
    if ((rc = gather()) != OVGPU_OK) return rc;
    if (status != OVGPU_OK) g_err = msg;
  }
  // ---- to the caller
  {
    const double qnan = std::nan("");
    const int32_t *st = reinterpret_cast<const int32_t *>(c->down.at(o_st));
    const int Fd = pl.first[k_done];
    if (feat_status && Fd > 0) std::memcpy(feat_status, st, sizeof(int32_t) * Fd);
    if (chi2 && Fd > 0) std::memcpy(chi2, c->down.at(o_c2), sizeof(double) * Fd);
    if (chi2_thresh && Fd > 0) std::memcpy(chi2_thresh, c->down.at(o_th), sizeof(double) * Fd);
    for (int k = 0; k < k_done; k++) {
      int n_used = 0;
      int64_t rows = 0;
      for (int f = pl.first[k]; f < pl.first[k + 1]; f++) {
        if (st[f] == OVGPU_FEAT_USED) n_used++, rows += pl.row_off[(size_t)f + k + 1] - pl.row_off[(size_t)f + k];
        if (st[f] != OVGPU_FEAT_USED && st[f] != OVGPU_FEAT_CHI2_REJECTED) { // the gate is only reached by features with rows
          if (chi2) chi2[f] = qnan;
          if (chi2_thresh) chi2_thresh[f] = qnan;
        }
      }
      if (stats && pl.first[k + 1] > pl.first[k])
        stats[k].n_used = n_used, stats[k].n_rows = (int32_t)rows, stats[k].D = pl.D[k], stats[k].n_rows_comp = rows > 0 ? pl.D[k] : 0, stats[k].n_gate_bound = flags[(size_t)4 * n + k];
    }
    if (dx_seq) std::memcpy(dx_seq, c->down.at(o_dx), sizeof(double) * (size_t)n * N);
    if (lm_out) std::memcpy(lm_out, c->down.at(o_lm), sizeof(double) * 3 * L);
    if (P_out) std::memcpy(P_out, c->down.at(o_P), sizeof(double) * (size_t)N * N);
  }
  if (status != OVGPU_OK) return status;
  return check_tree_error(c);
}

// ---------------------------------------------------------------------------
// UpdaterSLAM::delayed_init (UpdaterSLAM.cpp:61-251): a chain of StateHelper::initialize calls, one feature after the
// other on the stream, no host round trip in between.  The covariance is padded to its final capacity N + 3F up front
// (the rows / columns of landmarks that do not exist yet are zero, which every kernel of the update treats exactly), the
// current dimension and landmark count live in a device counter.
// ---------------------------------------------------------------------------
// One feature of the delayed initialisation's chain (UpdaterSLAM.cpp:147-239) at the state the previous ones left: its system, StateHelper::
// initialize_invertible, the EKF update of its 2m - 3 projected rows (StateHelper.cpp:476-478) and the resident landmarks' share of it.  `exp`
// (ovgpu_slam_init_systems): the system is copied out between the first two.  Lcap: landmark slots the update kernel covers.
static int enqueue_init_feature(ovgpu_ctx *c, int f, int rep, int Nmax, int Lcap, size_t init_lds, double *dx, const InitExportParams *exp) {
  hipStream_t s = c->stream;
  const Batch b = batch_of(c);
  const int m = b.h_offsets[f + 1] - b.h_offsets[f];
  int rc = enqueue_system(c, f, rep);
  if (rc != OVGPU_OK) return rc;
  if (exp && exp->rows * std::max(exp->h, 3) > 0) {
    hipLaunchKernelGGL(k_init_export, dim3((exp->rows * std::max(exp->h, 3) + 255) / 256), dim3(256), 0, s, *exp);
    HIPCHK(hipGetLastError());
  }
  InitParams ip;
  ip.N = Nmax, ip.D = c->D, ip.LD = c->LD, ip.rep = rep, ip.f = f, ip.sz = lm_dof(rep), ip.col_cov = c->col_cov.p, ip.init_out = c->init_ws.p, ip.P = c->P.p;
  ip.sigma2 = c->dopt.sigma_pix_sq, ip.ctr = c->init_ctr.p, ip.p_FinG = b.pG, ip.p_FinA = b.pA, ip.meas_cc = b.meas_cc;
  ip.anchor_meas = c->anchor.p, ip.lm = landmark_store(c), ip.feat_slot = c->feat_slot.p;
  hipLaunchKernelGGL(k_init_invertible, dim3(1), dim3(256), init_lds, s, ip);
  HIPCHK(hipGetLastError());
  EkfJob job;
  job.R = c->Hbig.p + (size_t)b.h_row_off[f] * c->LD, job.rows = 2 * m - 3, job.pred = c->init_ctr.p + 2, job.dx = dx;
  job.keep_flags = true;
  if ((rc = enqueue_ekf(c, job)) != OVGPU_OK) return rc;
  hipLaunchKernelGGL(k_landmark_update, dim3((3 * Lcap + 255) / 256), dim3(256), 0, s, 0, (const int32_t *)(c->init_ctr.p + 1), (const int32_t *)c->lm_repd.p, job.dx,
                     c->lm_cov.p, c->lm_val.p, job.pred);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// The fused step's bound on a candidate's measurements, by ovgpu_debug_option "delayed_init_fused_long"
static int initf_m_bound(const ovgpu_ctx *c) { return c->init_fused_long ? INITF_M_MAX_LONG : INITF_M_MAX; }
// k_init_rows' carve for the batch in force: its longest track, at most the bound in force (a batch of tracks of 64 measurements at most keeps the
// carve it had before the long bound)
static int init_rows_m_max(const ovgpu_ctx *c) { return std::min(std::max(c->m_max, 1), initf_m_bound(c)); }

// The system of candidate f without its gate (k_init_rows, k_init_fused.h): enqueue_system's parameters for f_one = f, one workgroup whose carve
// holds the fused step's longest track at most
static int enqueue_init_rows(ovgpu_ctx *c, int f, int rep) {
  const Batch b = batch_of(c);
  SysParams p;
  fill_sys_params(c, b, p);
  sys_params_init_mode(c, p, f, rep);
  c->stack_is_f32 = false, c->last_stack_raw = false; // (as enqueue_system leaves them: the candidate's rows are float64 and projected)
  p.P = nullptr, p.ws = nullptr, p.init_keep = 0;      // nothing of the gate is read
  p.m_max = std::min(p.m_max, initf_m_bound(c));
  // 42496 bytes at 64 measurements and 72-double records, 152704 at 232: beyond the 64 KB a kernel may ask for by default, hence with_max_lds
  const size_t lds = init_rows_lds_layout(p.m_max, p.row_stride).total;
  if (p.row_stride > 72 || lds > (size_t)c->lds_limit) return set_err(OVGPU_ERR_INVALID, "internal: k_init_rows' carve is sized for records of 72 doubles at most, within the device's LDS");
  // a long track's phase (d) — 3m steps over LDS per column — is dealt to a workgroup per 64 columns (each repeats the phases before it: measured at
  // 232 measurements, one workgroup spent 285 us, 40 % of the step); up to 64 measurements the one workgroup the launch always had
  const int m = b.h_offsets[f + 1] - b.h_offsets[f];
  const int wgs = m > INITF_M_MAX ? (p.LD + INIT_ROWS_CPW - 1) / INIT_ROWS_CPW : 1;
  hipLaunchKernelGGL(with_max_lds<k_init_rows>(c), dim3(wgs), dim3(SYS_NT), lds, c->stream, p);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// One candidate as the fused step (k_init_fused.h): five launches, no memset (eight and the host's clears of the step words where r > 256).  The
// caller has checked initf_holds(c, m, level), the one place that knows the step's bounds: on the track (64 measurements; 232 under
// "delayed_init_fused_long"), on the factorisation (one panel of k_chol_fused up to r = 2m - 3 = 256, the two panels of k_chol_wide.h up to 461,
// each where the context's options leave it usable) and, at level 2, on k_init_rows' carve.
// level 1: k_system_t decides the gate ahead of the step; 2: k_init_rows, and the tail decides it from the factorisation's carried residual.
static bool initf_holds(const ovgpu_ctx *c, int m, int level) {
  if (m < 2 || m > initf_m_bound(c)) return false;
  const int r = 2 * m - 3;
  if (!chol_pipe_usable(c, r) && !chol_wide_usable(c, r)) return false;
  return level < 2 || (c->row_stride <= 72 && init_rows_lds_layout(init_rows_m_max(c), c->row_stride).total <= (size_t)c->lds_limit);
}
static int enqueue_init_feature_fused(ovgpu_ctx *c, int f, int rep, int Nmax, double *dx, int level) {
  hipStream_t s = c->stream;
  const Batch b = batch_of(c);
  const int m = b.h_offsets[f + 1] - b.h_offsets[f], r = 2 * m - 3;
  int rc = level >= 2 ? enqueue_init_rows(c, f, rep) : enqueue_system(c, f, rep);
  if (rc != OVGPU_OK) return rc;
  c->last_update_tform = false;
  InitFusedParams p;
  p.N = Nmax, p.D = c->D, p.LD = c->LD, p.r = r, p.LA = r + Nmax + 1, p.rep = rep, p.f = f, p.sz = lm_dof(rep);
  p.col_cov = c->col_cov.p, p.init_out = c->init_ws.p, p.stack = c->Hbig.p + (size_t)b.h_row_off[f] * c->LD, p.P = c->P.p;
  p.A = c->Aaug.p, p.Y = c->Yaug.p, p.T = c->init_ws.p + (size_t)3 * c->LD + 16, p.PLL = p.T + (size_t)3 * Nmax;
  p.sigma2 = c->dopt.sigma_pix_sq, p.ctr = c->init_ctr.p, p.dx = dx, p.flags = c->flags.p;
  p.C = c->C, p.K = c->K, p.clone_cov = c->clone_cov.p, p.calib_cov = c->calib_cov.p, p.intr_cov = c->intr_cov.p;
  p.clone_qp = c->clone_qp.p, p.calib_qp = c->calib_qp.p, p.intr = c->intr.p, p.clone_fej = c->clone_fej.p;
  p.tab_clone = c->tab_clone.p, p.tab_cam = c->tab_cam.p, p.tab_cc = c->tab_cc.p;
  p.p_FinG = b.pG, p.p_FinA = b.pA, p.meas_cc = b.meas_cc, p.anchor_meas = c->anchor.p, p.lm = landmark_store(c), p.feat_slot = c->feat_slot.p;
  // r <= 256: one panel, whose step words k_initf_s' last workgroup clears.  Beyond ("delayed_init_fused_long"): the two panels of k_chol_wide.h
  // use both sets of step words and the GO word, and enqueue_chol_wide clears the sets through ctrl_zero — k_initf_s is told to leave them alone.
  const bool wide = !chol_pipe_usable(c, r);
  const int slot = wide ? 0 : chol_next_slot(c);
  p.prog = wide ? nullptr : c->chol_prog.p + CHOL_PROG_STRIDE * slot;
  if (!wide) c->ctrl_clean &= ~(slot ? CTRL_PROG1 : CTRL_PROG0), c->ctrl_pre &= ~(slot ? CTRL_PROG1 : CTRL_PROG0); // (the step words are k_initf_s's to clear, and dirty afterwards)
  const int tn = (Nmax + 15) / 16, tw = (r + 3 + 15) / 16, tm = (r + 15) / 16;
  hipLaunchKernelGGL(k_initf_w, dim3((tw * tn + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_initf_s, dim3((tm * tw + 3) / 4 + 1), dim3(256), 0, s, p);
  if (wide) {
    // panel, Schur step, panel, place on [S | W2 | new columns | res2] (CH_SRC_MATRIX), predicated on ctr[2], the step's pivot tolerance; the
    // second panel's rows of Y, the carried residual Y[k LA + r + N] among them, are where the tails read them once k_chol_place has run
    EkfParams e;
    e.N = Nmax, e.D = r, e.DC = c->D, e.LD = c->LD, e.LA = p.LA, e.tri = 0, e.pred = c->init_ctr.p + 2, e.R = nullptr, e.col_cov = p.col_cov, e.P = p.P, e.Mt = nullptr;
    e.A = p.A, e.Y = c->Yaug.p, e.dx = dx, e.flags = c->flags.p, e.sigma2 = p.sigma2, e.diag0 = nullptr, e.pivot_tol = 1e-13, e.pred_not = nullptr;
    if ((rc = enqueue_chol_wide(c, e, s, nullptr)) != OVGPU_OK) return rc;
  } else {
    chol::CholParams q;
    q.D = r, q.LA = p.LA, q.A = p.A, q.Y = c->Yaug.p, q.Lt = nullptr, q.flags = c->flags.p, q.diag0 = nullptr, q.pivot_tol = 1e-13, q.pred = c->init_ctr.p + 2;
    q.src = chol::CH_SRC_MATRIX, q.N = Nmax, q.pred_not = nullptr;
    if ((rc = launch_chol_fused(c, q, slot, s)) != OVGPU_OK) return rc;
  }
  if (level >= 2) hipLaunchKernelGGL(k_initf_tail_gate, dim3((tn * tn + 3) / 4 + 1), dim3(256), 0, s, p, InitGateParams{b.chi2_thr, b.chi2, b.status});
  else hipLaunchKernelGGL(k_initf_tail, dim3((tn * tn + 3) / 4 + 1), dim3(256), 0, s, p);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// the representation feature f is initialised in: the call's, or ovgpu_set_feature_reps' (UpdaterSLAM.cpp:160-166: feat_rep_aruco for an
// ArUco corner, feat_rep_slam otherwise); the resident landmarks keep their own
static int feat_rep_of(const ovgpu_ctx *c, int32_t feat_rep, int f) { return ((int)c->h_feat_rep.size() == c->F && c->F > 0) ? (int)c->h_feat_rep[f] : (int)feat_rep; }

// What the chain's set-up leaves for the per-feature steps of both delayed-initialisation entries
struct InitChain {
  int N0 = 0, L0 = 0, Nmax = 0, r_max = 1; // dimension and landmarks at entry, the padded capacity, the most rows of one EKF update
  size_t init_lds = 0;                     // k_init_invertible's dynamic LDS
  std::vector<int32_t> rep;                // feat_rep_of every feature
  // mode A (ovgpu_slam_init_systems) sets these before the call; null otherwise
  double *save = nullptr;                  // the moving state is set aside here ahead of the triangulation (state_snapshot)
  const std::vector<int32_t> *up_src = nullptr; // a second upload under the set-up's one synchronisation ...
  int32_t *up_dst = nullptr;                    // ... and where it goes
};

// The chain's set-up for the features [first, F): the 48 / 72 row layout, the workspaces, the triangulation (or the caller's), P padded to the
// capacity N0 + the candidates' dof (the rows / columns of landmarks that do not exist yet are zero), the device counters, the cleared flags.
static int begin_init_chain(ovgpu_ctx *c, int32_t feat_rep, int first, bool fused, InitChain &ch) {
  const Batch b = batch_of(c); // (only fields the row layout below leaves alone are read from it)
  const int F = b.F;
  hipStream_t s = c->stream;
  ch.N0 = ch.Nmax = c->N, ch.L0 = c->L, ch.r_max = 1;
  ch.rep.assign(std::max(F, 1), feat_rep);
  for (int f = 0; f < F; f++) ch.rep[f] = feat_rep_of(c, feat_rep, f);
  bool new_anchored = false;
  for (int f = first; f < F; f++) {
    ch.Nmax += lm_dof(ch.rep[f]), new_anchored = new_anchored || ch.rep[f] >= OVGPU_REP_ANCHORED_3D;
    ch.r_max = std::max(ch.r_max, 2 * (b.h_offsets[f + 1] - b.h_offsets[f]) - 3);
  }
  // the per-feature kernel needs the anchor blocks in its row store for an anchored representation
  const int want_stride = (new_anchored || c->dopt.feat_rep >= OVGPU_REP_ANCHORED_3D || lm_any_anchored(c)) ? 72 : 48;
  if (c->slam_rows || want_stride != c->row_stride) {
    c->row_stride = want_stride;
    const int rcl = set_row_layout(c, false);
    if (rcl != OVGPU_OK) return rcl;
  }
  // ---- workspaces.  One size for every entry, the largest any of them needs: init_ws holds k_init_fused.h's T and P_LL behind the system's
  // three rows and R1, init_ctr the fused tail's arrival count in [4], dx_seq a row per feature (mode A uses the first).
  const size_t Nmax = (size_t)ch.Nmax, rD = (size_t)std::max(ch.r_max, c->D);
  int rc = reserve_landmarks(c, ch.L0 + F, ch.L0);
  if (rc != OVGPU_OK) return rc;
  HIPCHK(c->Ppad.reserve(Nmax * Nmax));
  HIPCHK(c->init_ws.reserve((size_t)3 * c->LD + 16 + 3 * Nmax + 16));
  HIPCHK(c->init_ctr.reserve(8));
  HIPCHK(c->feat_slot.reserve(std::max(F, 1)));
  HIPCHK(c->dx_seq.reserve((size_t)std::max(F, 1) * Nmax));
  if (fused) HIPCHK(c->chol_uinv.reserve((size_t)2 * 16 * 256));
  const int r_wide = std::min(ch.r_max, 2 * chol::CW_D1);
  if (fused && c->init_fused_long && chol_wide_usable(c, r_wide)) { // the second panel's compact matrices for the batch's longest track: nothing is allocated inside the chain
    const size_t D2 = (size_t)r_wide - chol::CW_D1;
    HIPCHK(c->chol_wide_A.reserve(D2 * (D2 + Nmax + 1)));
    HIPCHK(c->chol_wide_Y.reserve(D2 * (D2 + Nmax + 1)));
  }
  HIPCHK(c->Mt.reserve(rD * Nmax));
  HIPCHK(c->Aaug.reserve(rD * (rD + Nmax + 1)));
  HIPCHK(c->Yaug.reserve(rD * (rD + Nmax + 1)));
  HIPCHK(c->dx.reserve(Nmax));
  if (ch.save && (rc = state_snapshot(c, ch.save, false, false)) != OVGPU_OK) return rc;
  // ---- triangulate every feature against the clone poses at entry (UpdaterSLAM.cpp:121-144), or take the caller's (ovgpu_set_triangulation)
  if (!c->given_tri) {
    if ((rc = enqueue_triangulate(c)) != OVGPU_OK) return rc;
  } else if (F > 0) {
    HIPCHK(hipMemcpyAsync(b.status, c->given_status.p, sizeof(int32_t) * F, hipMemcpyDeviceToDevice, s));
  }
  if ((rc = cov_resize(c, ch.N0, ch.Nmax, ch.N0)) != OVGPU_OK) return rc; // (the entry's P waits in Ppad)
  const int32_t ctr0[8] = {ch.N0, ch.L0, 0, 0, 0, 0, 0, 0};
  HIPCHK(upload(c->init_ctr.p, ctr0, sizeof(ctr0), s));
  if (ch.up_src && !ch.up_src->empty()) HIPCHK(upload(ch.up_dst, ch.up_src->data(), sizeof(int32_t) * ch.up_src->size(), s));
  HIPCHK(upload_sync(c, s)); // ctr0 is a stack variable
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), s));
  if (!ch.save) HIPCHK(hipMemsetAsync(c->dx_seq.p, 0, sizeof(double) * (size_t)std::max(F, 1) * Nmax, s)); // (mode A hands no dx out)
  HIPCHK(hipMemsetAsync(c->feat_slot.p, 0xFF, sizeof(int32_t) * std::max(F, 1), s));
  ch.init_lds = ((size_t)3 * c->LD + 3 * Nmax + 16) * sizeof(double);
  return OVGPU_OK;
}

// ovgpu_slam_delayed_init (fused = false) and ovgpu_slam_delayed_init_fused: one body, the step per candidate differs
static int delayed_init_impl(ovgpu_ctx *c, bool fused, int32_t feat_rep, int32_t *feat_status, double *chi2, double *chi2_thresh, int32_t *lm_cov_id,
                             double *lm_value, double *lm_fej, int32_t *anchor_cam, int32_t *anchor_clone, double *dx_seq, int32_t *N_out,
                             double *P_out, ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features was never called (or the state changed since)");
  if (feat_rep < OVGPU_REP_GLOBAL_3D || feat_rep > OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE)
    return set_err(OVGPU_ERR_INVALID, "unknown landmark representation");
  if (c->cols_over) return set_err(OVGPU_ERR_CAPACITY, c->cols_over_msg);
  HIPCHK(hipSetDevice(c->device));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  InitChain ch;
  int rc = begin_init_chain(c, feat_rep, 0, fused, ch);
  if (rc != OVGPU_OK) return rc;
  const Batch b = batch_of(c); // (as the chain's set-up laid it out)
  const int F = b.F, N0 = ch.N0, L0 = ch.L0, Nmax = ch.Nmax;
  hipStream_t s = c->stream;
  // ---- 4. one feature after the other (UpdaterSLAM.cpp:147-239)
  for (int f = 0; f < F && rc == OVGPU_OK; f++) {
    const int m = b.h_offsets[f + 1] - b.h_offsets[f];
    if (m < 2) continue; // :91-93, flagged OVGPU_FEAT_TOO_FEW_MEAS by the triangulation
    if (fused && c->init_fused > 0 && initf_holds(c, m, c->init_fused)) {
      rc = enqueue_init_feature_fused(c, f, ch.rep[f], Nmax, c->dx_seq.p + (size_t)f * Nmax, c->init_fused);
      c->init_fused_steps++;
      if (c->init_fused >= 2) c->init_rows_steps++;
      if (m > INITF_M_MAX) c->init_long_steps++;
      continue;
    }
    rc = enqueue_init_feature(c, f, ch.rep[f], Nmax, L0 + F, ch.init_lds, c->dx_seq.p + (size_t)f * Nmax, nullptr);
    if (fused) c->init_chain_steps++; // (a track beyond the fused step's bound, a factorisation the step cannot take, or "delayed_init_fused" = 0)
  }
  // ---- results
  int32_t ctr[4] = {N0, L0, 0, 0};
  std::vector<int32_t> slot(std::max(F, 1), -1);
  if (rc == OVGPU_OK) {
    HIPCHK(hipMemcpyAsync(ctr, c->init_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
    if (F > 0) HIPCHK(hipMemcpyAsync(slot.data(), c->feat_slot.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
  } else {
    (void)upload_sync(c, s);
  }
  const int N1 = ctr[0], L1 = ctr[1];
  // covariance back to its own leading dimension; it is the new baseline of ovgpu_reset_state as well
  {
    int rcb = cov_resize(c, N1, N1, Nmax);
    if (rcb != OVGPU_OK || (rcb = copy_reset_baseline(c)) != OVGPU_OK) return rcb;
  }
  if (rc != OVGPU_OK) return rc;
  std::vector<double> val(3 * (size_t)std::max(L1, 1)), fej(3 * (size_t)std::max(L1, 1));
  std::vector<int32_t> cov(std::max(L1, 1)), anc(std::max(L1, 1));
  if (L1 > 0) {
    HIPCHK(hipMemcpyAsync(val.data(), c->lm_val.p, sizeof(double) * 3 * L1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fej.data(), c->lm_fej.p, sizeof(double) * 3 * L1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cov.data(), c->lm_cov.p, sizeof(int32_t) * L1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(anc.data(), c->lm_anchor.p, sizeof(int32_t) * L1, hipMemcpyDeviceToHost, s));
  }
  if (dx_seq && F > 0) HIPCHK(hipMemcpyAsync(dx_seq, c->dx_seq.p, sizeof(double) * (size_t)F * Nmax, hipMemcpyDeviceToHost, s));
  if (P_out) HIPCHK(hipMemcpyAsync(P_out, c->P.p, sizeof(double) * (size_t)N1 * N1, hipMemcpyDeviceToHost, s));
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
  std::vector<int32_t> tri_am(std::max(F, 1), -1);
  std::vector<uint16_t> tri_cc(std::max(b.M, 1), 0);
  if (F > 0 && (!c->given_tri || c->given_has_anchor)) HIPCHK(hipMemcpyAsync(tri_am.data(), c->anchor.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
  if (b.M > 0) HIPCHK(hipMemcpyAsync(tri_cc.data(), b.meas_cc, sizeof(uint16_t) * b.M, hipMemcpyDeviceToHost, s));
  c->slam_rows = false;
  rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, nullptr, stats); // synchronises
  if (rc != OVGPU_OK) return rc;
  const double qnan = std::nan("");
  for (int f = 0; f < F; f++) {
    const int l = slot[f];
    if (lm_cov_id) lm_cov_id[f] = l >= 0 ? cov[l] : -1;
    for (int i = 0; i < 3; i++) {
      if (lm_value) lm_value[3 * f + i] = l >= 0 ? val[3 * l + i] : qnan;
      if (lm_fej) lm_fej[3 * f + i] = l >= 0 ? fej[3 * l + i] : qnan;
    }
    // anchored landmark: its anchor; otherwise the anchor of the triangulation (FeatureInitializer.cpp:36-46 writes it into the
    // Feature for every representation, and UpdaterSLAM.cpp:214 takes Landmark::_unique_camera_id from it)
    const int tri_anchor = (f < (int)tri_am.size() && tri_am[f] >= 0 && tri_am[f] < (int)tri_cc.size()) ? (int)tri_cc[tri_am[f]] : -1;
    const int a = (l >= 0 && anc[l] >= 0) ? anc[l] : tri_anchor;
    if (anchor_cam) anchor_cam[f] = ovg::anchor_cam(a);
    if (anchor_clone) anchor_clone[f] = ovg::anchor_clone(a);
  }
  if (N_out) *N_out = N1;
  if (stats) stats->n_used = L1 - L0, stats->D = c->D;
  // the new landmarks join the resident ones and the column map
  c->L = L1;
  c->h_lm_rep.resize(L1, feat_rep);
  for (int f = 0; f < F; f++)
    if (slot[f] >= L0 && slot[f] < L1) c->h_lm_rep[slot[f]] = ch.rep[f];
  c->h_lm_cov.assign(cov.begin(), cov.begin() + L1);
  c->h_lm_anchor.assign(anc.begin(), anc.begin() + L1);
  c->dx.release(), c->Mt.release(), c->Aaug.release(), c->Yaug.release(); // sized by the old N below
  HIPCHK(c->dx.reserve(N1));
  rc = build_columns(c);
  if (rc != OVGPU_OK) return rc;
  c->tri_readable = true; // include/ovgpu.h: ovgpu_get_triangulation reads the triangulation of THIS call (the shim's delayed_init needs it for the Feature side effects)
  return decode_update_flags(c, flags, stats, UPDATE_FLAG_TEXT);
}

int ovgpu_slam_delayed_init(ovgpu_ctx *c, int32_t feat_rep, int32_t *feat_status, double *chi2, double *chi2_thresh, int32_t *lm_cov_id,
                            double *lm_value, double *lm_fej, int32_t *anchor_cam, int32_t *anchor_clone, double *dx_seq, int32_t *N_out,
                            double *P_out, ovgpu_update_stats *stats) {
  return delayed_init_impl(c, false, feat_rep, feat_status, chi2, chi2_thresh, lm_cov_id, lm_value, lm_fej, anchor_cam, anchor_clone, dx_seq, N_out, P_out, stats);
}

// The same call with every candidate the fused step holds (initf_holds: m <= INITF_M_MAX, or INITF_M_MAX_LONG under "delayed_init_fused_long")
// run as five launches (eight beyond r = 256); the others take enqueue_init_feature where they stand in the chain.
int ovgpu_slam_delayed_init_fused(ovgpu_ctx *c, int32_t feat_rep, int32_t *feat_status, double *chi2, double *chi2_thresh, int32_t *lm_cov_id,
                                  double *lm_value, double *lm_fej, int32_t *anchor_cam, int32_t *anchor_clone, double *dx_seq, int32_t *N_out,
                                  double *P_out, ovgpu_update_stats *stats) {
  return delayed_init_impl(c, true, feat_rep, feat_status, chi2, chi2_thresh, lm_cov_id, lm_value, lm_fej, anchor_cam, anchor_clone, dx_seq, N_out, P_out, stats);
}


// ---------------------------------------------------------------------------
// Mode A of UpdaterSLAM::delayed_init: the chain of ovgpu_slam_delayed_init run speculatively on scratch copies, every feature's
// system exported in the form StateHelper::initialize takes (k_init_export).  The host replays the systems through its own
// initialize and calls again from the feature after the first one whose gate it decided differently.
// ---------------------------------------------------------------------------
// The ragged outputs' layout, from the batch alone: every feature from `first` on with two measurements or more gets 2m rows (2m - 2 for
// the single depth) and the variables its measurements touch (UpdaterHelper::get_feature_jacobian_full's Hx_order: the clones, the
// extrinsics and intrinsics of the observing cameras that the state estimates; an anchor is one of the feature's own clones / cameras),
// ordered by covariance id.  Reads the packed measurement codes back (one synchronisation).
struct InitSysLayout {
  ovgpu_init_sizes tot{};
  std::vector<int32_t> rows, nvar, h, var_id, var_size, cols; // cols: the context's column of every H_x column, feature after feature
  std::vector<int64_t> var_off, hx_off, hf_off, res_off, col_off;
};
static int init_sys_layout(ovgpu_ctx *c, int32_t feat_rep, int first, InitSysLayout &lo) {
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features was never called (or the state changed since)");
  if (feat_rep < OVGPU_REP_GLOBAL_3D || feat_rep > OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) return set_err(OVGPU_ERR_INVALID, "unknown landmark representation");
  const Batch b = batch_of(c);
  const int F = b.F, M = b.M;
  if (first < 0 || first > F) return set_err(OVGPU_ERR_INVALID, "first_feature out of range");
  if (c->cols_over) return set_err(OVGPU_ERR_CAPACITY, c->cols_over_msg);
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint16_t> cc(std::max(M, 1));
  if (M > 0) HIPCHK(hipMemcpyAsync(cc.data(), b.meas_cc, sizeof(uint16_t) * M, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(upload_sync(c, c->stream));
  std::vector<int32_t> col_of(std::max(c->N, 1), -1);
  for (int j = 0; j < c->D; j++) col_of[c->h_col_cov[j]] = j;
  lo = InitSysLayout();
  lo.rows.assign(F, 0), lo.nvar.assign(F, 0), lo.h.assign(F, 0);
  lo.var_off.assign(F, 0), lo.hx_off.assign(F, 0), lo.hf_off.assign(F, 0), lo.res_off.assign(F, 0), lo.col_off.assign(F, 0);
  std::vector<std::pair<int32_t, int32_t>> vars; // (covariance id, size)
  std::vector<char> seen_clone(c->C), seen_cam(c->K);
  for (int f = 0; f < F; f++) {
    lo.var_off[f] = lo.tot.n_vars, lo.hx_off[f] = lo.tot.n_hx, lo.hf_off[f] = lo.tot.n_hf, lo.res_off[f] = lo.tot.n_res, lo.col_off[f] = (int64_t)lo.cols.size();
    const int m = b.h_offsets[f + 1] - b.h_offsets[f];
    if (f < first || m < 2) continue;
    const bool single = feat_rep_of(c, feat_rep, f) == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE;
    vars.clear();
    std::fill(seen_clone.begin(), seen_clone.end(), 0), std::fill(seen_cam.begin(), seen_cam.end(), 0);
    for (int i = b.h_offsets[f]; i < b.h_offsets[f + 1]; i++) {
      const int cam = anchor_cam(cc[i]), cl = anchor_clone(cc[i]);
      if (!seen_clone[cl]) seen_clone[cl] = 1, vars.push_back({c->h_clone_cov[cl], 6});
      if (!seen_cam[cam]) {
        seen_cam[cam] = 1;
        if (c->h_calib_cov[cam] >= 0) vars.push_back({c->h_calib_cov[cam], 6});
        if (c->h_intr_cov[cam] >= 0) vars.push_back({c->h_intr_cov[cam], 8});
      }
    }
    std::sort(vars.begin(), vars.end());
    int h = 0;
    for (const auto &v : vars) {
      lo.var_id.push_back(v.first), lo.var_size.push_back(v.second);
      for (int i = 0; i < v.second; i++) lo.cols.push_back(col_of[v.first + i]);
      h += v.second;
    }
    const int rows = single ? 2 * m - 2 : 2 * m;
    lo.rows[f] = rows, lo.nvar[f] = (int)vars.size(), lo.h[f] = h;
    lo.tot.n_vars += (int64_t)vars.size(), lo.tot.n_hx += (int64_t)rows * h, lo.tot.n_hf += (int64_t)rows * (single ? 1 : 3), lo.tot.n_res += rows;
  }
  return OVGPU_OK;
}

int ovgpu_slam_init_systems_len(ovgpu_ctx *c, int32_t feat_rep, int32_t first_feature, ovgpu_init_sizes *sizes) {
  if (!c || !sizes) return set_err(OVGPU_ERR_INVALID, "null argument");
  InitSysLayout lo;
  const int rc = init_sys_layout(c, feat_rep, first_feature, lo);
  if (rc != OVGPU_OK) return rc;
  *sizes = lo.tot;
  return OVGPU_OK;
}

int ovgpu_slam_init_systems(ovgpu_ctx *c, int32_t feat_rep, int32_t first_feature, const ovgpu_init_sizes *cap, ovgpu_init_system *sys, int32_t *var_id,
                            int32_t *var_size, double *H_x, double *H_f, double *res, ovgpu_update_stats *stats) {
  if (!c || !cap) return set_err(OVGPU_ERR_INVALID, "null argument");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the chain uses the factorisation's work matrices
  InitSysLayout lo;
  int rc = init_sys_layout(c, feat_rep, first_feature, lo);
  if (rc != OVGPU_OK) return rc;
  const int F = batch_of(c).F, first = first_feature;
  if (F > 0 && !sys) return set_err(OVGPU_ERR_INVALID, "null sys");
  if ((lo.tot.n_vars > 0 && (!var_id || !var_size)) || (lo.tot.n_hx > 0 && !H_x) || (lo.tot.n_hf > 0 && (!H_f || !res)))
    return set_err(OVGPU_ERR_INVALID, "null output arrays");
  if (cap->n_vars < lo.tot.n_vars || cap->n_hx < lo.tot.n_hx || cap->n_hf < lo.tot.n_hf || cap->n_res < lo.tot.n_res)
    return set_err(OVGPU_ERR_CAPACITY, "output capacities below ovgpu_slam_init_systems_len");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  hipStream_t s = c->stream;
  // the row layout of the delayed initialisation (as ovgpu_slam_delayed_init); the batch's own is put back at the end
  const int stride0 = c->row_stride;
  const bool slam_rows0 = c->slam_rows;
  // ---- what the chain moves, kept aside: clones, calibration, intrinsics, the resident landmarks' values (P waits in Ppad)
  const size_t n_out = (size_t)(lo.tot.n_hx + lo.tot.n_hf + lo.tot.n_res);
  HIPCHK(c->isx_arena.reserve(std::max<size_t>(n_out, 1)));
  HIPCHK(c->isx_cols.reserve(std::max<size_t>(lo.cols.size(), 1)));
  HIPCHK(c->isx_save.reserve(state_segs(c, false).total));
  InitChain ch;
  ch.save = c->isx_save.p, ch.up_src = &lo.cols, ch.up_dst = c->isx_cols.p;
  if ((rc = begin_init_chain(c, feat_rep, first, false, ch)) != OVGPU_OK) return rc;
  const Batch b = batch_of(c); // (as the chain's set-up laid it out; the device arrays and offsets are the same under the layout put back below)
  double *a_hx = c->isx_arena.p, *a_hf = a_hx + lo.tot.n_hx, *a_res = a_hf + lo.tot.n_hf;
  c->init_export = true;
  for (int f = first; f < F && rc == OVGPU_OK; f++) {
    if (lo.rows[f] == 0) continue; // fewer than two measurements: OVGPU_FEAT_TOO_FEW_MEAS
    InitExportParams ep;
    ep.LD = c->LD, ep.D = c->D, ep.h = lo.h[f], ep.rows = lo.rows[f], ep.single = ch.rep[f] == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE, ep.f = f;
    ep.init_out = c->init_ws.p, ep.stack = c->Hbig.p + (size_t)b.h_row_off[f] * c->LD, ep.cols = c->isx_cols.p + lo.col_off[f];
    ep.feat_sigma = b.have_sigma ? b.feat_sigma : nullptr, ep.sigma = std::sqrt(c->dopt.sigma_pix_sq);
    ep.Hx = a_hx + lo.hx_off[f], ep.Hf = a_hf + lo.hf_off[f], ep.res = a_res + lo.res_off[f];
    rc = enqueue_init_feature(c, f, ch.rep[f], ch.Nmax, ch.L0 + F, ch.init_lds, c->dx_seq.p, &ep);
  }
  c->init_export = false;
  // ---- results: one gather, one synchronisation
  std::vector<int32_t> st(std::max(F, 1), OVGPU_FEAT_TOO_FEW_MEAS), am(std::max(F, 1), -1), slot(std::max(F, 1), -1);
  std::vector<double> x2(std::max(F, 1)), thr(std::max(F, 1)), pA(3 * (size_t)std::max(F, 1)), pG(3 * (size_t)std::max(F, 1));
  std::vector<uint16_t> cc(std::max(b.M, 1), 0);
  int32_t flags[4] = {0, 0, 0, 0};
  if (rc == OVGPU_OK && F > 0) {
    HIPCHK(hipMemcpyAsync(st.data(), b.status, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(x2.data(), b.chi2, sizeof(double) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(thr.data(), b.chi2_thr, sizeof(double) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(slot.data(), c->feat_slot.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pA.data(), b.pA, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pG.data(), b.pG, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (!c->given_tri || c->given_has_anchor) HIPCHK(hipMemcpyAsync(am.data(), c->anchor.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    if (b.M > 0) HIPCHK(hipMemcpyAsync(cc.data(), b.meas_cc, sizeof(uint16_t) * b.M, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
    if (lo.tot.n_hx > 0) HIPCHK(hipMemcpyAsync(H_x, a_hx, sizeof(double) * lo.tot.n_hx, hipMemcpyDeviceToHost, s));
    if (lo.tot.n_hf > 0) HIPCHK(hipMemcpyAsync(H_f, a_hf, sizeof(double) * lo.tot.n_hf, hipMemcpyDeviceToHost, s));
    if (lo.tot.n_res > 0) HIPCHK(hipMemcpyAsync(res, a_res, sizeof(double) * lo.tot.n_res, hipMemcpyDeviceToHost, s));
  }
  // ---- the resident state as it was: P back from Ppad, the saved values, the pose tables, the batch's row layout
  std::swap(c->P, c->Ppad); // (undoes begin_init_chain's cov_resize: no copy, the entry's P was never written)
  c->N = ch.N0;
  {
    const int rcs = state_snapshot(c, c->isx_save.p, false, true);
    if (rc == OVGPU_OK) rc = rcs;
  }
  {
    const int rct = launch_build_tables(c);
    if (rc == OVGPU_OK) rc = rct;
  }
  if (c->row_stride != stride0 || c->slam_rows != slam_rows0) {
    c->row_stride = stride0;
    const int rcl = set_row_layout(c, slam_rows0);
    if (rc == OVGPU_OK) rc = rcl;
  }
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), s));
  c->ctrl_pre = 0; // the chain used the control block: the next update zeroes what it needs itself
  HIPCHK(upload_sync(c, s));
  if (rc != OVGPU_OK) return rc;
  // ---- per feature
  const double qnan = std::nan("");
  for (int i = 0; i < lo.tot.n_vars; i++) var_id[i] = lo.var_id[i], var_size[i] = lo.var_size[i];
  int n_acc = 0;
  for (int f = 0; f < F; f++) {
    ovgpu_init_system &o = sys[f];
    std::memset(&o, 0, sizeof(o));
    o.feat_rep = ch.rep[f];
    o.var_off = lo.var_off[f], o.hx_off = lo.hx_off[f], o.hf_off = lo.hf_off[f], o.res_off = lo.res_off[f];
    o.chi2 = o.chi2_thresh = qnan;
    o.anchor_cam = o.anchor_clone = -1;
    if (f < first) {
      o.status = -1;
      continue;
    }
    const int m = b.h_offsets[f + 1] - b.h_offsets[f];
    o.status = m < 2 ? OVGPU_FEAT_TOO_FEW_MEAS : st[f];
    const bool has_system = lo.rows[f] > 0 && (o.status == OVGPU_FEAT_USED || o.status == OVGPU_FEAT_CHI2_REJECTED);
    if (has_system) {
      o.rows = lo.rows[f], o.n_vars = lo.nvar[f], o.h = lo.h[f], o.cols_f = o.feat_rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? 1 : 3;
      o.chi2 = x2[f], o.chi2_thresh = thr[f];
    }
    n_acc += slot[f] >= 0;
    if (am[f] >= 0 && am[f] < b.M) o.anchor_cam = anchor_cam(cc[am[f]]), o.anchor_clone = anchor_clone(cc[am[f]]);
    const double *p = (o.feat_rep >= OVGPU_REP_ANCHORED_3D ? pA.data() : pG.data()) + 3 * f;
    for (int i = 0; i < 3; i++) o.p_seed[i] = p[i];
  }
  if (stats) stats->n_used = n_acc, stats->D = c->D;
  return decode_update_flags(c, flags, stats, {CHOL_TIMED_OUT CHOL_STEPWISE_HINT, "innovation covariance not SPD in the chain", "negative covariance diagonal in the chain"});
}

// ---------------------------------------------------------------------------
// Window bookkeeping on the resident covariance (SURVEY.md 8f N3): StateHelper::marginalize, clone / augment_clone,
// EKFPropagation.  The host keeps the covariance ids of the resident variables; the kernels move the data.
// ---------------------------------------------------------------------------
// h_vars, the device copies of the ids, the column map, the pose tables and the reset baseline after a structural change
static int rebuild_variables(ovgpu_ctx *c) {
  const int C = c->C, K = c->K, N = c->N;
  c->h_vars.clear();
  for (int k = 0; k < K; k++) {
    if (c->h_calib_cov[k] >= 0) c->h_vars.push_back({c->h_calib_cov[k], 6, COL_CALIB_POSE, k});
    if (c->h_intr_cov[k] >= 0) c->h_vars.push_back({c->h_intr_cov[k], 8, COL_CALIB_INTR, k});
  }
  for (int i = 0; i < C; i++) c->h_vars.push_back({c->h_clone_cov[i], 6, COL_CLONE, i});
  hipStream_t s = c->stream;
  HIPCHK(c->clone_cov.reserve(C));
  HIPCHK(c->clone_col.reserve(C));
  HIPCHK(upload(c->clone_cov.p, c->h_clone_cov.data(), sizeof(int32_t) * C, s));
  HIPCHK(upload(c->calib_cov.p, c->h_calib_cov.data(), sizeof(int32_t) * K, s));
  HIPCHK(upload(c->intr_cov.p, c->h_intr_cov.data(), sizeof(int32_t) * K, s));
  if (c->L > 0) HIPCHK(upload(c->lm_cov.p, c->h_lm_cov.data(), sizeof(int32_t) * c->L, s));
  HIPCHK(c->tab_clone.reserve(24 * (size_t)C));
  HIPCHK(c->tab_cc.reserve((size_t)12 * K * C));
  HIPCHK(c->dx.reserve(N));
  int rc = build_columns(c); // synchronises
  if (rc != OVGPU_OK) return rc;
  if ((rc = copy_reset_baseline(c)) != OVGPU_OK) return rc;
  return launch_build_tables(c);
}

// UpdaterSLAM::perform_anchor_change: k_anchor_change builds Phi and rewrites the landmark, k_cov_propagate applies it (Q = 0)
static int enqueue_anchor_change(ovgpu_ctx *c, int l, int new_cam, int new_clone) {
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }
  const int32_t old = c->h_lm_anchor[l];
  const int old_cam = anchor_cam(old);
  const int lsz = lm_dof(c->h_lm_rep[l]);
  int n_old = 6 + 6 + lsz;
  if (c->h_calib_cov[old_cam] >= 0) n_old += 6;
  if (c->h_calib_cov[new_cam] >= 0 && new_cam != old_cam) n_old += 6;
  hipStream_t s = c->stream;
  const int N = c->N;
  HIPCHK(c->prop_in.reserve(3 * 27 + 9));
  HIPCHK(c->prop_ids.reserve(28));
  HIPCHK(c->prop_w.reserve((size_t)N * 3 + 9));
  double *dPhi = c->prop_in.p, *dQ = dPhi + 3 * 27, *W = c->prop_w.p, *PCP = W + (size_t)N * 3;
  HIPCHK(hipMemsetAsync(dQ, 0, 9 * sizeof(double), s));
  AnchorParams ap;
  ap.rep = c->h_lm_rep[l], ap.do_fej = c->dopt.do_fej, ap.l = l, ap.new_cam = new_cam, ap.new_clone = new_clone, ap.sz = lsz;
  ap.tab_clone = c->tab_clone.p, ap.tab_cam = c->tab_cam.p, ap.clone_cov = c->clone_cov.p, ap.calib_cov = c->calib_cov.p;
  ap.lm = landmark_store(c), ap.phi = dPhi, ap.ids = c->prop_ids.p, ap.n_old = c->prop_ids.p + 27;
  hipLaunchKernelGGL(k_anchor_change, dim3(1), dim3(64), 0, s, ap);
  for (int pass = 0; pass < 3; pass++) {
    const int n = pass == 1 ? lsz * lsz : N * lsz;
    hipLaunchKernelGGL(k_cov_propagate, dim3((n + 255) / 256), dim3(256), 0, s, N, (int)c->h_lm_cov[l], lsz, n_old, c->prop_ids.p, dPhi, dQ, c->P.p, W, PCP,
                       c->flags.p, pass);
  }
  HIPCHK(hipGetLastError());
  c->h_lm_anchor[l] = anchor_pack(new_cam, new_clone);
  return OVGPU_OK;
}

static int anchor_change_checks(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (c->L <= 0) return set_err(OVGPU_ERR_NO_STATE, "no resident landmarks");
  HIPCHK(hipSetDevice(c->device));
  return OVGPU_OK;
}

int ovgpu_slam_change_anchor(ovgpu_ctx *c, int32_t lm_index, int32_t new_anchor_cam, int32_t new_anchor_clone) {
  int rc = anchor_change_checks(c);
  if (rc != OVGPU_OK) return rc;
  if (lm_index < 0 || lm_index >= c->L || new_anchor_cam < 0 || new_anchor_cam >= c->K || new_anchor_clone < 0 || new_anchor_clone >= c->C)
    return set_err(OVGPU_ERR_INVALID, "landmark / camera / clone index out of range");
  if (c->h_lm_rep[lm_index] < OVGPU_REP_ANCHORED_3D) return set_err(OVGPU_ERR_INVALID, "the landmark is not anchored");
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), c->stream));
  return enqueue_anchor_change(c, lm_index, new_anchor_cam, new_anchor_clone);
}

int ovgpu_slam_change_anchors(ovgpu_ctx *c, int32_t marg_clone, int32_t new_clone, int32_t *n_changed) {
  if (n_changed) *n_changed = 0;
  if (c && c->have_state && !c->poses_only && (c->L <= 0 || !lm_any_anchored(c))) return OVGPU_OK; // :493-496: global landmarks are skipped
  int rc = anchor_change_checks(c);
  if (rc != OVGPU_OK) return rc;
  if (marg_clone < 0 || marg_clone >= c->C || new_clone < 0 || new_clone >= c->C || marg_clone == new_clone)
    return set_err(OVGPU_ERR_INVALID, "clone index out of range");
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), c->stream));
  int n = 0;
  for (int l = 0; l < c->L; l++) {
    const int32_t a = c->h_lm_anchor[l];
    if (anchor_clone(a) != marg_clone) continue;
    if ((rc = enqueue_anchor_change(c, l, anchor_cam(a), new_clone)) != OVGPU_OK) return rc; // same camera (:499-500)
    n++;
  }
  if (n_changed) *n_changed = n;
  return OVGPU_OK;
}

// ---------------------------------------------------------------------------
// UpdaterSLAM::change_anchors for all moving landmarks at once: k_anchor_change_all + k_cov_propagate_multi (mode B), or the first alone
// with its outputs handed to the host (mode A)
// ---------------------------------------------------------------------------
// The landmarks anchored in marg_clone, in landmark order, and the ragged layout of what the kernels write for them (host prefix sums)
struct AnchorBatchPlan {
  int n = 0, S = 0;              // moving landmarks, the sum of their dof
  int64_t n_ids = 0, n_phi = 0;  // sum of n_old, sum of dof * n_old
  int64_t n_vars = 0;
  std::vector<int32_t> tab;      // 8 ints per landmark (k_anchor_change_all)
};
// ovgpu_slam_change_anchors' checks; *none = there is nothing to move and the call returns OVGPU_OK (:493-496: global landmarks are skipped)
static int anchor_batch_plan(ovgpu_ctx *c, int marg_clone, int new_clone, AnchorBatchPlan &pl, bool *none) {
  *none = false;
  if (c && c->have_state && !c->poses_only && (c->L <= 0 || !lm_any_anchored(c))) {
    *none = true;
    return OVGPU_OK;
  }
  int rc = anchor_change_checks(c);
  if (rc != OVGPU_OK) return rc;
  if (marg_clone < 0 || marg_clone >= c->C || new_clone < 0 || new_clone >= c->C || marg_clone == new_clone)
    return set_err(OVGPU_ERR_INVALID, "clone index out of range");
  pl = AnchorBatchPlan();
  for (int l = 0; l < c->L; l++) {
    const int32_t a = c->h_lm_anchor[l];
    if (anchor_clone(a) != marg_clone) continue;
    const int cam = anchor_cam(a), lsz = lm_dof(c->h_lm_rep[l]); // same camera (:499-500): its extrinsics appear once in phi_order_OLD
    const int est = c->h_calib_cov[cam] >= 0 ? 1 : 0;
    const int n_old = 6 + 6 * est + 6 + lsz;
    const int32_t e[8] = {l, cam, new_clone, lsz, n_old, (int32_t)pl.n_phi, (int32_t)pl.n_ids, c->h_lm_cov[l]};
    pl.tab.insert(pl.tab.end(), e, e + 8);
    pl.n++, pl.S += lsz, pl.n_ids += n_old, pl.n_phi += (int64_t)lsz * n_old, pl.n_vars += 3 + est;
  }
  *none = pl.n == 0;
  return OVGPU_OK;
}

// the table on the device and ONE launch of k_anchor_change_all; Phi | value | fej in anc_phi, the ids in anc_ids
static int enqueue_anchor_change_all(ovgpu_ctx *c, const AnchorBatchPlan &pl, bool rewrite, size_t tab_ints) {
  hipStream_t s = c->stream;
  HIPCHK(c->anc_tab.reserve(tab_ints));
  HIPCHK(c->anc_ids.reserve((size_t)pl.n_ids));
  HIPCHK(c->anc_phi.reserve((size_t)pl.n_phi + 6 * (size_t)pl.n));
  HIPCHK(upload(c->anc_tab.p, c->h_anc_tab.data(), sizeof(int32_t) * tab_ints, s));
  AnchorAllParams ap;
  ap.n = pl.n, ap.do_fej = c->dopt.do_fej, ap.rewrite = rewrite ? 1 : 0, ap.tab = c->anc_tab.p;
  ap.tab_clone = c->tab_clone.p, ap.tab_cam = c->tab_cam.p, ap.clone_cov = c->clone_cov.p, ap.calib_cov = c->calib_cov.p;
  ap.lm = landmark_store(c), ap.phi = c->anc_phi.p, ap.ids = c->anc_ids.p;
  ap.val = c->anc_phi.p + pl.n_phi, ap.fej = ap.val + 3 * (size_t)pl.n;
  hipLaunchKernelGGL(k_anchor_change_all, dim3(pl.n), dim3(64), 0, s, ap);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

int ovgpu_slam_change_anchors_batched(ovgpu_ctx *c, int32_t marg_clone, int32_t new_clone, int32_t *n_changed) {
  if (n_changed) *n_changed = 0;
  AnchorBatchPlan pl;
  bool none = false;
  int rc = anchor_batch_plan(c, marg_clone, new_clone, pl, &none);
  if (rc != OVGPU_OK || none) return rc;
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }
  hipStream_t s = c->stream;
  const int N = c->N, S = pl.S;
  // table | gmap [S]: (entry << 2 | row) of every joint row | rowg [N]: the joint row of every covariance row
  const size_t tab_ints = pl.tab.size() + (size_t)S + (size_t)N;
  c->h_anc_tab = pl.tab;
  c->h_anc_tab.resize(pl.tab.size() + S);
  c->h_anc_tab.resize(tab_ints, -1);
  int32_t *gmap = c->h_anc_tab.data() + pl.tab.size(), *rowg = gmap + S;
  for (int b = 0, g = 0; b < pl.n; b++) {
    const int32_t *e = pl.tab.data() + 8 * b;
    if (e[7] < 0 || e[7] + e[3] > N) return set_err(OVGPU_ERR_INVALID, "a landmark's covariance id lies outside the covariance");
    for (int a = 0; a < e[3]; a++, g++) gmap[g] = (b << 2) | a, rowg[e[7] + a] = g;
  }
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), s));
  HIPCHK(c->anc_w.reserve((size_t)N * S + (size_t)S * S));
  if ((rc = enqueue_anchor_change_all(c, pl, true, tab_ints)) != OVGPU_OK) return rc;
  PropMultiParams pp;
  pp.N = N, pp.S = S, pp.tab = c->anc_tab.p, pp.gmap = c->anc_tab.p + pl.tab.size(), pp.rowg = pp.gmap + S;
  pp.ids = c->anc_ids.p, pp.phi = c->anc_phi.p, pp.P = c->P.p, pp.W = c->anc_w.p, pp.G = c->anc_w.p + (size_t)N * S, pp.flags = c->flags.p;
  for (int pass = 0; pass < 3; pass++) {
    const int nt = pass == 1 ? S * S : N * S;
    hipLaunchKernelGGL(k_cov_propagate_multi, dim3((nt + 255) / 256), dim3(256), 0, s, pp, pass);
  }
  HIPCHK(hipGetLastError());
  for (int b = 0; b < pl.n; b++) c->h_lm_anchor[pl.tab[8 * b]] = anchor_pack(pl.tab[8 * b + 1], new_clone);
  if (n_changed) *n_changed = pl.n;
  return OVGPU_OK;
}

int ovgpu_slam_anchor_systems_len(ovgpu_ctx *c, int32_t marg_clone, int32_t new_clone, ovgpu_anchor_sizes *sizes) {
  if (!c || !sizes) return set_err(OVGPU_ERR_INVALID, "null argument");
  sizes->n_sys = sizes->n_vars = sizes->n_phi = 0;
  AnchorBatchPlan pl;
  bool none = false;
  const int rc = anchor_batch_plan(c, marg_clone, new_clone, pl, &none);
  if (rc != OVGPU_OK || none) return rc;
  sizes->n_sys = pl.n, sizes->n_vars = pl.n_vars, sizes->n_phi = pl.n_phi;
  return OVGPU_OK;
}

int ovgpu_slam_anchor_systems(ovgpu_ctx *c, int32_t marg_clone, int32_t new_clone, const ovgpu_anchor_sizes *cap, ovgpu_anchor_system *sys, int32_t *var_id,
                              int32_t *var_size, double *Phi, double *value, double *fej) {
  if (!c || !cap) return set_err(OVGPU_ERR_INVALID, "null argument");
  AnchorBatchPlan pl;
  bool none = false;
  int rc = anchor_batch_plan(c, marg_clone, new_clone, pl, &none);
  if (rc != OVGPU_OK || none) return rc;
  if (cap->n_sys < pl.n || cap->n_vars < pl.n_vars || cap->n_phi < pl.n_phi)
    return set_err(OVGPU_ERR_CAPACITY, "output capacities below ovgpu_slam_anchor_systems_len");
  if (!sys || !var_id || !var_size || !Phi || !value || !fej) return set_err(OVGPU_ERR_INVALID, "null output arrays");
  // nothing of the resident state is written: no flag is cleared, a prior-block factorisation in flight stays valid (it reads P only)
  hipStream_t s = c->stream;
  c->h_anc_tab = pl.tab;
  if ((rc = enqueue_anchor_change_all(c, pl, false, pl.tab.size())) != OVGPU_OK) return rc;
  std::vector<double> out((size_t)pl.n_phi + 6 * (size_t)pl.n);
  HIPCHK(hipMemcpyAsync(out.data(), c->anc_phi.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s)); // Phi | value | fej: one gather
  HIPCHK(upload_sync(c, s));
  std::memcpy(Phi, out.data(), sizeof(double) * pl.n_phi);
  std::memcpy(value, out.data() + pl.n_phi, sizeof(double) * 3 * pl.n);
  std::memcpy(fej, out.data() + pl.n_phi + 3 * (size_t)pl.n, sizeof(double) * 3 * pl.n);
  // phi_order_OLD (:592-610) from the host's mirrors of the ids: the kernel's column walk
  int64_t nv = 0;
  for (int b = 0; b < pl.n; b++) {
    const int32_t *e = pl.tab.data() + 8 * b;
    const int l = e[0], cam = e[1];
    ovgpu_anchor_system &o = sys[b];
    std::memset(&o, 0, sizeof(o));
    o.lm_index = l, o.cov_id = e[7], o.lsz = e[3], o.feat_rep = c->h_lm_rep[l], o.n_old = e[4], o.anchor_cam = cam, o.anchor_clone = new_clone;
    o.var_off = nv, o.phi_off = e[5];
    auto push = [&](int32_t id, int32_t size) { var_id[nv] = id, var_size[nv] = size, nv++; };
    push(c->h_clone_cov[marg_clone], 6);
    if (c->h_calib_cov[cam] >= 0) push(c->h_calib_cov[cam], 6);
    push(c->h_clone_cov[new_clone], 6);
    push(e[7], e[3]);
    o.n_vars = (int32_t)(nv - o.var_off);
  }
  return OVGPU_OK;
}

int ovgpu_set_feature_reps(ovgpu_ctx *c, const int32_t *feat_rep) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "no feature batch is resident");
  c->h_feat_rep.clear();
  for (int f = 0; f < c->F && feat_rep; f++)
    if (feat_rep[f] < OVGPU_REP_GLOBAL_3D || feat_rep[f] > OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) return set_err(OVGPU_ERR_INVALID, "unknown landmark representation");
  if (feat_rep) c->h_feat_rep.assign(feat_rep, feat_rep + c->F);
  return OVGPU_OK;
}

int ovgpu_set_feature_options(ovgpu_ctx *c, const double *sigma_pix, const double *chi2_multipler) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "no feature batch is resident");
  HIPCHK(hipSetDevice(c->device));
  const int F = c->F;
  for (int f = 0; f < F && sigma_pix; f++)
    if (!(sigma_pix[f] > 0.0)) return set_err(OVGPU_ERR_INVALID, "sigma_pix must be positive");
  c->have_feat_sigma = sigma_pix != nullptr && F > 0, c->have_feat_mult = chi2_multipler != nullptr && F > 0;
  if (c->have_feat_sigma) {
    HIPCHK(c->feat_sigma.reserve(F));
    HIPCHK(upload(c->feat_sigma.p, sigma_pix, sizeof(double) * F, c->stream));
  }
  if (c->have_feat_mult) {
    HIPCHK(c->feat_mult.reserve(F));
    HIPCHK(upload(c->feat_mult.p, chi2_multipler, sizeof(double) * F, c->stream));
  }
  HIPCHK(upload_sync(c, c->stream));
  return OVGPU_OK;
}
