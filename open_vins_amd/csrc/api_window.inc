// api_window.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): window bookkeeping on the resident covariance (marginalise, clone, propagate), the device-resident track store, retriangulation.
int ovgpu_state_dims(ovgpu_ctx *c, int32_t *N_out, int32_t *C_out) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (N_out) *N_out = c->N;
  if (C_out) *C_out = c->C;
  return OVGPU_OK;
}

int ovgpu_state_marginal_covariance(ovgpu_ctx *c, int32_t n, const int32_t *cov_idx, double *out) {
  if (!c || !cov_idx || !out) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (n < 1 || n > 1024) return set_err(OVGPU_ERR_INVALID, "1 .. 1024 covariance indices");
  for (int i = 0; i < n; i++)
    if (cov_idx[i] < 0 || cov_idx[i] >= c->N) return set_err(OVGPU_ERR_INVALID, "covariance index outside the state");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->marg_idx.reserve(n));
  HIPCHK(c->marg_out.reserve((size_t)n * n));
  HIPCHK(upload(c->marg_idx.p, cov_idx, sizeof(int32_t) * n, c->stream));
  hipLaunchKernelGGL(k_cov_gather, dim3((n * n + 255) / 256), dim3(256), 0, c->stream, c->N, n, c->marg_idx.p, c->P.p, c->marg_out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->marg_out.p, sizeof(double) * n * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(upload_sync(c, c->stream));
  return OVGPU_OK;
}

int ovgpu_state_marginalize(ovgpu_ctx *c, int32_t cov_id, int32_t size) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (cov_id < 0 || size <= 0 || cov_id + size > c->N) return set_err(OVGPU_ERR_INVALID, "marginalised block outside the covariance");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int N = c->N, Nn = N - size;
  // a resident variable that starts inside the block must be exactly the block
  auto hit = [&](int id, int sz) { return id >= 0 && id < cov_id + size && id + sz > cov_id; };
  int drop_clone = -1, drop_lm = -1;
  for (int i = 0; i < c->C; i++)
    if (hit(c->h_clone_cov[i], 6)) {
      if (c->h_clone_cov[i] != cov_id || size != 6 || c->C <= 1) return set_err(OVGPU_ERR_INVALID, "block cuts through a clone (or it is the last one)");
      drop_clone = i;
    }
  for (int l = 0; l < c->L; l++)
    if (hit(c->h_lm_cov[l], lm_dof(c->h_lm_rep[l]))) {
      if (c->h_lm_cov[l] != cov_id || size != lm_dof(c->h_lm_rep[l])) return set_err(OVGPU_ERR_INVALID, "block cuts through a landmark");
      drop_lm = l;
    }
  int drop_calib = -1, drop_intr = -1;
  for (int k = 0; k < c->K; k++) {
    if (hit(c->h_calib_cov[k], 6)) {
      if (c->h_calib_cov[k] != cov_id || size != 6) return set_err(OVGPU_ERR_INVALID, "block cuts through a camera pose");
      drop_calib = k;
    }
    if (hit(c->h_intr_cov[k], 8)) {
      if (c->h_intr_cov[k] != cov_id || size != 8) return set_err(OVGPU_ERR_INVALID, "block cuts through camera intrinsics");
      drop_intr = k;
    }
  }
  if (drop_clone >= 0 && c->L > 0) { // (global landmarks carry anchor -1)
    // a landmark anchored in the clone that goes away must have been re-anchored before (UpdaterSLAM::change_anchors runs before
    // StateHelper::marginalize_old_clone, VioManager.cpp:585-590); checked before anything is modified
    for (int l = 0; l < c->L; l++)
      if (l != drop_lm && anchor_clone(c->h_lm_anchor[l]) == drop_clone)
        return set_err(OVGPU_ERR_INVALID, "a resident landmark is anchored in the marginalised clone (ovgpu_slam_change_anchors first)");
  }
  // ---- nothing was modified so far; from here on the call goes through
  if (drop_calib >= 0) c->h_calib_cov[drop_calib] = -1;
  if (drop_intr >= 0) c->h_intr_cov[drop_intr] = -1;
  // ---- covariance
  HIPCHK(c->Ppad.reserve((size_t)std::max(Nn, 1) * std::max(Nn, 1)));
  if (Nn > 0) {
    dim3 g((Nn + 255) / 256, Nn);
    hipLaunchKernelGGL(k_cov_remove, g, dim3(256), 0, s, N, (int)cov_id, (int)size, c->P.p, c->Ppad.p);
    HIPCHK(hipGetLastError());
  }
  std::swap(c->P, c->Ppad);
  c->N = Nn;
  // ---- resident variables: ids behind the block move forward (:320-323), a dropped clone / landmark leaves its arrays
  DevBuf<double> tmpd;
  DevBuf<int32_t> tmpi;
  if (drop_clone >= 0) {
    HIPCHK(remove_record(c->clone_qp, tmpd, c->C, 7, drop_clone, s));
    HIPCHK(remove_record(c->clone_fej, tmpd, c->C, 7, drop_clone, s));
    c->h_clone_cov.erase(c->h_clone_cov.begin() + drop_clone);
    c->C -= 1;
  }
  if (drop_lm >= 0) {
    HIPCHK(remove_record(c->lm_val, tmpd, c->L, 3, drop_lm, s));
    HIPCHK(remove_record(c->lm_fej, tmpd, c->L, 3, drop_lm, s));
    HIPCHK(remove_record(c->lm_anchor, tmpi, c->L, 1, drop_lm, s));
    HIPCHK(remove_record(c->lm_repd, tmpi, c->L, 1, drop_lm, s));
    c->h_lm_rep.erase(c->h_lm_rep.begin() + drop_lm);
    c->h_lm_cov.erase(c->h_lm_cov.begin() + drop_lm);
    c->h_lm_anchor.erase(c->h_lm_anchor.begin() + drop_lm);
    if (c->active_given && drop_lm < (int)c->h_lm_active.size()) c->h_lm_active.erase(c->h_lm_active.begin() + drop_lm); // the set follows the landmarks' indices
    c->L -= 1;
  }
  HIPCHK(upload_sync(c, s)); // (the scratch copies are done with; tmpd and tmpi go with the scope)
  auto shift = [&](int32_t &id) { if (id > cov_id) id -= size; };
  for (auto &id : c->h_clone_cov) shift(id);
  for (auto &id : c->h_calib_cov) shift(id);
  for (auto &id : c->h_intr_cov) shift(id);
  for (auto &id : c->h_lm_cov) shift(id);
  if (drop_clone >= 0 && c->L > 0 && lm_any_anchored(c)) {
    // anchored landmarks refer to clone INDICES: the clones behind the dropped one moved down
    std::vector<int32_t> &anc = c->h_lm_anchor;
    for (auto &a : anc) {
      if (a < 0) continue;
      const int cl = anchor_clone(a);
      a = anchor_pack(anchor_cam(a), cl > drop_clone ? cl - 1 : cl);
    }
    HIPCHK(hipMemcpy(c->lm_anchor.p, anc.data(), sizeof(int32_t) * c->L, hipMemcpyHostToDevice));
  }
  return rebuild_variables(c);
}

// StateHelper::marginalize_slam + marginalize_old_clone of one frame (StateHelper.cpp:618-651) as ONE removal: the blocks name the covariance as
// it is at entry.  Three launches (k_marg_plan, k_cov_remove_many, k_records_compact) and one rebuild_variables whatever n is; the only host
// copy is the block list, which travels through the page-locked arena.
int ovgpu_state_marginalize_batched(ovgpu_ctx *c, int32_t n, const int32_t *cov_id, const int32_t *size) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (n < 0 || (n > 0 && (!cov_id || !size))) return set_err(OVGPU_ERR_INVALID, "bad block arrays");
  if (n == 0) return OVGPU_OK;
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  const int N = c->N, C = c->C, L = c->L, K = c->K;
  // ---- checks: nothing is modified before all of them have passed
  std::vector<std::pair<int32_t, int32_t>> blk(n);
  for (int b = 0; b < n; b++) {
    if (cov_id[b] < 0 || size[b] <= 0 || (int64_t)cov_id[b] + size[b] > N) return set_err(OVGPU_ERR_INVALID, "marginalised block outside the covariance");
    blk[b] = {cov_id[b], size[b]};
  }
  std::sort(blk.begin(), blk.end());
  for (int b = 1; b < n; b++)
    if (blk[b].first < blk[b - 1].first + blk[b - 1].second) return set_err(OVGPU_ERR_INVALID, "marginalised blocks overlap or repeat");
  // the block that touches [id, id + sz), if any (the blocks are disjoint: when it IS the variable no other one touches it); -1: none, -2: one that cuts it
  auto block_of = [&](int id, int sz) {
    if (id < 0) return -1;
    auto it = std::upper_bound(blk.begin(), blk.end(), id, [](int v, const std::pair<int32_t, int32_t> &b) { return v < b.first + b.second; }); // first block that ends behind id
    if (it == blk.end() || it->first >= id + sz) return -1;
    return (it->first == id && it->second == sz) ? (int)(it - blk.begin()) : -2;
  };
  std::vector<int32_t> tab((size_t)2 * n + C + L); // blocks | clone_keep | lm_keep: what k_marg_plan reads
  int32_t *clone_keep = tab.data() + 2 * n, *lm_keep = clone_keep + C;
  int Cn = 0, Ln = 0;
  for (int i = 0; i < C; i++) {
    const int b = block_of(c->h_clone_cov[i], 6);
    if (b == -2) return set_err(OVGPU_ERR_INVALID, "block cuts through a clone (or it is the last one)");
    clone_keep[i] = b < 0, Cn += b < 0;
  }
  if (Cn < 1) return set_err(OVGPU_ERR_INVALID, "block cuts through a clone (or it is the last one)");
  for (int l = 0; l < L; l++) {
    const int b = block_of(c->h_lm_cov[l], lm_dof(c->h_lm_rep[l]));
    if (b == -2) return set_err(OVGPU_ERR_INVALID, "block cuts through a landmark");
    lm_keep[l] = b < 0, Ln += b < 0;
  }
  std::vector<uint8_t> calib_gone(K, 0), intr_gone(K, 0);
  for (int k = 0; k < K; k++) {
    const int bc = block_of(c->h_calib_cov[k], 6), bi = block_of(c->h_intr_cov[k], 8);
    if (bc == -2) return set_err(OVGPU_ERR_INVALID, "block cuts through a camera pose");
    if (bi == -2) return set_err(OVGPU_ERR_INVALID, "block cuts through camera intrinsics");
    calib_gone[k] = bc >= 0, intr_gone[k] = bi >= 0;
  }
  if (Cn < C) // a landmark anchored in a clone that leaves must leave with it, or have been re-anchored before (UpdaterSLAM::change_anchors, VioManager.cpp:585-590)
    for (int l = 0; l < L; l++)
      if (lm_keep[l] && c->h_lm_anchor[l] >= 0 && !clone_keep[anchor_clone(c->h_lm_anchor[l])])
        return set_err(OVGPU_ERR_INVALID, "a resident landmark is anchored in the marginalised clone (ovgpu_slam_change_anchors first)");
  int gone = 0;
  for (int b = 0; b < n; b++) tab[2 * b] = blk[b].first, tab[2 * b + 1] = blk[b].second, gone += blk[b].second;
  const int Nn = N - gone; // (>= 6: a clone stays)
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  HIPCHK(c->up.begin());
  HIPCHK(c->marg_tab.reserve(tab.size() + (size_t)N + 2 * (size_t)C + L));
  HIPCHK(c->Ppad.reserve((size_t)Nn * Nn));
  HIPCHK(c->clone_qp_b.reserve(std::max<size_t>(c->clone_qp.cap, 1)));
  HIPCHK(c->clone_fej_b.reserve(std::max<size_t>(c->clone_fej.cap, 1)));
  HIPCHK(c->lm_val_b.reserve(std::max<size_t>(c->lm_val.cap, 1)));
  HIPCHK(c->lm_fej_b.reserve(std::max<size_t>(c->lm_fej.cap, 1)));
  HIPCHK(c->lm_anchor_b.reserve(std::max<size_t>(c->lm_anchor.cap, 1)));
  HIPCHK(c->lm_repd_b.reserve(std::max<size_t>(c->lm_repd.cap, 1)));
  // ---- the device pass (a HIP error from here on is reported; the host tables below change only behind the launches)
  HIPCHK(c->up.put(c->marg_tab.p, tab.data(), sizeof(int32_t) * tab.size()));
  HIPCHK(c->up.flush());
  MargPlan mp;
  mp.N = N, mp.C = C, mp.L = L, mp.n = n;
  mp.blk = c->marg_tab.p, mp.clone_keep = mp.blk + 2 * n, mp.lm_keep = mp.clone_keep + C;
  mp.keep = c->marg_tab.p + tab.size(), mp.clone_src = mp.keep + N, mp.clone_new = mp.clone_src + C, mp.lm_src = mp.clone_new + C;
  hipLaunchKernelGGL(k_marg_plan, dim3(1), dim3(64), 0, s, mp);
  hipLaunchKernelGGL(k_cov_remove_many, dim3((Nn + 255) / 256, Nn), dim3(256), 0, s, N, Nn, (const int32_t *)mp.keep, (const double *)c->P.p, c->Ppad.p);
  RecordsCompact rp;
  rp.Cn = Cn, rp.Ln = Ln, rp.clone_src = mp.clone_src, rp.clone_new = mp.clone_new, rp.lm_src = mp.lm_src;
  rp.clone_qp = c->clone_qp.p, rp.clone_fej = c->clone_fej.p, rp.lm_val = c->lm_val.p, rp.lm_fej = c->lm_fej.p, rp.lm_anchor = c->lm_anchor.p, rp.lm_rep = c->lm_repd.p;
  rp.clone_qp_out = c->clone_qp_b.p, rp.clone_fej_out = c->clone_fej_b.p, rp.lm_val_out = c->lm_val_b.p, rp.lm_fej_out = c->lm_fej_b.p;
  rp.lm_anchor_out = c->lm_anchor_b.p, rp.lm_rep_out = c->lm_repd_b.p;
  hipLaunchKernelGGL(k_records_compact, dim3((std::max(7 * Cn, 3 * Ln) + 255) / 256), dim3(256), 0, s, rp);
  HIPCHK(hipGetLastError());
  std::swap(c->P, c->Ppad);
  std::swap(c->clone_qp, c->clone_qp_b), std::swap(c->clone_fej, c->clone_fej_b);
  std::swap(c->lm_val, c->lm_val_b), std::swap(c->lm_fej, c->lm_fej_b), std::swap(c->lm_anchor, c->lm_anchor_b), std::swap(c->lm_repd, c->lm_repd_b);
  // ---- the host's mirrors: what the chain of single calls leaves (ids behind a block move forward by its size, :320-323; indices close up)
  std::vector<int32_t> before(n + 1, 0); // rows removed by the first b blocks
  for (int b = 0; b < n; b++) before[b + 1] = before[b] + blk[b].second;
  auto shifted = [&](int32_t id) {
    if (id < 0) return id;
    const int b = (int)(std::upper_bound(blk.begin(), blk.end(), std::make_pair(id, (int32_t)0x7fffffff)) - blk.begin()); // blocks that start at or before id
    return id - before[b];
  };
  std::vector<int32_t> clone_new(C, -1);
  for (int i = 0, w = 0; i < C; i++)
    if (clone_keep[i]) clone_new[i] = w, c->h_clone_cov[w++] = shifted(c->h_clone_cov[i]);
  c->h_clone_cov.resize(Cn);
  for (int k = 0; k < K; k++) {
    c->h_calib_cov[k] = calib_gone[k] ? -1 : shifted(c->h_calib_cov[k]);
    c->h_intr_cov[k] = intr_gone[k] ? -1 : shifted(c->h_intr_cov[k]);
  }
  const bool act = c->active_given && (int)c->h_lm_active.size() >= L; // the set follows the landmarks' indices
  for (int l = 0, w = 0; l < L; l++) {
    if (!lm_keep[l]) continue;
    const int32_t a = c->h_lm_anchor[l];
    c->h_lm_rep[w] = c->h_lm_rep[l], c->h_lm_cov[w] = shifted(c->h_lm_cov[l]);
    c->h_lm_anchor[w] = a >= 0 ? anchor_pack(anchor_cam(a), clone_new[anchor_clone(a)]) : a;
    if (act) c->h_lm_active[w] = c->h_lm_active[l];
    w++;
  }
  c->h_lm_rep.resize(Ln), c->h_lm_cov.resize(Ln), c->h_lm_anchor.resize(Ln);
  if (act) c->h_lm_active.resize(Ln);
  c->N = Nn, c->C = Cn, c->L = Ln;
  return rebuild_variables(c);
}

int ovgpu_state_augment_clone(ovgpu_ctx *c, int32_t src_cov_id, const double *q_p, const double *q_p_fej, int32_t dt_cov_id, const double *dnc_dt,
                              int32_t *new_cov_id) {
  if (!c || !q_p || !q_p_fej) return set_err(OVGPU_ERR_INVALID, "null argument");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (src_cov_id < 0 || src_cov_id + 6 > c->N) return set_err(OVGPU_ERR_INVALID, "cloned pose outside the covariance");
  if (dt_cov_id >= c->N || (dt_cov_id >= 0 && !dnc_dt)) return set_err(OVGPU_ERR_INVALID, "bad time-offset argument");
  if (c->C + 1 > OVG_MAX_CLONES) return set_err(OVGPU_ERR_CAPACITY, "too many clones");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int N = c->N, Nn = N + 6, C = c->C;
  // ---- covariance: grow, copy the pose's rows / columns to the end (StateHelper.cpp:348-372)
  {
    const int rcr = cov_resize(c, N, Nn, N);
    if (rcr != OVGPU_OK) return rcr;
    hipLaunchKernelGGL(k_cov_clone, dim3((N + 36 + 255) / 256), dim3(256), 0, s, Nn, N, (int)src_cov_id, N, 6, c->P.p);
    HIPCHK(hipGetLastError());
  }
  if (dt_cov_id >= 0) { // :601-611
    HIPCHK(c->prop_in.reserve(64));
    HIPCHK(upload(c->prop_in.p, dnc_dt, sizeof(double) * 6, s));
    HIPCHK(upload_sync(c, s));
    hipLaunchKernelGGL(k_cov_dt, dim3((Nn + 255) / 256), dim3(256), 0, s, Nn, N, (int)dt_cov_id, c->prop_in.p, c->P.p, 0);
    hipLaunchKernelGGL(k_cov_dt, dim3((Nn + 255) / 256), dim3(256), 0, s, Nn, N, (int)dt_cov_id, c->prop_in.p, c->P.p, 1);
    HIPCHK(hipGetLastError());
  }
  // ---- the clone joins the resident ones (State::_clones_IMU[timestamp] = pose, :597)
  HIPCHK(c->clone_qp.reserve(7 * (size_t)(C + 1), 7 * (size_t)C));
  HIPCHK(c->clone_fej.reserve(7 * (size_t)(C + 1), 7 * (size_t)C));
  HIPCHK(upload(c->clone_qp.p + 7 * C, q_p, sizeof(double) * 7, s));
  HIPCHK(upload(c->clone_fej.p + 7 * C, q_p_fej, sizeof(double) * 7, s));
  HIPCHK(upload_sync(c, s));
  c->h_clone_cov.push_back(N);
  c->C = C + 1;
  if (new_cov_id) *new_cov_id = N;
  return rebuild_variables(c);
}

int ovgpu_state_propagate(ovgpu_ctx *c, int32_t new_cov_id, int32_t n_new, int32_t n_old, const int32_t *old_cov_ids, const double *Phi,
                          const double *Q) {
  if (!c || !old_cov_ids || !Phi || !Q) return set_err(OVGPU_ERR_INVALID, "null argument");
  { const int rdp = drop_pending_prior(c); if (rdp != OVGPU_OK) return rdp; }  // the covariance changes: a prior-block factorisation started for a sharded update is stale
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (n_new <= 0 || n_old <= 0 || new_cov_id < 0 || new_cov_id + n_new > c->N) return set_err(OVGPU_ERR_INVALID, "propagated block outside the covariance"); // :41-44
  for (int k = 0; k < n_old; k++)
    if (old_cov_ids[k] < 0 || old_cov_ids[k] >= c->N) return set_err(OVGPU_ERR_INVALID, "old variable outside the covariance");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int N = c->N;
  HIPCHK(c->prop_in.reserve((size_t)n_new * n_old + (size_t)n_new * n_new));
  HIPCHK(c->prop_ids.reserve(n_old));
  HIPCHK(c->prop_w.reserve((size_t)N * n_new + (size_t)n_new * n_new));
  double *dPhi = c->prop_in.p, *dQ = dPhi + (size_t)n_new * n_old, *W = c->prop_w.p, *PCP = W + (size_t)N * n_new;
  HIPCHK(upload(dPhi, Phi, sizeof(double) * n_new * n_old, s));
  HIPCHK(upload(dQ, Q, sizeof(double) * n_new * n_new, s));
  HIPCHK(upload(c->prop_ids.p, old_cov_ids, sizeof(int32_t) * n_old, s));
  HIPCHK(hipMemsetAsync(c->flags.p, 0, 4 * sizeof(int32_t), s));
  HIPCHK(upload_sync(c, s)); // the caller's buffers may change
  const int n1 = N * n_new;
  for (int pass = 0; pass < 3; pass++) {
    const int n = pass == 1 ? n_new * n_new : n1;
    hipLaunchKernelGGL(k_cov_propagate, dim3((n + 255) / 256), dim3(256), 0, s, N, (int)new_cov_id, (int)n_new, (int)n_old, c->prop_ids.p, dPhi, dQ, c->P.p, W,
                       PCP, c->flags.p, pass);
  }
  HIPCHK(hipGetLastError());
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  if (flags[1]) return set_err(OVGPU_ERR_NEGATIVE_DIAGONAL, "negative covariance diagonal after the propagation");
  return OVGPU_OK;
}

// ---------------------------------------------------------------------------
// FeatureDatabase on the device (SURVEY.md 8f N2)
// ---------------------------------------------------------------------------
static TrackStore track_store(ovgpu_ctx *c) { return TrackStore{c->trk_obs, c->trk_count.p, c->trk_time.p, c->trk_cam.p, c->trk_uv.p, c->trk_uvn.p}; }

int ovgpu_tracks_create(ovgpu_ctx *c, int32_t max_tracks, int32_t max_obs) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (max_tracks <= 0 || max_obs <= 0 || (int64_t)max_tracks * max_obs > ((int64_t)1 << 31)) return set_err(OVGPU_ERR_INVALID, "bad track store size");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)max_tracks * max_obs;
  HIPCHK(c->trk_count.reserve(max_tracks));
  HIPCHK(c->trk_time.reserve(n));
  HIPCHK(c->trk_cam.reserve(n));
  HIPCHK(c->trk_uv.reserve(2 * n));
  HIPCHK(c->trk_uvn.reserve(2 * n));
  HIPCHK(c->trk_flag.reserve(1));
  HIPCHK(hipMemsetAsync(c->trk_count.p, 0, sizeof(int32_t) * max_tracks, c->stream));
  HIPCHK(hipMemsetAsync(c->trk_flag.p, 0, sizeof(int32_t), c->stream));
  HIPCHK(upload_sync(c, c->stream));
  c->trk_max = max_tracks, c->trk_obs = max_obs;
  c->trk_slot_of.clear();
  c->trk_free.resize(max_tracks);
  for (int i = 0; i < max_tracks; i++) c->trk_free[i] = max_tracks - 1 - i; // slot 0 is handed out first
  c->trk_h_count.assign(max_tracks, 0), c->trk_h_id.assign(max_tracks, -1);
  c->trk_h_cams.assign(max_tracks, std::vector<int8_t>());
  return OVGPU_OK;
}

// ---------------------------------------------------------------------------------------------------
// VioManager::retriangulate_active_tracks (VioManagerHelper.cpp:190-387)
// ---------------------------------------------------------------------------------------------------
int ovgpu_retriangulate_reset(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  c->retri_slot_of.clear();
  return OVGPU_OK;
}

int ovgpu_retriangulate(ovgpu_ctx *c, int32_t clone_index, int32_t n, const int64_t *featid, const int32_t *cam_id, const float *uv, const float *uvn,
                        int32_t cam0, int32_t img_w, int32_t img_h, int32_t *n_tracks, int64_t *out_featid, double *out_p_FinG, double *out_uvd) {
  if (!c || !n_tracks) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state (or ovgpu_set_camera_poses) was never called");
  if (n < 0 || (n > 0 && (!featid || !cam_id || !uv || !uvn || !out_featid || !out_p_FinG || !out_uvd))) return set_err(OVGPU_ERR_INVALID, "bad observation arrays");
  if (clone_index < 0 || clone_index >= c->C) return set_err(OVGPU_ERR_INVALID, "clone_index outside the window");
  if (cam0 >= c->K) return set_err(OVGPU_ERR_INVALID, "cam0 is not a camera of the state");
  HIPCHK(hipSetDevice(c->device));
  // ---- group the frame's observations by track, in order of first appearance; observations of a track keep the frame's camera order
  std::unordered_map<int64_t, int32_t> slot_now;
  std::vector<int64_t> ids;
  std::vector<int32_t> tr_of(n);
  for (int i = 0; i < n; i++) {
    if (cam_id[i] < 0 || cam_id[i] >= c->K) return set_err(OVGPU_ERR_INVALID, "camera index outside the state's cameras");
    auto it = slot_now.find(featid[i]);
    if (it == slot_now.end()) it = slot_now.emplace(featid[i], (int32_t)ids.size()).first, ids.push_back(featid[i]);
    tr_of[i] = it->second;
  }
  const int T = (int)ids.size();
  *n_tracks = T;
  if (T == 0) { // no track is alive: every system is dropped (:305-309)
    c->retri_slot_of.clear();
    return OVGPU_OK;
  }
  std::vector<int32_t> ints((size_t)(T + 1) + n + T, 0); // obs_off | obs_cam | old_slot
  int32_t *off = ints.data(), *ocam = off + T + 1, *old = ocam + n;
  for (int i = 0; i < n; i++) off[tr_of[i] + 1]++;
  for (int t = 0; t < T; t++) off[t + 1] += off[t];
  std::vector<int32_t> fill(off, off + T);
  std::vector<float> fl((size_t)4 * n);
  for (int i = 0; i < n; i++) {
    const int j = fill[tr_of[i]]++;
    ocam[j] = cam_id[i];
    fl[2 * j] = uv[2 * i], fl[2 * j + 1] = uv[2 * i + 1];
    fl[(size_t)2 * n + 2 * j] = uvn[2 * i], fl[(size_t)2 * n + 2 * j + 1] = uvn[2 * i + 1];
  }
  for (int t = 0; t < T; t++) {
    auto it = c->retri_slot_of.find(ids[t]);
    old[t] = it == c->retri_slot_of.end() ? -1 : it->second;
  }
  const int g = c->retri_gen;
  HIPCHK(c->retri_sys[g ^ 1].reserve((size_t)13 * T));
  HIPCHK(c->retri_sys[g].reserve(13));
  HIPCHK(c->retri_pos.reserve((size_t)3 * T));
  HIPCHK(c->retri_uvd.reserve((size_t)3 * T));
  HIPCHK(c->retri_int.reserve(ints.size()));
  HIPCHK(c->retri_f.reserve(fl.size()));
  hipStream_t s = c->stream;
  HIPCHK(upload(c->retri_int.p, ints.data(), sizeof(int32_t) * ints.size(), s));
  HIPCHK(upload(c->retri_f.p, fl.data(), sizeof(float) * fl.size(), s));
  RetriParams p;
  p.n_tracks = T, p.C = c->C, p.clone = clone_index;
  p.obs_off = c->retri_int.p, p.obs_cam = c->retri_int.p + T + 1, p.old_slot = c->retri_int.p + T + 1 + n;
  p.obs_uv = c->retri_f.p, p.obs_uvn = c->retri_f.p + (size_t)2 * n;
  p.old_sys = c->retri_sys[g].p, p.new_sys = c->retri_sys[g ^ 1].p, p.tab_cc = c->tab_cc.p;
  p.cam0 = cam0, p.img_w = img_w, p.img_h = img_h;
  p.max_cond = c->dopt.max_cond_number, p.min_dist = c->dopt.min_dist, p.max_dist = c->dopt.max_dist;
  p.out_pos = c->retri_pos.p, p.out_uvd = c->retri_uvd.p;
  hipLaunchKernelGGL(k_retriangulate, dim3((T + 255) / 256), dim3(256), 0, s, p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_p_FinG, c->retri_pos.p, sizeof(double) * 3 * T, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(out_uvd, c->retri_uvd.p, sizeof(double) * 3 * T, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  std::copy(ids.begin(), ids.end(), out_featid);
  c->retri_gen = g ^ 1;
  c->retri_slot_of.swap(slot_now); // only the tracks of this frame stay alive
  return OVGPU_OK;
}

int ovgpu_tracks_count(ovgpu_ctx *c, int32_t *n_tracks) {
  if (!c || !n_tracks) return set_err(OVGPU_ERR_INVALID, "null argument");
  *n_tracks = (int32_t)c->trk_slot_of.size();
  return OVGPU_OK;
}

int ovgpu_tracks_append(ovgpu_ctx *c, double timestamp, int32_t n, const int64_t *featid, const int32_t *cam_id, const float *uv, const float *uvn) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  if (n < 0 || (n > 0 && (!featid || !cam_id || !uv || !uvn))) return set_err(OVGPU_ERR_INVALID, "bad observation arrays");
  if (n == 0) return OVGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  // ---- capacity first: nothing is appended when the call cannot go through as a whole
  {
    std::unordered_map<int64_t, int> add;
    size_t fresh = 0;
    for (int i = 0; i < n; i++) {
      if (cam_id[i] < 0 || cam_id[i] >= OVG_MAX_CAMS) return set_err(OVGPU_ERR_INVALID, "camera id out of range");
      add[featid[i]]++;
    }
    for (const auto &kv : add) {
      auto it = c->trk_slot_of.find(kv.first);
      const int have = it == c->trk_slot_of.end() ? 0 : c->trk_h_count[it->second];
      if (it == c->trk_slot_of.end()) fresh++;
      if (have + kv.second > c->trk_obs) return set_err(OVGPU_ERR_CAPACITY, "a track is full");
    }
    if (fresh > c->trk_free.size()) return set_err(OVGPU_ERR_CAPACITY, "the track store is full");
  }
  // slots of the observations: decided on COPIES of the host tables, which are committed only after the device has taken the call
  // (a HIP error in between would otherwise leave the host's counts ahead of the device's)
  std::vector<int32_t> slot(n);
  std::unordered_map<int64_t, int> fresh_slot;
  size_t free_used = 0;
  for (int i = 0; i < n; i++) {
    auto it = c->trk_slot_of.find(featid[i]);
    if (it != c->trk_slot_of.end()) {
      slot[i] = it->second;
      continue;
    }
    auto fi = fresh_slot.find(featid[i]);
    if (fi == fresh_slot.end()) fi = fresh_slot.emplace(featid[i], c->trk_free[c->trk_free.size() - 1 - free_used++]).first; // FeatureDatabase.cpp:76-84: a new feature
    slot[i] = fi->second;
  }
  hipStream_t s = c->stream;
  HIPCHK(c->trk_slot_in.reserve(n));
  HIPCHK(c->trk_cam_in.reserve(n));
  HIPCHK(c->trk_uv_in.reserve(2 * (size_t)n));
  HIPCHK(c->trk_uvn_in.reserve(2 * (size_t)n));
  HIPCHK(upload(c->trk_slot_in.p, slot.data(), sizeof(int32_t) * n, s));
  HIPCHK(upload(c->trk_cam_in.p, cam_id, sizeof(int32_t) * n, s));
  HIPCHK(upload(c->trk_uv_in.p, uv, sizeof(float) * 2 * n, s));
  HIPCHK(upload(c->trk_uvn_in.p, uvn, sizeof(float) * 2 * n, s));
  hipLaunchKernelGGL(k_tracks_append, dim3((n + 255) / 256), dim3(256), 0, s, n, timestamp, c->trk_slot_in.p, c->trk_cam_in.p, c->trk_uv_in.p, c->trk_uvn_in.p,
                     track_store(c), c->trk_flag.p);
  HIPCHK(hipGetLastError());
  HIPCHK(upload_sync(c, s)); // the caller's arrays and `slot` may go away
  // ---- commit
  for (size_t u = 0; u < free_used; u++) c->trk_free.pop_back();
  for (const auto &kv : fresh_slot) {
    c->trk_slot_of.emplace(kv.first, kv.second);
    c->trk_h_id[kv.second] = kv.first, c->trk_h_count[kv.second] = 0;
    c->trk_h_cams[kv.second].clear();
  }
  for (int i = 0; i < n; i++) {
    const int sl = slot[i];
    // Feature::timestamps[cam_id] (FeatureDatabase.cpp:72, :81): a new key the first time the camera sees the feature
    std::vector<int8_t> &cams = c->trk_h_cams[sl];
    if (std::find(cams.begin(), cams.end(), (int8_t)cam_id[i]) == cams.end()) cams.push_back((int8_t)cam_id[i]);
    c->trk_h_count[sl]++;
  }
  return OVGPU_OK;
}

int ovgpu_tracks_erase(ovgpu_ctx *c, int32_t n, const int64_t *featid) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (n < 0 || (n > 0 && !featid)) return set_err(OVGPU_ERR_INVALID, "bad id array");
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  HIPCHK(hipSetDevice(c->device));
  // the slots to clear: ONE upload and one launch (round 4 issued a 4-byte copy from pageable memory per track: 2000 staged copies for the
  // batch of one update in the resident-track mode of the drop-in); the host tables follow once the device has taken the call
  std::vector<int32_t> slots;
  std::vector<int64_t> ids;
  std::unordered_set<int64_t> seen;
  slots.reserve(n), ids.reserve(n);
  for (int i = 0; i < n; i++) {
    auto it = c->trk_slot_of.find(featid[i]);
    if (it == c->trk_slot_of.end() || !seen.insert(featid[i]).second) continue;
    slots.push_back(it->second), ids.push_back(featid[i]);
  }
  if (slots.empty()) return OVGPU_OK;
  const int T = (int)slots.size();
  HIPCHK(c->trk_slot_in.reserve(T));
  HIPCHK(upload(c->trk_slot_in.p, slots.data(), sizeof(int32_t) * T, c->stream));
  hipLaunchKernelGGL(k_tracks_clear, dim3((T + 255) / 256), dim3(256), 0, c->stream, T, (const int32_t *)c->trk_slot_in.p, c->trk_count.p);
  HIPCHK(hipGetLastError());
  HIPCHK(upload_sync(c, c->stream));
  for (int i = 0; i < T; i++) {
    const int sl = slots[i];
    c->trk_h_count[sl] = 0, c->trk_h_id[sl] = -1;
    c->trk_free.push_back(sl);
    c->trk_slot_of.erase(ids[i]);
  }
  return OVGPU_OK;
}

// ---------------------------------------------------------------------------------------------------
// FeatureDatabase's queries and clean-ups on the device store (k_tracks.h: k_tracks_query, k_tracks_cleanup)
// ---------------------------------------------------------------------------------------------------
// the live tracks in ascending id order (the reference returns them in the iteration order of an unordered_map, which nothing
// downstream depends on: VioManager.cpp:366-378 concatenates and sorts by track length), their slots uploaded to trk_sel
static int tracks_live(ovgpu_ctx *c, std::vector<int64_t> &ids, std::vector<int32_t> &slots) {
  ids.clear(), slots.clear();
  ids.reserve(c->trk_slot_of.size());
  for (const auto &kv : c->trk_slot_of) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  slots.reserve(ids.size());
  for (int64_t id : ids) slots.push_back(c->trk_slot_of.at(id));
  const size_t T = ids.size();
  HIPCHK(c->trk_sel.reserve(std::max<size_t>(T, 1)));
  HIPCHK(c->trk_nvalid.reserve(std::max<size_t>(T, 1)));
  HIPCHK(c->trk_aux.reserve(std::max<size_t>(T, 1)));
  if (T > 0) HIPCHK(upload(c->trk_sel.p, slots.data(), sizeof(int32_t) * T, c->stream));
  return OVGPU_OK;
}
// one query over every live track: ids (ascending), flag per track, aux per track when asked for
static int tracks_query(ovgpu_ctx *c, int mode, double timestamp, std::vector<int64_t> &ids, std::vector<int32_t> &flag, std::vector<double> *aux) {
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int32_t> slots;
  const int rc = tracks_live(c, ids, slots);
  if (rc != OVGPU_OK) return rc;
  const int T = (int)ids.size();
  flag.assign(T, 0);
  if (aux) aux->assign(T, 0.0);
  if (T == 0) return OVGPU_OK;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_tracks_query, dim3((T + 127) / 128), dim3(128), 0, s, T, c->trk_sel.p, mode, timestamp, track_store(c), c->trk_nvalid.p,
                     aux ? c->trk_aux.p : (double *)nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(flag.data(), c->trk_nvalid.p, sizeof(int32_t) * T, hipMemcpyDeviceToHost, s));
  if (aux) HIPCHK(hipMemcpyAsync(aux->data(), c->trk_aux.p, sizeof(double) * T, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}
static int tracks_query_ids(ovgpu_ctx *c, int mode, double timestamp, int32_t capacity, int64_t *ids_out, int32_t *n_out) {
  if (!c || !n_out) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (capacity < 0 || (capacity > 0 && !ids_out)) return set_err(OVGPU_ERR_INVALID, "bad id array");
  std::vector<int64_t> ids;
  std::vector<int32_t> flag;
  const int rc = tracks_query(c, mode, timestamp, ids, flag, nullptr);
  if (rc != OVGPU_OK) return rc;
  int n = 0;
  for (size_t t = 0; t < ids.size(); t++)
    if (flag[t]) {
      if (ids_out && n < capacity) ids_out[n] = ids[t];
      n++;
    }
  *n_out = n;
  return OVGPU_OK;
}

int ovgpu_tracks_not_containing_newer(ovgpu_ctx *c, double timestamp, int32_t capacity, int64_t *ids, int32_t *n_out) {
  return tracks_query_ids(c, TRK_Q_NOT_NEWER, timestamp, capacity, ids, n_out); // FeatureDatabase.cpp:103-108
}
int ovgpu_tracks_containing_older(ovgpu_ctx *c, double timestamp, int32_t capacity, int64_t *ids, int32_t *n_out) {
  return tracks_query_ids(c, TRK_Q_CONTAINING_OLDER, timestamp, capacity, ids, n_out); // FeatureDatabase.cpp:144-149
}
int ovgpu_tracks_containing(ovgpu_ctx *c, double timestamp, int32_t capacity, int64_t *ids, int32_t *n_out) {
  return tracks_query_ids(c, TRK_Q_CONTAINING, timestamp, capacity, ids, n_out); // FeatureDatabase.cpp:186-191
}

int ovgpu_tracks_oldest_timestamp(ovgpu_ctx *c, double *t_out) {
  if (!c || !t_out) return set_err(OVGPU_ERR_INVALID, "null argument");
  std::vector<int64_t> ids;
  std::vector<int32_t> flag;
  std::vector<double> first;
  const int rc = tracks_query(c, TRK_Q_OLDEST, 0.0, ids, flag, &first);
  if (rc != OVGPU_OK) return rc;
  double oldest = -1.0; // FeatureDatabase.cpp:267: -1 when the database holds no observation
  bool any = false;
  for (double t : first)
    if (t < __builtin_huge_val() && (!any || t < oldest)) oldest = t, any = true;
  *t_out = oldest;
  return OVGPU_OK;
}

static int tracks_cleanup(ovgpu_ctx *c, double timestamp, int exact, int32_t *n_erased) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int64_t> ids;
  std::vector<int32_t> slots;
  const int rc = tracks_live(c, ids, slots);
  if (rc != OVGPU_OK) return rc;
  const int T = (int)ids.size();
  int erased = 0;
  if (T > 0) {
    hipStream_t s = c->stream;
    std::vector<int32_t> left(T);
    hipLaunchKernelGGL(k_tracks_cleanup, dim3((T + 127) / 128), dim3(128), 0, s, T, c->trk_sel.p, exact, timestamp, track_store(c), c->trk_nvalid.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(left.data(), c->trk_nvalid.p, sizeof(int32_t) * T, hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
    for (int t = 0; t < T; t++) {
      const int sl = slots[t];
      c->trk_h_count[sl] = left[t];
      if (left[t] < 1) { // FeatureDatabase.cpp:236-238, :255-257: a feature without measurements leaves the database
        c->trk_h_id[sl] = -1;
        c->trk_free.push_back(sl);
        c->trk_slot_of.erase(ids[t]);
        erased++;
      }
    }
  }
  if (n_erased) *n_erased = erased;
  return OVGPU_OK;
}
int ovgpu_tracks_cleanup_measurements(ovgpu_ctx *c, double timestamp, int32_t *n_erased) { return tracks_cleanup(c, timestamp, 0, n_erased); }
int ovgpu_tracks_cleanup_measurements_exact(ovgpu_ctx *c, double timestamp, int32_t *n_erased) { return tracks_cleanup(c, timestamp, 1, n_erased); }

int ovgpu_tracks_get_feature(ovgpu_ctx *c, int64_t featid, int32_t capacity, int32_t *n_out, double *timestamps, int32_t *cam_id, float *uv, float *uvn) {
  if (!c || !n_out) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  if (capacity < 0) return set_err(OVGPU_ERR_INVALID, "negative capacity");
  *n_out = 0;
  auto it = c->trk_slot_of.find(featid);
  if (it == c->trk_slot_of.end()) return OVGPU_OK; // FeatureDatabase.cpp:44-46: unknown id
  const int sl = it->second, n = c->trk_h_count[sl], k = std::min(n, (int)capacity);
  *n_out = n;
  if (k == 0) return OVGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t base = (size_t)sl * c->trk_obs;
  if (timestamps) HIPCHK(hipMemcpyAsync(timestamps, c->trk_time.p + base, sizeof(double) * k, hipMemcpyDeviceToHost, s));
  if (cam_id) HIPCHK(hipMemcpyAsync(cam_id, c->trk_cam.p + base, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s));
  if (uv) HIPCHK(hipMemcpyAsync(uv, c->trk_uv.p + 2 * base, sizeof(float) * 2 * k, hipMemcpyDeviceToHost, s));
  if (uvn) HIPCHK(hipMemcpyAsync(uvn, c->trk_uvn.p + 2 * base, sizeof(float) * 2 * k, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}

int ovgpu_tracks_group_order(ovgpu_ctx *c, int32_t order) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null context");
  if (order != OVGPU_GROUPS_REFERENCE && order != OVGPU_GROUPS_DESCENDING && order != OVGPU_GROUPS_ASCENDING)
    return set_err(OVGPU_ERR_INVALID, "unknown camera-group order");
  c->trk_group_order = order;
  return OVGPU_OK;
}

int ovgpu_tracks_to_features(ovgpu_ctx *c, int32_t F, const int64_t *featid, const double *clone_times) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state must precede ovgpu_tracks_to_features");
  if (c->trk_max <= 0) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_tracks_create was never called");
  if (F < 0 || (F > 0 && !featid) || !clone_times) return set_err(OVGPU_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int C = c->C, K = c->K;
  std::vector<int32_t> sel(std::max(F, 1), -1);
  for (int f = 0; f < F; f++) {
    auto it = c->trk_slot_of.find(featid[f]);
    if (it != c->trk_slot_of.end()) sel[f] = it->second;
  }
  HIPCHK(c->trk_sel.reserve(std::max(F, 1)));
  HIPCHK(c->trk_nvalid.reserve(std::max(F, 1)));
  HIPCHK(c->trk_clone_times.reserve(C));
  HIPCHK(upload(c->trk_sel.p, sel.data(), sizeof(int32_t) * F, s));
  HIPCHK(upload(c->trk_clone_times.p, clone_times, sizeof(double) * C, s));
  // the order in which the reference would walk each feature's camera groups: reverse order of first insertion (k_tracks.h)
  const int8_t *order_dev = nullptr;
  std::vector<int8_t> order_h;
  if (c->trk_group_order == OVGPU_GROUPS_REFERENCE && F > 0) {
    order_h.assign((size_t)F * K, (int8_t)-1);
    for (int f = 0; f < F; f++) {
      if (sel[f] < 0) continue;
      const std::vector<int8_t> &cams = c->trk_h_cams[sel[f]];
      int w = 0;
      for (int e = (int)cams.size() - 1; e >= 0 && w < K; e--)
        if (cams[e] < K) order_h[(size_t)f * K + w++] = cams[e];
    }
    HIPCHK(c->trk_order.reserve(order_h.size()));
    HIPCHK(upload(c->trk_order.p, order_h.data(), order_h.size(), s));
    order_dev = c->trk_order.p;
  }
  const int desc = c->trk_group_order != OVGPU_GROUPS_ASCENDING;
  std::vector<int32_t> offs(F + 1, 0);
  if (F > 0) {
    hipLaunchKernelGGL(k_tracks_gather, dim3((F + 127) / 128), dim3(128), 0, s, F, K, C, c->trk_sel.p, c->trk_clone_times.p, track_store(c), c->trk_nvalid.p,
                       (const int32_t *)nullptr, (float *)nullptr, (float *)nullptr, (uint16_t *)nullptr, 0, desc, order_dev);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> nv(F);
    HIPCHK(hipMemcpyAsync(nv.data(), c->trk_nvalid.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
    for (int f = 0; f < F; f++) offs[f + 1] = offs[f] + nv[f];
  } else {
    HIPCHK(upload_sync(c, s));
  }
  HIPCHK(c->up.begin()); // the stream is idle: the page-locked upload arena starts over
  const int M = offs[F];
  int rc = begin_feature_batch(c, F, M, offs.data());
  if (rc != OVGPU_OK) return rc;
  HIPCHK(c->up.flush()); // (the gather below reads the offsets begin_feature_batch packed)
  if (F > 0) {
    const Batch b = batch_of(c); // (the batch begin_feature_batch made room for)
    hipLaunchKernelGGL(k_tracks_gather, dim3((F + 127) / 128), dim3(128), 0, s, F, K, C, c->trk_sel.p, c->trk_clone_times.p, track_store(c), c->trk_nvalid.p,
                       (const int32_t *)b.meas_offsets, b.uv, b.uvn, b.meas_cc, 1, desc, order_dev);
    HIPCHK(hipGetLastError());
  }
  return end_feature_batch(c);
}

int ovgpu_get_features(ovgpu_ctx *c, int32_t *F_out, int32_t *M_out, int32_t *meas_offsets, float *uv, float *uvn, int32_t *clone_idx, int32_t *cam_idx) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "no feature batch is resident");
  HIPCHK(hipSetDevice(c->device));
  const Batch b = batch_of(c);
  const int F = b.F, M = b.M;
  if (F_out) *F_out = F;
  if (M_out) *M_out = M;
  if (meas_offsets) std::memcpy(meas_offsets, b.h_offsets.p, sizeof(int32_t) * (F + 1));
  hipStream_t s = c->stream;
  const bool want_cc = clone_idx || cam_idx, want_any = M > 0 && (uv || uvn || want_cc);
  if (!want_any) return OVGPU_OK; // offsets and counts only (the drop-in's length check): host tables, no copy, no synchronisation
  std::vector<uint16_t> cc(want_cc ? std::max(M, 1) : 1);
  if (uv) HIPCHK(hipMemcpyAsync(uv, b.uv, sizeof(float) * 2 * M, hipMemcpyDeviceToHost, s));
  if (uvn) HIPCHK(hipMemcpyAsync(uvn, b.uvn, sizeof(float) * 2 * M, hipMemcpyDeviceToHost, s));
  if (want_cc) HIPCHK(hipMemcpyAsync(cc.data(), b.meas_cc, sizeof(uint16_t) * M, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  for (int i = 0; want_cc && i < M; i++) {
    if (clone_idx) clone_idx[i] = anchor_clone(cc[i]);
    if (cam_idx) cam_idx[i] = anchor_cam(cc[i]);
  }
  return OVGPU_OK;
}

// ---------------------------------------------------------------------------
// UpdaterHelper::measurement_compress_inplace and StateHelper::EKFUpdate as standalone calls on a
// caller-supplied dense system (UpdaterZeroVelocity.cpp:183-321 uses them this way)
// ---------------------------------------------------------------------------
struct DenseJob { // temporarily re-targets the context's compression buffers at a (rows x cols) system
  ovgpu_ctx *c;
  int D, LD, W;
  int64_t rows_total, rows_per_node;
  explicit DenseJob(ovgpu_ctx *ctx) : c(ctx), D(ctx->D), LD(ctx->LD), W(ctx->W), rows_total(ctx->rows_total), rows_per_node(ctx->rows_per_node) {}
  ~DenseJob() { c->D = D, c->LD = LD, c->W = W, c->rows_total = rows_total, c->rows_per_node = rows_per_node; }
};

// uploads [H | res] and runs the TSQR; the triangle ends in c->Rws (cols x (cols + 1))
static int dense_compress(ovgpu_ctx *c, int rows, int cols, const double *H, const double *res) {
  if (rows < 0 || cols <= 0 || cols + 1 > 512) return set_err(OVGPU_ERR_INVALID, "bad system size");
  if (rows > 0 && (!H || !res)) return set_err(OVGPU_ERR_INVALID, "null system");
  HIPCHK(hipSetDevice(c->device));
  c->D = cols, c->LD = cols + 1, c->rows_total = rows;
  int rc = configure_tsqr(c);
  if (rc != OVGPU_OK) return rc;
  std::vector<double> st((size_t)std::max(rows, 1) * c->LD);
  for (int i = 0; i < rows; i++) {
    std::memcpy(&st[(size_t)i * c->LD], H + (size_t)i * cols, sizeof(double) * cols);
    st[(size_t)i * c->LD + cols] = res[i];
  }
  if (rows > 0) HIPCHK(upload(c->Hbig.p, st.data(), sizeof(double) * (size_t)rows * c->LD, c->stream));
  HIPCHK(upload_sync(c, c->stream));
  if (rows == 0) {
    HIPCHK(hipMemsetAsync(c->Rws.p, 0, sizeof(double) * (size_t)cols * c->LD, c->stream));
    return OVGPU_OK;
  }
  return enqueue_compress(c);
}
