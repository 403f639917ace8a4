// api_standalone.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): stand-alone measurement_compress / EKFUpdate, the building blocks of the host-driven sharded update, camera models, synchronisation.
int ovgpu_measurement_compress(ovgpu_ctx *c, int rows, int cols, const double *H, const double *res, double *H_out, double *res_out, int32_t *rows_out) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (rows <= cols) { // UpdaterHelper.cpp:459-460: nothing to compress
    if (H_out && H && H_out != H) std::memcpy(H_out, H, sizeof(double) * (size_t)rows * cols);
    if (res_out && res && res_out != res) std::memcpy(res_out, res, sizeof(double) * rows);
    if (rows_out) *rows_out = rows;
    return OVGPU_OK;
  }
  DenseJob job(c);
  int rc = dense_compress(c, rows, cols, H, res);
  if (rc != OVGPU_OK) return rc;
  const int LD = cols + 1;
  std::vector<double> tri((size_t)cols * LD);
  HIPCHK(hipMemcpyAsync(tri.data(), c->Rws.p, sizeof(double) * tri.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(upload_sync(c, c->stream));
  for (int i = 0; i < cols; i++) {
    if (H_out) std::memcpy(H_out + (size_t)i * cols, &tri[(size_t)i * LD], sizeof(double) * cols);
    if (res_out) res_out[i] = tri[(size_t)i * LD + cols];
  }
  if (rows_out) *rows_out = cols; // :481-486
  return check_tree_error(c);
}

int ovgpu_ekf_update(ovgpu_ctx *c, int rows, int cols, const int32_t *col_cov_id, const double *H, const double *res, double sigma2, double *dx,
                     double *P_out) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (!col_cov_id || sigma2 < 0.0) return set_err(OVGPU_ERR_INVALID, "bad argument");
  for (int i = 0; i < cols; i++)
    if (col_cov_id[i] < 0 || col_cov_id[i] >= c->N) return set_err(OVGPU_ERR_INVALID, "column id outside the covariance");
  int rc;
  {
    DenseJob job(c);
    // the EKF kernels take an upper-triangular system: any (rows x cols) stack goes through the QR first (an orthogonal
    // transform of the rows changes neither K res nor K H P; the reference's EKFUpdate uses H as given)
    rc = dense_compress(c, rows, cols, H, res);
    if (rc != OVGPU_OK) return rc;
    DevBuf<int32_t> cols_dev;
    HIPCHK(cols_dev.reserve(cols));
    HIPCHK(upload(cols_dev.p, col_cov_id, sizeof(int32_t) * cols, c->stream));
    HIPCHK(c->Mt.reserve((size_t)cols * c->N));
    HIPCHK(c->Aaug.reserve((size_t)cols * (cols + c->N + 1)));
    HIPCHK(c->Yaug.reserve((size_t)cols * (cols + c->N + 1)));
    EkfJob ej;
    ej.col_cov = cols_dev.p, ej.sigma2 = sigma2;
    rc = enqueue_ekf(c, ej);
    if (rc == OVGPU_OK) rc = finish_update(c, dx, P_out, nullptr);
  }
  // the context's own workspaces are sized by its column map again
  HIPCHK(c->Mt.reserve((size_t)c->D * c->N));
  HIPCHK(c->Aaug.reserve((size_t)c->D * (c->D + c->N + 1)));
  HIPCHK(c->Yaug.reserve((size_t)c->D * (c->D + c->N + 1)));
  c->tri_readable = false;
  c->have_feats = false; // Hbig / Rws were re-targeted: upload the feature batch again before the next feature update
  return rc;
}

int ovgpu_triangle_len(ovgpu_ctx *c, int64_t *n_doubles) {
  if (!c || !n_doubles) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  *n_doubles = (int64_t)c->D * c->LD;
  return OVGPU_OK;
}

int ovgpu_msckf_local(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, void *tri_dev,
                      ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  int rc = enqueue_pipeline(c, STAGE_LOCAL);
  if (rc != OVGPU_OK) return rc;
  if (tri_dev) HIPCHK(hipMemcpyAsync(tri_dev, c->Rws.p, sizeof(double) * c->D * c->LD, hipMemcpyDeviceToDevice, c->stream));
  if (feat_status || chi2 || chi2_thresh || p_FinG || stats) {
    rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, stats);
    if (rc != OVGPU_OK) return rc;
    fill_times(c, stats);
  } else {
    HIPCHK(upload_sync(c, c->stream)); // tri_dev is consumed by another library's stream (RCCL)
  }
  return OVGPU_OK;
}

// ---- the same exchange in Gram form: G_total = sum over GPUs of [H_g | r_g]^T [H_g | r_g] is ONE all-reduce (sum) of
// 16 NT x 16 NT doubles + the accepted-row count; every rank then factors and updates identically
__global__ void k_gram_count(double *dst, const int32_t *rows_used) { dst[0] = (double)rows_used[0]; }

int ovgpu_gram_len(ovgpu_ctx *c, int64_t *n_doubles) {
  if (!c || !n_doubles) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  const int NT = (c->LD + 15) / 16;
  if (NT > gram::GR_NT_BLK) return set_err(OVGPU_ERR_CAPACITY, "the Gram route holds at most 383 Jacobian columns");
  *n_doubles = (int64_t)256 * NT * NT + 1;
  return OVGPU_OK;
}

int ovgpu_msckf_local_gram(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, void *gram_dev,
                           ovgpu_update_stats *stats) {
  if (!c || !gram_dev) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  HIPCHK(hipSetDevice(c->device));
  int rc = OVGPU_OK;
  // the prior block's factorisation (its factor whitens the local stack, and the update that follows, ovgpu_msckf_gram_update,
  // continues from it) is enqueued by the pipeline: second stream, next to the triangulation
  c->prior_pending = false;
  rc = enqueue_pipeline(c, STAGE_LOCAL, false, true, true);
  if (rc != OVGPU_OK) return rc;
  const size_t n = (size_t)256 * ((c->LD + 15) / 16) * ((c->LD + 15) / 16);
  double *dst = static_cast<double *>(gram_dev);
  if (batch_of(c).F > 0) {
    HIPCHK(hipMemcpyAsync(dst, c->gram_G.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_gram_count, dim3(1), dim3(1), 0, c->stream, dst + n, c->rows_used.p);
    HIPCHK(hipGetLastError());
  } else { // an empty shard: nothing was whitened here, but the sum ovgpu_msckf_gram_update receives is the other ranks' whitened Gram matrix
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(double) * (n + 1), c->stream));
    c->gram_is_whitened = c->whiten;
  }
  if (feat_status || chi2 || chi2_thresh || p_FinG || stats) {
    rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, stats);
    if (rc != OVGPU_OK) return rc;
    fill_times(c, stats);
  } else {
    HIPCHK(upload_sync(c, c->stream)); // gram_dev is consumed by another library's stream (RCCL)
  }
  return OVGPU_OK;
}

int ovgpu_msckf_gram_update(ovgpu_ctx *c, const void *gram_dev, double *dx, double *P_out, ovgpu_update_stats *stats) {
  if (!c || !gram_dev) return set_err(OVGPU_ERR_INVALID, "bad argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  const int NT = (c->LD + 15) / 16;
  if (NT > gram::GR_NT_BLK) return set_err(OVGPU_ERR_CAPACITY, "the Gram route holds at most 383 Jacobian columns");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)256 * NT * NT;
  HIPCHK(c->gram_G.reserve(n));
  HIPCHK(c->Rws.reserve((size_t)16 * c->D * c->LD));
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(c->gram_G.p, gram_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  // the Gram matrices of all ranks were formed with this rank's own factor of the (replicated) prior: c->gram_is_whitened
  int rc = enqueue_ekf_gram(c, c->prior_pending ? 2 : 3);
  c->prior_pending = false;
  if (rc != OVGPU_OK) return rc;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->D = c->D;
    stats->n_rows_comp = c->D;
  }
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
  if (dx) HIPCHK(hipMemcpyAsync(dx, c->dx.p, sizeof(double) * c->N, hipMemcpyDeviceToHost, s));
  if (P_out) HIPCHK(hipMemcpyAsync(P_out, c->P.p, sizeof(double) * c->N * c->N, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  // a follower's time-out switched the kernels behind the factorisation off: nothing was modified, and dx / P_out are not an update's
  if (flags[2]) {
    c->chol_timeouts++;
    return set_err(OVGPU_ERR_HIP, CHOL_TIMED_OUT "; the state was not modified: call again with the same buffer" CHOL_STEPWISE_HINT);
  }
  const int status = flags[0] ? OVGPU_ERR_NOT_SPD : (flags[1] ? OVGPU_ERR_NEGATIVE_DIAGONAL : OVGPU_OK);
  if (stats) stats->status = status;
  if (status != OVGPU_OK) return set_err(status, "EKF update failed");
  return OVGPU_OK;
}

int ovgpu_msckf_merge_update(ovgpu_ctx *c, const void *tris_dev, int G, double *dx, double *P_out, ovgpu_update_stats *stats) {
  if (!c || !tris_dev || G < 1) return set_err(OVGPU_ERR_INVALID, "bad argument");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  HIPCHK(hipSetDevice(c->device));
  const size_t tri = (size_t)c->D * c->LD;
  HIPCHK(c->Rws.reserve(std::max<size_t>((size_t)G, 16) * tri));
  HIPCHK(hipMemcpyAsync(c->Rws.p, tris_dev, sizeof(double) * tri * G, hipMemcpyDeviceToDevice, c->stream));
  int rc = enqueue_merge_tree(c, G);
  if (rc != OVGPU_OK) return rc;
  rc = enqueue_ekf(c);
  if (rc != OVGPU_OK) return rc;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->D = c->D;
    stats->n_rows_comp = c->D;
  }
  ovgpu_update_stats *no_times = nullptr;
  (void)no_times;
  hipStream_t s = c->stream;
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
  if (dx) HIPCHK(hipMemcpyAsync(dx, c->dx.p, sizeof(double) * c->N, hipMemcpyDeviceToHost, s));
  if (P_out) HIPCHK(hipMemcpyAsync(P_out, c->P.p, sizeof(double) * c->N * c->N, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  if (flags[2]) { // (as ovgpu_msckf_gram_update)
    c->chol_timeouts++;
    return set_err(OVGPU_ERR_HIP, CHOL_TIMED_OUT "; no update was applied: upload the state again, then repeat the call" CHOL_STEPWISE_HINT);
  }
  int status = flags[0] ? OVGPU_ERR_NOT_SPD : (flags[1] ? OVGPU_ERR_NEGATIVE_DIAGONAL : OVGPU_OK);
  if (stats) stats->status = status;
  if (status != OVGPU_OK) return set_err(status, "EKF update failed");
  return check_tree_error(c);
}

// diagnostic kernel: evaluates the device camera model on a batch of normalized points
__global__ void k_cam_distort(int n, int fisheye, const double *__restrict__ cam8, const double *__restrict__ uvn, double *uv, double *dzn, double *dze) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CamIntr ci = load_cam(cam8);
  double u, v, a[4], b[16];
  if (fisheye) {
    equi_distort_d(ci, uvn[2 * i], uvn[2 * i + 1], u, v);
    equi_jacobian(ci, uvn[2 * i], uvn[2 * i + 1], a, b);
  } else {
    radtan_distort_d(ci, uvn[2 * i], uvn[2 * i + 1], u, v);
    radtan_jacobian(ci, uvn[2 * i], uvn[2 * i + 1], a, b);
  }
  uv[2 * i] = u, uv[2 * i + 1] = v;
  for (int k = 0; k < 4; k++) dzn[4 * i + k] = a[k];
  for (int k = 0; k < 16; k++) dze[16 * i + k] = b[k];
}

int ovgpu_cam_distort(ovgpu_ctx *c, int is_fisheye, const double *cam8, int n, const double *uv_norm, double *uv_dist, double *dz_dzn, double *dz_dzeta) {
  if (!c || !cam8 || !uv_norm || n < 0) return set_err(OVGPU_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  DevBuf<double> d_cam, d_in, d_uv, d_a, d_b;
  HIPCHK(d_cam.reserve(8));
  HIPCHK(d_in.reserve((size_t)2 * n));
  HIPCHK(d_uv.reserve((size_t)2 * n));
  HIPCHK(d_a.reserve((size_t)4 * n));
  HIPCHK(d_b.reserve((size_t)16 * n));
  hipStream_t s = c->stream;
  HIPCHK(upload(d_cam.p, cam8, 8 * sizeof(double), s));
  HIPCHK(upload(d_in.p, uv_norm, sizeof(double) * 2 * n, s));
  if (n > 0) hipLaunchKernelGGL(k_cam_distort, dim3((n + 255) / 256), dim3(256), 0, s, n, is_fisheye, d_cam.p, d_in.p, d_uv.p, d_a.p, d_b.p);
  HIPCHK(hipGetLastError());
  if (uv_dist) HIPCHK(hipMemcpyAsync(uv_dist, d_uv.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, s));
  if (dz_dzn) HIPCHK(hipMemcpyAsync(dz_dzn, d_a.p, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, s));
  if (dz_dzeta) HIPCHK(hipMemcpyAsync(dz_dzeta, d_b.p, sizeof(double) * 16 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}

int ovgpu_synchronize(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(upload_sync(c, c->stream));
  if (c->async_pending) { // the status of the last ovgpu_msckf_update_async (a synchronous call reports its own)
    c->async_pending = false;
    int32_t flags[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[2]) return set_err(OVGPU_ERR_HIP, "single-launch Cholesky: a follower workgroup timed out waiting for the factor workgroup; the state was not modified (the synchronous calls repeat the update with the step-wise kernels)");
    if (flags[0]) return set_err(OVGPU_ERR_NOT_SPD, c->last_update_tform ? "prior block of the involved variables not positive definite (state untouched; ovgpu_msckf_update falls back to the Householder route)" : "innovation covariance not SPD");
    if (flags[1]) return set_err(OVGPU_ERR_NEGATIVE_DIAGONAL, "negative covariance diagonal after the update");
  }
  return check_tree_error(c);
}
