// api_multi.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): multi-GPU: RCCL resolved at run time, ovgpu_comm_*, ovgpu_msckf_update_sharded, one-process ovgpu_multi_*.

// ---------------------------------------------------------------------------------------------------------------------
// Native multi-GPU exchange (SURVEY.md 8e): features shard across GPUs, every GPU accumulates the Gram matrix of ITS whitened
// stack (the prior and therefore its factor L are replicated, so the stacks are whitened identically), ONE ncclAllReduce (sum)
// of 16 NT x 16 NT doubles on the context's stream, every GPU applies the identical update.  No host synchronisation between the
// local stage, the collective and the update; the prior block's factorisation runs on the second stream next to all of it.
// RCCL is resolved at run time (dlopen librccl.so.1: the copy already in the process, e.g. PyTorch's, is reused).
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
  void *h = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, ovgpu_comm_id, int) = nullptr;
  int (*CommInitAll)(void **, int, const int *) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*CommCount)(void *, int *) = nullptr;    // (optional: ovgpu_comm_info)
  int (*CommUserRank)(void *, int *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  bool ok = false;
};
Rccl &rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  for (const char *name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
    r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (r.h) break;
  }
  if (!r.h) return r;
  auto sym = [&](const char *n) { return dlsym(r.h, n); };
  r.GetUniqueId = (int (*)(void *))sym("ncclGetUniqueId");
  r.CommInitRank = (int (*)(void **, int, ovgpu_comm_id, int))sym("ncclCommInitRank");
  r.CommInitAll = (int (*)(void **, int, const int *))sym("ncclCommInitAll");
  r.CommDestroy = (int (*)(void *))sym("ncclCommDestroy");
  r.CommCount = (int (*)(void *, int *))sym("ncclCommCount");
  r.CommUserRank = (int (*)(void *, int *))sym("ncclCommUserRank");
  r.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))sym("ncclAllReduce");
  r.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))sym("ncclAllGather");
  r.GroupStart = (int (*)())sym("ncclGroupStart");
  r.GroupEnd = (int (*)())sym("ncclGroupEnd");
  r.GetErrorString = (const char *(*)(int))sym("ncclGetErrorString");
  r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.AllReduce && r.AllGather && r.GroupStart && r.GroupEnd;
  return r;
}
constexpr int NCCL_DOUBLE = 8, NCCL_SUM = 0; // rccl.h: ncclFloat64 = 8, ncclSum = 0
int nccl_err(int rc, const char *what) {
  Rccl &r = rccl();
  return set_err(OVGPU_ERR_HIP, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}
} // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Loop-back collective: G ranks that share ONE device (ovgpu_multi_create with a repeated device id).  RCCL refuses such a
// communicator, and this machine pool leases one GPU at a time — so without it the G > 1 branches of the sharded update (the
// empty shard's zero contribution, the triangle all-gather + merge tree of the Householder protocol, the Gram all-reduce feeding
// G identical updates) would never execute on hardware before the first multi-GPU run.  Semantics of the real thing: every rank
// marks its buffer ready on its own stream; when all have, the sum (rank order: bit-identical on every rank) / the concatenation is
// delivered to every rank's stream.  A test double of the TRANSPORT only: everything before and after it is the production path.
// ---------------------------------------------------------------------------------------------------------------------
struct LoopComm {
  int G = 0;
  std::vector<ovgpu_ctx *> ranks;
  std::vector<Event> ready;
  Event done;
  DevBuf<double> sum;
};
struct LoopPtrs {
  const double *p[8];
};
__global__ void k_loop_sum(int64_t n, int G, LoopPtrs in, double *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = in.p[0][i];
  for (int g = 1; g < G; g++) s += in.p[g][i];
  out[i] = s;
}
// called once per exchange, after every rank has been through sharded_exchange (its buffer is final on its stream)
static int loop_finish(LoopComm *L, bool gram) {
  const int G = L->G;
  for (int g = 0; g < G; g++) HIPCHK(hipEventRecord(L->ready[g], L->ranks[g]->stream));
  ovgpu_ctx *c0 = L->ranks[0];
  if (gram) {
    const size_t n = (size_t)256 * ((c0->LD + 15) / 16) * ((c0->LD + 15) / 16);
    HIPCHK(L->sum.reserve(n));
    LoopPtrs in;
    for (int g = 0; g < 8; g++) in.p[g] = L->ranks[g < G ? g : 0]->gram_G.p;
    for (int g = 0; g < G; g++) HIPCHK(hipStreamWaitEvent(c0->stream, L->ready[g], 0));
    hipLaunchKernelGGL(k_loop_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c0->stream, (int64_t)n, G, in, L->sum.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(L->done, c0->stream));
    for (int g = 0; g < G; g++) {
      HIPCHK(hipStreamWaitEvent(L->ranks[g]->stream, L->done, 0));
      HIPCHK(hipMemcpyAsync(L->ranks[g]->gram_G.p, L->sum.p, sizeof(double) * n, hipMemcpyDeviceToDevice, L->ranks[g]->stream));
    }
    return OVGPU_OK;
  }
  const size_t tri = (size_t)c0->D * c0->LD;
  for (int g = 0; g < G; g++) {
    ovgpu_ctx *c = L->ranks[g];
    for (int h = 0; h < G; h++) HIPCHK(hipStreamWaitEvent(c->stream, L->ready[h], 0));
    for (int h = 0; h < G; h++)
      HIPCHK(hipMemcpyAsync(c->comm_buf.p + (size_t)h * tri, L->ranks[h]->Rws.p, sizeof(double) * tri, hipMemcpyDeviceToDevice, c->stream));
  }
  // nobody may overwrite its triangle (the merge tree works in Rws) before every rank has copied it
  for (int g = 0; g < G; g++) HIPCHK(hipEventRecord(L->ready[g], L->ranks[g]->stream));
  for (int g = 0; g < G; g++)
    for (int h = 0; h < G; h++) HIPCHK(hipStreamWaitEvent(L->ranks[g]->stream, L->ready[h], 0));
  return OVGPU_OK;
}

// the local stage of a sharded update up to (not including) the exchange; gram: which protocol this state uses
static int sharded_local(ovgpu_ctx *c, bool &gram) {
  gram = c->compress_gram == 1 && (c->LD + 15) / 16 <= gram::GR_NT_BLK && !c->force_tsqr;
  const int rc = enqueue_pipeline(c, STAGE_LOCAL, false, true, gram);
  if (rc == OVGPU_OK && gram && batch_of(c).F == 0) { // an empty shard: nothing was whitened here, but the sum it joins is the other ranks' whitened Gram matrix
    const size_t n = (size_t)256 * ((c->LD + 15) / 16) * ((c->LD + 15) / 16);
    HIPCHK(c->gram_G.reserve(n));
    c->gram_is_whitened = c->whiten;
  }
  return rc;
}
// the exchange and the update behind it, all on the context's stream; grouped: the caller brackets several ranks' calls with
// ncclGroupStart / ncclGroupEnd (single-process multi-device)
static int sharded_exchange(ovgpu_ctx *c, bool gram) {
  Rccl &r = rccl();
  const int G = c->comm_world;
  if (gram) {
    const size_t n = (size_t)256 * ((c->LD + 15) / 16) * ((c->LD + 15) / 16);
    if (batch_of(c).F == 0) HIPCHK(hipMemsetAsync(c->gram_G.p, 0, sizeof(double) * n, c->stream)); // an empty shard contributes nothing
    if (c->loop) return OVGPU_OK; // (loop_finish delivers the sum once every rank is here)
    if (G > 1) {
      const int rc = r.AllReduce(c->gram_G.p, c->gram_G.p, n, NCCL_DOUBLE, NCCL_SUM, c->comm, c->stream);
      if (rc != 0) return nccl_err(rc, "ncclAllReduce");
    }
    return OVGPU_OK;
  }
  const size_t tri = (size_t)c->D * c->LD;
  HIPCHK(c->comm_buf.reserve(tri * G));
  if (batch_of(c).F == 0) { // an empty shard's triangle is all zeros (the leaf kernels never ran): say so explicitly before it is gathered
    HIPCHK(c->Rws.reserve(tri));
    HIPCHK(hipMemsetAsync(c->Rws.p, 0, sizeof(double) * tri, c->stream));
  }
  if (c->loop) return OVGPU_OK;
  if (G > 1) {
    const int rc = r.AllGather(c->Rws.p, c->comm_buf.p, tri, NCCL_DOUBLE, c->comm, c->stream);
    if (rc != 0) return nccl_err(rc, "ncclAllGather");
  }
  return OVGPU_OK;
}
static int sharded_update(ovgpu_ctx *c, bool gram) {
  c->last_route = gram ? OVGPU_COMPRESS_GRAM : OVGPU_COMPRESS_TSQR; // ovgpu_last_update_route: the exchange this rank took (the pipeline sets it for STAGE_EKF only)
  if (gram) return enqueue_ekf_gram(c, c->prior_pending ? 2 : 3);
  const int G = c->comm_world;
  if (G > 1) {
    const size_t tri = (size_t)c->D * c->LD;
    HIPCHK(c->Rws.reserve(std::max<size_t>((size_t)G, 16) * tri));
    HIPCHK(hipMemcpyAsync(c->Rws.p, c->comm_buf.p, sizeof(double) * tri * G, hipMemcpyDeviceToDevice, c->stream));
    const int rc = enqueue_merge_tree(c, G);
    if (rc != OVGPU_OK) return rc;
  }
  return enqueue_ekf(c);
}

extern "C" {

int ovgpu_comm_unique_id(ovgpu_comm_id *id) {
  if (!id) return set_err(OVGPU_ERR_INVALID, "null argument");
  Rccl &r = rccl();
  if (!r.ok) return set_err(OVGPU_ERR_HIP, "RCCL (librccl.so.1) is not available in this process");
  const int rc = r.GetUniqueId(id);
  return rc == 0 ? OVGPU_OK : nccl_err(rc, "ncclGetUniqueId");
}

int ovgpu_comm_init_rank(ovgpu_ctx *c, const ovgpu_comm_id *id, int rank, int world) {
  if (!c || !id || world < 1 || rank < 0 || rank >= world) return set_err(OVGPU_ERR_INVALID, "bad argument");
  Rccl &r = rccl();
  if (!r.ok) return set_err(OVGPU_ERR_HIP, "RCCL (librccl.so.1) is not available in this process");
  HIPCHK(hipSetDevice(c->device));
  if (c->comm) (void)r.CommDestroy(c->comm), c->comm = nullptr;
  const int rc = r.CommInitRank(&c->comm, world, *id, rank);
  if (rc != 0) return nccl_err(rc, "ncclCommInitRank");
  c->comm_rank = rank, c->comm_world = world;
  return OVGPU_OK;
}

// What the COMMUNICATOR says about itself (ncclCommCount / ncclCommUserRank), next to what ovgpu_comm_init_rank was told: a multi-GPU bench
// line carries both, so that a reader can check that RCCL really saw N ranks.  -1 where no communicator exists (a world of one never
// issues a collective) or the installed RCCL lacks the query.
int ovgpu_comm_info(ovgpu_ctx *c, int32_t *rank_told, int32_t *world_told, int32_t *rccl_rank, int32_t *rccl_ranks) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (rank_told) *rank_told = c->comm_rank;
  if (world_told) *world_told = c->comm_world;
  int r = -1, n = -1;
  Rccl &lib = rccl();
  if (c->comm && lib.CommCount && lib.CommUserRank) {
    if (lib.CommCount(c->comm, &n) != 0) n = -1;
    if (lib.CommUserRank(c->comm, &r) != 0) r = -1;
  }
  if (rccl_rank) *rccl_rank = r;
  if (rccl_ranks) *rccl_ranks = n;
  return OVGPU_OK;
}

int ovgpu_comm_destroy(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (c->comm) {
    (void)hipSetDevice(c->device);
    (void)upload_sync(c, c->stream);
    (void)rccl().CommDestroy(c->comm);
    c->comm = nullptr;
  }
  c->comm_rank = 0, c->comm_world = 1;
  return OVGPU_OK;
}

int ovgpu_msckf_update_sharded_async(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (c->loop) return set_err(OVGPU_ERR_INVALID, "ranks that share a device are driven through ovgpu_multi_msckf_update");
  if (c->comm_world > 1 && !c->comm) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_comm_init_rank was never called");
  bool gram = false;
  int rc = sharded_local(c, gram);
  if (rc != OVGPU_OK) return rc;
  if ((rc = sharded_exchange(c, gram)) != OVGPU_OK) return rc;
  c->async_pending = true;
  return sharded_update(c, gram);
}

int ovgpu_msckf_update_sharded(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out,
                               ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  // Of the one-GPU update's fall-backs only the REPLICATED condition repeats here: the prior is the same on every rank, so every
  // rank sees OVGPU_ERR_NOT_SPD together and every rank repeats (the Householder repeat exchanges triangles instead of Gram
  // matrices: the collective stays matched).  The single-launch Cholesky's follower time-out is a scheduling event of ONE rank: a
  // local repeat would issue a collective its peers never match.  In a world of more than one rank it is therefore returned as
  // OVGPU_ERR_HIP: THIS rank's state is untouched while its peers have applied the update, so the caller uploads the state again on
  // every rank (options.no_single_launch_cholesky = 1 rules the time-out out); a world of one keeps the local repeat.
  return update_with_fallbacks(c, stats, [&]() {
    int rc = ovgpu_msckf_update_sharded_async(c);
    if (rc != OVGPU_OK) return rc;
    c->async_pending = false;
    PendingFeatOut pend; // one synchronisation for the per-feature outputs and dx / P'
    if ((rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, stats, &pend, finish_update_bytes(c))) != OVGPU_OK) return rc;
    return finish_update(c, dx, P_out, stats, &pend);
  }, c->comm_world <= 1);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// One host process, several GPUs (the reference's host is ONE C++ process, VioManager.cpp:155-156, :518-526): a set of contexts,
// the feature batch dealt round-robin by track length, the exchange grouped over the set's communicators.
// ---------------------------------------------------------------------------------------------------------------------
struct ovgpu_multi {
  std::vector<ovgpu_ctx *> ctx;
  LoopComm *loop = nullptr; // a device appears more than once: loop-back collective instead of RCCL
  std::vector<std::vector<int32_t>> feat_of; // per device: global feature index of each local feature
  int F = 0;
};

extern "C" {

int ovgpu_multi_create(const ovgpu_options *opts, int n, const int *devices, ovgpu_multi **out) {
  if (!opts || !out || n < 1) return set_err(OVGPU_ERR_INVALID, "bad argument");
  *out = nullptr;
  Rccl &r = rccl();
  std::vector<int> devs(n);
  for (int i = 0; i < n; i++) devs[i] = devices ? devices[i] : i;
  bool repeated = false;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++) repeated = repeated || devs[i] == devs[j];
  if (repeated && n > 8) return set_err(OVGPU_ERR_CAPACITY, "at most 8 ranks on one device");
  if (n > 1 && !repeated && !r.ok) return set_err(OVGPU_ERR_HIP, "RCCL (librccl.so.1) is not available in this process");
  ovgpu_multi *m = new ovgpu_multi();
  for (int i = 0; i < n; i++) {
    ovgpu_ctx *c = nullptr;
    const int rc = ovgpu_create(opts, devs[i], &c);
    if (rc != OVGPU_OK) {
      for (auto *x : m->ctx) ovgpu_destroy(x);
      delete m;
      return rc;
    }
    m->ctx.push_back(c);
  }
  if (n > 1 && repeated) { // several ranks on one device: the loop-back collective (see LoopComm)
    LoopComm *L = new LoopComm();
    L->G = n, L->ranks = m->ctx, L->ready.resize(n);
    bool ok = L->done.create(hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < n; i++) ok = ok && L->ready[i].create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      for (auto *x : m->ctx) ovgpu_destroy(x);
      delete L;
      delete m;
      return set_err(OVGPU_ERR_HIP, "event creation failed");
    }
    m->loop = L;
    for (int i = 0; i < n; i++) m->ctx[i]->loop = L, m->ctx[i]->comm_rank = i, m->ctx[i]->comm_world = n;
  } else if (n > 1) {
    std::vector<void *> comms(n, nullptr);
    const int rc = r.CommInitAll(comms.data(), n, devs.data());
    if (rc != 0) {
      for (auto *x : m->ctx) ovgpu_destroy(x);
      delete m;
      return nccl_err(rc, "ncclCommInitAll");
    }
    for (int i = 0; i < n; i++) m->ctx[i]->comm = comms[i], m->ctx[i]->comm_rank = i, m->ctx[i]->comm_world = n;
  }
  m->feat_of.resize(n);
  *out = m;
  return OVGPU_OK;
}

void ovgpu_multi_destroy(ovgpu_multi *m) {
  if (!m) return;
  for (auto *c : m->ctx) {
    (void)ovgpu_comm_destroy(c);
    c->loop = nullptr;
    ovgpu_destroy(c);
  }
  delete m->loop; // (every rank's streams are idle: its sum buffer and events go with it)
  delete m;
}

int ovgpu_multi_size(ovgpu_multi *m) { return m ? (int)m->ctx.size() : 0; }
ovgpu_ctx *ovgpu_multi_ctx(ovgpu_multi *m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }

int ovgpu_multi_set_state(ovgpu_multi *m, const ovgpu_state_view *st) {
  if (!m || !st) return set_err(OVGPU_ERR_INVALID, "null argument");
  for (auto *c : m->ctx) {
    const int rc = ovgpu_set_state(c, st);
    if (rc != OVGPU_OK) return rc;
  }
  return OVGPU_OK;
}

int ovgpu_multi_set_features(ovgpu_multi *m, const ovgpu_features_view *fv) {
  if (!m || !fv) return set_err(OVGPU_ERR_INVALID, "null argument");
  const int G = (int)m->ctx.size(), F = fv->F;
  // tracks sorted by length (the order VioManager.cpp:509-518 produces), dealt round-robin: every GPU gets the same mix
  std::vector<int32_t> order(F);
  for (int f = 0; f < F; f++) order[f] = f;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return fv->meas_offsets[a + 1] - fv->meas_offsets[a] > fv->meas_offsets[b + 1] - fv->meas_offsets[b];
  });
  m->F = F;
  for (int g = 0; g < G; g++) {
    std::vector<int32_t> &mine = m->feat_of[g];
    mine.clear();
    for (int k = g; k < F; k += G) mine.push_back(order[k]);
    std::sort(mine.begin(), mine.end());
    std::vector<int32_t> offs(1, 0), cl, cam;
    std::vector<float> uv, uvn;
    for (int32_t f : mine) {
      for (int i = fv->meas_offsets[f]; i < fv->meas_offsets[f + 1]; i++) {
        uv.push_back(fv->uv[2 * i]), uv.push_back(fv->uv[2 * i + 1]);
        uvn.push_back(fv->uvn[2 * i]), uvn.push_back(fv->uvn[2 * i + 1]);
        cl.push_back(fv->clone_idx[i]), cam.push_back(fv->cam_idx[i]);
      }
      offs.push_back((int32_t)cl.size());
    }
    ovgpu_features_view sub;
    sub.F = (int32_t)mine.size(), sub.M = (int32_t)cl.size();
    sub.meas_offsets = offs.data(), sub.uv = uv.data(), sub.uvn = uvn.data(), sub.clone_idx = cl.data(), sub.cam_idx = cam.data();
    const int rc = ovgpu_set_features(m->ctx[g], &sub); // synchronous upload: the staging vectors may go
    if (rc != OVGPU_OK) return rc;
  }
  return OVGPU_OK;
}

int ovgpu_multi_msckf_update(ovgpu_multi *m, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out,
                             ovgpu_update_stats *stats) {
  if (!m) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const int G = (int)m->ctx.size();
  Rccl &r = rccl();
  std::vector<char> gram(G, 0);
  int rc = OVGPU_OK;
  for (int g = 0; g < G; g++) { // local stages, asynchronous on every device
    bool gr = false;
    if ((rc = sharded_local(m->ctx[g], gr)) != OVGPU_OK) return rc;
    gram[g] = gr;
  }
  const bool rccl_group = G > 1 && !m->loop;
  if (rccl_group) (void)r.GroupStart();
  for (int g = 0; g < G; g++) {
    HIPCHK(hipSetDevice(m->ctx[g]->device));
    if ((rc = sharded_exchange(m->ctx[g], gram[g])) != OVGPU_OK) break;
  }
  if (rccl_group) {
    const int rg = r.GroupEnd();
    if (rc == OVGPU_OK && rg != 0) rc = nccl_err(rg, "ncclGroupEnd");
  }
  if (rc == OVGPU_OK && m->loop) rc = loop_finish(m->loop, gram[0] != 0);
  if (rc != OVGPU_OK) return rc;
  for (int g = 0; g < G; g++) {
    HIPCHK(hipSetDevice(m->ctx[g]->device));
    if ((rc = sharded_update(m->ctx[g], gram[g])) != OVGPU_OK) return rc;
  }
  // Every rank's factorisation flags BEFORE any result is taken.  A follower time-out of the single-launch Cholesky is local to one
  // rank (the factor workgroup was not co-scheduled there): that rank skipped its update while the others applied theirs, so the
  // replicas have diverged.  There is no local repeat that keeps the exchange matched (the one-GPU entry points repeat with the
  // step-wise kernels; here the peers have already moved on): the error is returned for the whole set and the caller uploads the
  // state again on every rank (ovgpu_multi_set_state) before the next update.
  for (int g = 0; g < G; g++) {
    ovgpu_ctx *c = m->ctx[g];
    HIPCHK(hipSetDevice(c->device));
    int32_t flags[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(flags, c->flags.p, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(upload_sync(c, c->stream));
    if (flags[2]) {
      c->chol_timeouts++;
      return set_err(OVGPU_ERR_HIP, "multi-device update: the single-launch Cholesky of one rank timed out; the ranks' states differ now -- "
                                    "upload the state again on every rank (options.no_single_launch_cholesky = 1 rules the time-out out)");
    }
  }
  // outputs: per-feature results from the shard that owns the feature, (dx, P') from device 0 (identical on all)
  ovgpu_update_stats total;
  std::memset(&total, 0, sizeof(total));
  for (int g = 0; g < G; g++) {
    ovgpu_ctx *c = m->ctx[g];
    HIPCHK(hipSetDevice(c->device));
    const int Fl = batch_of(c).F;
    std::vector<int32_t> st(Fl);
    std::vector<double> c2(Fl), th(Fl), pg((size_t)3 * Fl);
    ovgpu_update_stats loc;
    std::memset(&loc, 0, sizeof(loc));
    if ((rc = read_feature_outputs(c, st.data(), c2.data(), th.data(), pg.data(), &loc)) != OVGPU_OK) return rc;
    for (int k = 0; k < Fl; k++) {
      const int f = m->feat_of[g][k];
      if (feat_status) feat_status[f] = st[k];
      if (chi2) chi2[f] = c2[k];
      if (chi2_thresh) chi2_thresh[f] = th[k];
      if (p_FinG) std::memcpy(p_FinG + (size_t)3 * f, pg.data() + (size_t)3 * k, 3 * sizeof(double));
    }
    total.n_used += loc.n_used, total.n_rows += loc.n_rows, total.D = loc.D, total.n_gate_bound += loc.n_gate_bound;
    ovgpu_update_stats fin;
    std::memset(&fin, 0, sizeof(fin));
    if ((rc = finish_update(c, g == 0 ? dx : nullptr, g == 0 ? P_out : nullptr, &fin)) != OVGPU_OK) return rc;
    if (g == 0) total.status = fin.status, total.ms_total = fin.ms_total, total.ms_compress = fin.ms_compress, total.ms_system = fin.ms_system, total.ms_update = fin.ms_update;
  }
  total.n_rows_comp = total.n_rows > 0 ? total.D : 0;
  if (stats) *stats = total;
  return OVGPU_OK;
}

} // extern "C"
