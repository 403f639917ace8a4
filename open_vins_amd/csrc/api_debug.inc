// api_debug.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): developer aids: named debug options, cycle counters, stage timers.
int ovgpu_debug_option(ovgpu_ctx *c, const char *name, int64_t value, int64_t *old_value) {
  if (!c || !name) return set_err(OVGPU_ERR_INVALID, "null argument");
  const std::string n(name);
  if (n == "chol_follow_spin_limit") {
    if (old_value) *old_value = c->chol_spin_limit;
    if (value >= 0) c->chol_spin_limit = (int)std::min<int64_t>(value, 1 << 30);
  } else if (n == "slam_chunked_fail_chunk") { // k >= 0: the next ovgpu_slam_update_chunked reads chunk k's flag word as failed after its pass and takes the restore-and-chain path (one-shot)
    if (old_value) *old_value = c->chunk_fail_inject;
    c->chunk_fail_inject = value >= 0 ? (int)std::min<int64_t>(value, 1 << 20) : -1;
  } else if (n == "slam_chunked_fallbacks") { // reads the count of restore-and-chain passes; a value >= 0 sets it
    if (old_value) *old_value = c->chunk_fallbacks;
    if (value >= 0) c->chunk_fallbacks = value;
  } else if (n == "delayed_init_fused") { // a level.  0: ovgpu_slam_delayed_init_fused runs the chain's step (enqueue_init_feature) for every candidate; 1: the fused step, gated by k_system_t ahead of it (default); 2 (and above): the fused step behind k_init_rows, the gate read off the step's own factorisation in its tail; reads back the level
    if (old_value) *old_value = c->init_fused;
    if (value >= 0) c->init_fused = (int)std::min<int64_t>(value, 2);
  } else if (n == "delayed_init_fused_steps") { // reads the count of candidates that took the fused step; a value >= 0 sets it
    if (old_value) *old_value = c->init_fused_steps;
    if (value >= 0) c->init_fused_steps = value;
  } else if (n == "delayed_init_rows_steps") { // ... of those that took it at level 2 (k_init_rows in place of k_system_t)
    if (old_value) *old_value = c->init_rows_steps;
    if (value >= 0) c->init_rows_steps = value;
  } else if (n == "delayed_init_fused_long") { // 0 / 1.  1: under "delayed_init_fused" = 1 or 2 a candidate of ovgpu_slam_delayed_init_fused with 65 .. 232 measurements takes the fused step as well (k_init_rows' carve through with_max_lds; r = 2m - 3 > 256, m >= 130, factored by the two panels of k_chol_wide.h); default 0: such a candidate takes the chain's step; reads back 0 / 1
    if (old_value) *old_value = c->init_fused_long;
    if (value >= 0) c->init_fused_long = value != 0 ? 1 : 0;
  } else if (n == "delayed_init_long_steps") { // ... of those that took the fused step with more than 64 measurements ("delayed_init_fused_long" = 1)
    if (old_value) *old_value = c->init_long_steps;
    if (value >= 0) c->init_long_steps = value;
  } else if (n == "delayed_init_chain_steps") { // ... and of those ovgpu_slam_delayed_init_fused ran as the chain runs them
    if (old_value) *old_value = c->init_chain_steps;
    if (value >= 0) c->init_chain_steps = value;
  } else if (n == "gram_interleaved") {
    if (old_value) *old_value = c->gram_il ? 1 : 0;
    if (value >= 0) c->gram_il = value != 0;
  } else if (n == "layout_fpw") { // features per workgroup of k_batch_layout (8: 250 workgroups at 2000 features leave compute units to the prior's factorisation; 1: round 6's first form)
    if (old_value) *old_value = c->layout_fpw;
    if (value >= 1 && value <= 8) c->layout_fpw = (int)value;
  } else if (n == "unwhiten_blocked") { // 0: mode A's X = R L^-1 by k_unwhiten (one wavefront per 16 rows, substitution inside the tiles) instead of k_unwhiten_blk
    if (old_value) *old_value = c->unwhiten_blocked ? 1 : 0;
    if (value >= 0) c->unwhiten_blocked = value != 0;
  } else if (n == "pchol_blocked") { // 0: mode A's pivoted factor by the rank-one kernel of rounds 3-5 (k_gram_pchol) instead of k_gram_pchol_blk
    if (old_value) *old_value = c->pchol_blocked ? 1 : 0;
    if (value >= 0) c->pchol_blocked = value != 0;
  } else if (n == "speculative_prior") { // 0: the prior block's factorisation starts with the update, not with ovgpu_set_features
    if (old_value) *old_value = c->speculative_prior ? 1 : 0;
    if (value >= 0) c->speculative_prior = value != 0;
  } else if (n == "raw_stack") { // 0: the Gram route stacks the projected rows (rounds 2-5) instead of the unprojected ones in regions; takes effect with the next ovgpu_set_features
    if (old_value) *old_value = c->raw_enable ? 1 : 0;
    if (value >= 0) c->raw_enable = value != 0, c->raw_one_region = value == 2;
  } else if (n == "anchored_fast") { // 0: batches of an anchored feat_rep_msckf keep the general kernel (the routing before k_feat_rows_anchored); takes effect with the next ovgpu_set_features
    if (old_value) *old_value = c->anchored_fast ? 1 : 0;
    if (value >= 0) c->anchored_fast = value != 0;
  } else if (n == "slam_fused") { // a level.  1: SLAM batches of 3-dof landmarks take the fused per-feature kernel k_slam_y<false> on the whitened route (k_slam_y.h); 2: batches that observe a single-depth landmark take k_slam_y<true> as well; 3 (and above): batches whose longest track holds 63 .. 126 observations take the long shapes as well; default 0; reads back the level; takes effect with the next ovgpu_set_features
    if (old_value) *old_value = c->slam_fused;
    if (value >= 0) c->slam_fused = (int)std::min<int64_t>(value, 3);
  } else if (n == "slam_fused_big") { // a level.  1 (and above): under "slam_fused" = 3 a SLAM batch whose longest track holds 127 .. 232 observations takes the block-row shapes k_slam_y_big<false> / <true> (k_slam_y_big.h) on the long shape's terms; default 0; reads back the level; takes effect with the next ovgpu_set_features
    if (old_value) *old_value = c->slam_fused_big;
    if (value >= 0) c->slam_fused_big = (int)std::min<int64_t>(value, 1);
  } else if (n == "slam_fused_batches") { // reads the count of batch pipelines that took k_slam_y, once per update (the pipelines of a repeated attempt — Householder route, step-wise Cholesky — are not counted); a value >= 0 sets it
    if (old_value) *old_value = c->slam_fused_batches;
    if (value >= 0) c->slam_fused_batches = value;
  } else if (n == "gram_blocks_only") {
    if (old_value) *old_value = c->gram_blocks_only ? 1 : 0;
    if (value >= 0) c->gram_blocks_only = value != 0;
  } else if (n == "stage_timing_period") {
    if (old_value) *old_value = c->timing_period;
    if (value >= 1) c->timing_period = (int)value, c->timing_seq = 0;
  } else if (n == "fuse_chol_inputs") { // 0: k_tf_gather / k_tf_abh assemble the factorisations' work matrices (round 2's form)
    if (old_value) *old_value = c->fuse_chol_inputs ? 1 : 0;
    if (value >= 0) c->fuse_chol_inputs = value != 0;
  } else if (n == "featy_big") { // the multi-pass per-feature kernel on batches the one-pass kernels hold (tests)
    if (old_value) *old_value = c->featy_big;
    if (value >= 0) c->featy_big = (int)value;
  } else if (n == "upload_kernel") { // ovgpu_set_state / ovgpu_set_features: one scatter launch out of the page-locked arena (1, default) or one copy per array (0)
    if (old_value) *old_value = c->up.use_kernel;
    if (value >= 0) c->up.use_kernel = c->down.use_kernel = value != 0;
  } else if (n == "upload_arena_bytes") { // reads the arena's capacity; a value >= 64 is the size asked for at the next Uplink::begin (the arena only grows)
    if (old_value) *old_value = (int64_t)c->up.capacity();
    if (value >= 64) c->up.want = (size_t)std::min<int64_t>(value, (int64_t)1 << 30);
  } else if (n == "upload_bypasses") { // reads the count of uploads that did not fit the arena (host_link.h); a value >= 0 sets it
    if (old_value) *old_value = c->up.bypasses;
    if (value >= 0) c->up.bypasses = value;
  } else if (n == "layout_every_update") { // the per-batch integer tables rebuilt at the head of every update (api_state.inc: enqueue_batch_tables)
    if (old_value) *old_value = c->layout_every_update;
    if (value >= 0) c->layout_every_update = value != 0;
  } else if (n == "tri_waves") { // k_triangulate's workgroup size in wavefronts (api_context.inc)
    if (old_value) *old_value = c->tri_waves;
    if (value >= 0 && value <= 16) c->tri_waves = (int)value;
  } else if (n == "featy_skip") { // timing ablation of k_feat_y: 1 sweep, 2 V^T Y + output rows, 4 SYRK, 8 Cholesky (results are garbage)
#ifdef OVG_FEAT_ABLATE
    if (old_value) *old_value = c->featy_skip;
    if (value >= 0) c->featy_skip = (int)value;
#else
    return set_err(OVGPU_ERR_INVALID, "featy_skip: ablation switches exist in a developer build only (-DOVG_FEAT_ABLATE)");
#endif
  } else if (n == "gram_read_ahead") { // 0: k_gram_regions opens every k-step with its own operand reads (k_gram.h: gram_il_loop without PF) — same products in the same order, the same bits
    if (old_value) *old_value = c->gram_read_ahead ? 1 : 0;
    if (value >= 0) c->gram_read_ahead = value != 0;
  } else if (n == "gram_waves") { // 8 | 4: k_gram_regions with two wavefronts per SIMD or one (k_gram.h: gram_w8 | gram_il_loop) — every tile summed by one wavefront in the same order, the same bits
    if (old_value) *old_value = c->gram_waves;
    if (value >= 0) {
      if (value != 4 && value != 8) return set_err(OVGPU_ERR_INVALID, "gram_waves: 4 or 8");
      c->gram_waves = (int)value;
    }
  } else if (n == "featy_chains") { // 0: k_feat_y as it was before the run table and the requests ahead (k_featy.h: CH = false) — same products in the same order, the same bits
    if (old_value) *old_value = c->featy_chains ? 1 : 0;
    if (value >= 0) c->featy_chains = value != 0;
  } else if (n == "raw_work_const") {
    if (old_value) *old_value = c->raw_work_const;
    if (value >= 0) c->raw_work_const = (int)value;
  } else if (n == "last_stack_raw") { // read-only: the last pipeline's Gram matrix came from the unprojected stack (k_gram_regions)
    if (old_value) *old_value = c->last_stack_raw ? 1 : 0;
  } else if (n == "raw_gram_tile_rows") { // read-only: sum over the regions of rows x tiles of the region's triangle = 16 x 16 products per row that k_gram_regions executes for the resident batch
    int64_t t = 0;
    if (c->raw_tables_ok)
      for (int k = 0; k <= RAW_NEG; k++) t += c->raw_rows[k] * (int64_t)(c->raw_ntc[k] * (c->raw_ntc[k] + 1) / 2);
    if (old_value) *old_value = t;
  } else if (n == "stack_is_f32") { // read-only: the last pipeline stored the stack as floats and ran k_gram_f32 (options.gram_fp32)
    if (old_value) *old_value = c->stack_is_f32 ? 1 : 0;
  } else if (n == "last_feature_kernel") { // read-only: the per-feature kernel of the last batch pipeline, a FeatKernel (api_context.inc lists the codes)
    if (old_value) *old_value = c->last_feat_kernel;
  } else if (n == "feat_classes") { // a level.  1 (and above): an MSCKF batch laid out for the fast path runs a per-feature kernel per length class, each track on the smallest shape that holds it (plan_feature_stage, feat_classes.h); default 0: one kernel per batch, picked from its longest track; reads back the level; takes effect with the next ovgpu_set_features
    if (old_value) *old_value = c->feat_classes;
    if (value >= 0) c->feat_classes = (int)std::min<int64_t>(value, 1);
  } else if (n == "feat_class_batches") { // reads the count of batch pipelines that launched more than one length class, once per update (the pipelines of a repeated attempt — Householder route, step-wise Cholesky — are not counted); a value >= 0 sets it
    if (old_value) *old_value = c->feat_class_batches;
    if (value >= 0) c->feat_class_batches = value;
  } else if (n == "last_feature_classes") { // read-only: bit mask over the FeatKernel codes 0 .. 3 of the kernels the last batch pipeline launched; a single bit whenever one kernel took the batch
    if (old_value) *old_value = c->last_feat_classes;
  } else if (n.size() == 21 && n.compare(0, 20, "last_class_features_") == 0 && n[20] >= '0' && n[20] <= '3') { // read-only, "last_class_features_0" .. "_3": features of the last batch pipeline in the class of that FeatKernel code
    if (old_value) *old_value = c->last_class_features[n[20] - '0'];
  } else if (n == "last_gram_kernel") { // read-only, this and the two below: what the last batch pipeline launched (api_context.inc lists the codes)
    if (old_value) *old_value = c->last_gram_kernel;
  } else if (n == "last_gram_workgroups") { // read-only: gridDim.x of the last pipeline's k_gram_f32 or k_gram_blk launch (the row shares), 0 otherwise
    if (old_value) *old_value = c->last_gram_workgroups;
  } else if (n == "last_factor_kernel") {
    if (old_value) *old_value = c->last_factor_kernel;
  } else if (n == "last_unwhiten_kernel") {
    if (old_value) *old_value = c->last_unwhiten_kernel;
  } else if (n == "chol_wide") { // 0: beyond 256 columns the Cholesky-with-carry runs as one launch of k_ekf_chol_step per 16 rows instead of two panels of k_chol_fused (k_chol_wide.h)
    if (old_value) *old_value = c->chol_wide ? 1 : 0;
    if (value >= 0) c->chol_wide = value != 0;
  } else if (n == "chol_wide_factorisations") { // reads the count of factorisations enqueued on the two-panel path; a value >= 0 sets it
    if (old_value) *old_value = c->chol_wide_count;
    if (value >= 0) c->chol_wide_count = value;
  } else if (n == "gram_wide") { // a level.  1: a float64 context on OVGPU_COMPRESS_GRAM takes the whitened Gram route of mode B at 384 .. 511 Jacobian columns as well (k_gram_blk over four column windows, the fused per-feature kernels on the terms they have below 384); default 0: such updates take the Householder route; reads back the level; takes effect with the next ovgpu_set_state / ovgpu_set_features
    if (old_value) *old_value = c->gram_wide;
    if (value >= 0) c->gram_wide = (int)std::min<int64_t>(value, 1);
  } else if (n == "gram_wide_updates") { // read-only: the count of updates that took the Gram route beyond 383 columns, once per update (a repeated attempt — Householder route, step-wise Cholesky — is not counted)
    if (old_value) *old_value = c->gram_wide_updates;
  } else if (n == "mode_a_wide") { // a level.  1: ovgpu_msckf_compress on a float64 context with the whitened stack takes the pivoted Gram route at 384 .. 511 Jacobian columns as well (k_gram_blk over four column windows, k_pchol_wide.h, k_unwhiten_blk<32>); default 0: such compressions take the Householder route; independent of "gram_wide"; reads back the level; takes effect with the next ovgpu_set_state / ovgpu_set_features
    if (old_value) *old_value = c->mode_a_wide;
    if (value >= 0) c->mode_a_wide = (int)std::min<int64_t>(value, 1);
  } else if (n == "mode_a_wide_compressions") { // read-only: the count of compressions that took the pivoted route beyond 383 columns and stand (an attempt repeated through the Householder route is not counted)
    if (old_value) *old_value = c->mode_a_wide_compressions;
  } else if (n == "mode_a_panel") { // a level.  1 (and above): on mode A's pivoted Gram route (ovgpu_msckf_compress; ovgpu_slam_compress under "slam_mode_a") 17 .. 24 tile columns of [H | r] (256 .. 383 Jacobian columns) are factored by k_pchol_panel / k_pchol_schur (k_pchol_wide.h, 32 pivots per launch) instead of the rank-one k_gram_pchol<9 .. 12>, and ovgpu_msckf_compress un-whitens 257 .. 383 columns with k_unwhiten_blk<24>; default 0: the rank-one kernel and k_unwhiten<24>; reads back the level; takes effect with the next ovgpu_set_state / ovgpu_set_features
    if (old_value) *old_value = c->mode_a_panel;
    if (value >= 0) c->mode_a_panel = (int)std::min<int64_t>(value, 1);
  } else if (n == "mode_a_panel_compressions") { // read-only: the count of compressions that took the panelled factor at 256 .. 383 columns and stand (an attempt repeated through the Householder route is not counted)
    if (old_value) *old_value = c->mode_a_panel_compressions;
  } else if (n == "slam_mode_a") { // a level.  1 (and above): ovgpu_slam_compress takes the pivoted Gram route on the terms ovgpu_msckf_compress does (a float64 context on OVGPU_COMPRESS_GRAM, the whitened stack, D <= 383, or 511 with "mode_a_wide" = 1 as well), its per-feature stage the kernel "slam_fused" lays the batch out for, its un-whitening at D = 257 .. 383 k_unwhiten_blk<24>; default 0: the Householder triangle; reads back the level; takes effect with the next ovgpu_set_state / ovgpu_set_features
    if (old_value) *old_value = c->slam_mode_a;
    if (value >= 0) c->slam_mode_a = (int)std::min<int64_t>(value, 1);
  } else if (n == "slam_mode_a_compressions") { // read-only: the count of SLAM compressions that took the pivoted route and stand (an attempt repeated through the Householder route is not counted)
    if (old_value) *old_value = c->slam_mode_a_compressions;
  } else if (n == "tsqr_leaves") { // read-only, this and the four below: what the last Householder compression launched (enqueue_compress / enqueue_merge_tree)
    if (old_value) *old_value = c->tsqr_last_W;
  } else if (n == "tsqr_rows_per_node") {
    if (old_value) *old_value = c->tsqr_last_rpn;
  } else if (n == "tsqr_last_leaf_kernel") { // 0 pw::k_qr_node, 1 k_qr_node<.., false>, 2 k_qr_append; -1: no compression yet
    if (old_value) *old_value = c->tsqr_last_leaf;
  } else if (n == "tsqr_last_tree") { // 0 no merge, 1 k_qr_tree next to the leaves, 2 k_qr_tree behind them, 3 one launch per level
    if (old_value) *old_value = c->tsqr_last_tree;
  } else if (n == "tsqr_last_qh") { // 16 / 28 / 32: quads per register array of the merge kernels; 0: k_qr_append, or no merge
    if (old_value) *old_value = c->tsqr_last_qh;
  } else if (n == "sys_lds_limit") { // read-only, this and the four below: the general per-feature kernel's LDS carve for the batch in force (FeatPlan, plan_feature_stage in api_state.inc) — the byte limit it was carved under
    if (old_value) *old_value = c->lds_limit;
  } else if (n == "sys_m_lds_max") { // the largest track length whose gate matrix is LDS-resident; longer tracks of the batch keep theirs in the per-workgroup global workspace
    if (old_value) *old_value = c->plan.m_lds_max;
  } else if (n == "sys_rows_global") { // 1: the Jacobian records live in a global workspace (k_system_t<true>), 0: in LDS
    if (old_value) *old_value = c->plan.rows_global ? 1 : 0;
  } else if (n == "sys_row_stride") { // doubles per Jacobian record: 48, or 72 once an anchored representation is in force
    if (old_value) *old_value = c->row_stride;
  } else if (n == "sys_lds_bytes") { // the dynamic LDS size of the kernel's launch
    if (old_value) *old_value = (int64_t)c->plan.sys_lds;
  } else if (n == "live_allocations") { // read-only, this and the one below: what the library's buffers (OwnedBuf) hold in this PROCESS, device and page-locked memory together, whatever the context asked
    if (old_value) *old_value = DeviceAlloc::live.n.load() + PinnedAlloc::live.n.load();
  } else if (n == "live_allocation_bytes") { // ... in bytes as requested: max(n, 1) elements each
    if (old_value) *old_value = DeviceAlloc::live.bytes.load() + PinnedAlloc::live.bytes.load();
  } else if (n == "chol_timeouts") { // read-only counter: updates repeated with the step-wise Cholesky after a follower timed out
    if (old_value) *old_value = c->chol_timeouts;
  } else {
    return set_err(OVGPU_ERR_INVALID, "unknown debug option");
  }
  return OVGPU_OK;
}

// Developer aid: enable != 0 allocates and clears 512 cycle counters that workgroup 0 of the per-feature kernel accumulates
// (k_feat: slots 200..210 = its phases); out512 != NULL reads them back.
int ovgpu_debug_cycles(ovgpu_ctx *c, int enable, long long *out512) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(upload_sync(c, c->stream));
  if (out512 && c->dbg_cycles.p) HIPCHK(hipMemcpy(out512, c->dbg_cycles.p, 512 * sizeof(long long), hipMemcpyDeviceToHost));
  if (enable) {
    HIPCHK(c->dbg_cycles.reserve(512));
    HIPCHK(hipMemset(c->dbg_cycles.p, 0, 512 * sizeof(long long)));
  } else if (!out512) {
    c->dbg_cycles.release();
  }
  return OVGPU_OK;
}

#ifdef OVG_GRAM_PROF
// developer build (-DOVG_GRAM_PROF): the phase counters of the last k_gram_regions launch, eight values per wavefront, room for eight wavefronts per workgroup (k_gram.h; the four-wavefront form leaves the last four as they were);
// *launched = the workgroups of that launch (entries past it are an earlier launch's)
extern "C" int ovgpu_debug_gram_phases(ovgpu_ctx *c, long long *out, int workgroups, int *launched) {
  if (!c || !out || !launched || workgroups < 0 || workgroups > 1024) return set_err(OVGPU_ERR_INVALID, "bad argument");
  *launched = c->gram_wg_n;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(upload_sync(c, c->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(gram::gram_prof_buf), sizeof(long long) * 64 * workgroups));
  return OVGPU_OK;
}
#endif

// one wavefront, a dependent chain of integer multiply-adds for ~0.3 ms (20 000 steps): shader cycles against the constant reference counter
__global__ void k_clock_probe(long long *out, int iters) {
  const long long c0 = clock64(), w0 = wall_clock64();
  unsigned x = threadIdx.x + 1;
  for (int i = 0; i < iters; i++) x = x * 1664525u + 1013904223u;
  const long long c1 = clock64(), w1 = wall_clock64();
  if (threadIdx.x == 0) out[0] = c1 - c0, out[1] = w1 - w0, out[2] = (long long)x;
}
// the same ratio with every SIMD of the chip busy on the FP64 matrix pipe (four wavefronts per SIMD, four independent accumulator
// chains each): the clock the power limit leaves under the load this pipeline's big kernels put on the chip
__global__ void __launch_bounds__(256) k_clock_probe_load(long long *out, int iters) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
  const double x = 1.0 + 1e-9 * threadIdx.x, y = 1.0 - 1e-9 * threadIdx.x;
  const long long c0 = clock64(), w0 = wall_clock64();
  for (int i = 0; i < iters; i++) {
    a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, x, a1, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, a2, 0, 0, 0);
    a3 = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, a3, 0, 0, 0);
  }
  const long long c1 = clock64(), w1 = wall_clock64();
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = c1 - c0, out[1] = w1 - w0;
  if (a0[0] + a1[1] + a2[2] + a3[3] == 12345.678) out[2] = 1; // (keeps the products alive)
}
__global__ void k_probe_empty(int *sink) {
  if (sink == nullptr && threadIdx.x == 12345) *sink = 0;
}
// a cycle through n slots of `stride` ints each (slot i points to slot (i + step) % n, step odd and n a power of two: one cycle
// through all slots): lane 0 chases `hops` dependent loads
__global__ void k_chase_init(int32_t *buf, int n, int stride, int step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) buf[(size_t)i * stride] = (int32_t)(((long long)i + step) % n);
}
__global__ void k_chase(const int32_t *buf, int stride, int hops, long long *out) {
  if (threadIdx.x != 0) return;
  int i = 0;
  for (int h = 0; h < 64; h++) i = __builtin_nontemporal_load(buf + (size_t)i * stride); // (warm the TLB / page tables a little)
  const long long w0 = wall_clock64();
  for (int h = 0; h < hops; h++) i = __builtin_nontemporal_load(buf + (size_t)i * stride);
  const long long w1 = wall_clock64();
  out[0] = w1 - w0, out[1] = i;
}
int ovgpu_debug_box_probe(ovgpu_ctx *c, double *out3) { // (out3: six values, see include/ovgpu.h)
  if (!c || !out3) return set_err(OVGPU_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  long long h[3] = {0, 0, 0};
  DevBuf<long long> d_buf;
  HIPCHK(d_buf.reserve(3));
  long long *d = d_buf.p;
  for (int rep = 0; rep < 2; rep++) { // (the first launch wakes the clocks up)
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, d, 20000);
    HIPCHK(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
  }
  out3[0] = h[1] > 0 ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
  { // ... and under load: 4 workgroups of 4 wavefronts per compute unit, ~2 ms of matrix instructions
    hipLaunchKernelGGL(k_clock_probe_load, dim3(c->num_cu * 4), dim3(256), 0, s, d, 2500);
    hipLaunchKernelGGL(k_clock_probe_load, dim3(c->num_cu * 4), dim3(256), 0, s, d, 2500);
    HIPCHK(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
    out3[3] = h[1] > 0 ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
  }
  const struct { size_t bytes; int stride; } probes[2] = {{(size_t)1 << 20, 32}, {(size_t)256 << 20, 1024}}; // 128-byte slots in 1 MB; 4 KB slots in 256 MB
  for (int k = 0; k < 2; k++) {
    DevBuf<int32_t> chase;
    if (chase.reserve(probes[k].bytes / sizeof(int32_t)) != hipSuccess) {
      out3[1 + k] = 0.0;
      continue;
    }
    int32_t *buf = chase.p;
    const int n = (int)(probes[k].bytes / (sizeof(int32_t) * probes[k].stride)), hops = 2000;
    hipLaunchKernelGGL(k_chase_init, dim3((n + 255) / 256), dim3(256), 0, s, buf, n, probes[k].stride, k == 0 ? 2731 : 24571);
    hipLaunchKernelGGL(k_chase, dim3(1), dim3(64), 0, s, (const int32_t *)buf, probes[k].stride, hops, d);
    HIPCHK(hipMemcpyAsync(h, d, 2 * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(upload_sync(c, s));
    out3[1 + k] = 10.0 * (double)h[0] / hops; // the reference counter ticks at 100 MHz
  }
  { // the command processor: 200 dependent empty launches on one stream (us per launch), one launch of 65 536 empty workgroups (ns per workgroup)
    Event e0, e1;
    HIPCHK(e0.create());
    HIPCHK(e1.create());
    float ms = 0.f;
    for (int i = 0; i < 20; i++) hipLaunchKernelGGL(k_probe_empty, dim3(1), dim3(64), 0, s, (int *)nullptr);
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < 200; i++) hipLaunchKernelGGL(k_probe_empty, dim3(1), dim3(64), 0, s, (int *)nullptr);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    out3[4] = 1e3 * ms / 200.0;
    HIPCHK(hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_probe_empty, dim3(65536), dim3(64), 0, s, (int *)nullptr);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    out3[5] = 1e6 * ms / 65536.0;
  }
  return OVGPU_OK;
}

int ovgpu_last_update_route(ovgpu_ctx *c) { return c ? c->last_route : -1; }

uint64_t ovgpu_stream(ovgpu_ctx *c) { return c ? (uint64_t)(uintptr_t)c->stream.h : 0; }

#ifdef QR_PROFILE
int ovgpu_debug_tree_times(long long *out1024) {
  return hipMemcpy(out1024, tree_dbg_buffer(), 1024 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? OVGPU_OK : OVGPU_ERR_HIP;
}
int ovgpu_debug_qr_cycles(long long *out128) {
  return hipMemcpy(out128, qr_dbg_buffer(), 128 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? OVGPU_OK : OVGPU_ERR_HIP;
}
#endif

int ovgpu_system_time(ovgpu_ctx *c, double *ms_system_avg, int64_t *n_launches) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(upload_sync(c, c->stream));
  double ss = 0;
  int64_t n = 0;
  for (size_t i = 0; i < c->ev_used && i < c->ev_system.size(); i++) {
    float a = 0.f;
    if (hipEventElapsedTime(&a, c->ev_system[i].a, c->ev_system[i].b) != hipSuccess) continue;
    ss += a, n++;
  }
  if (ms_system_avg) *ms_system_avg = n ? ss / n : 0.0;
  if (n_launches) *n_launches = n;
  return OVGPU_OK;
}

int ovgpu_kernel_times(ovgpu_ctx *c, int reset, double *ms_compress_avg, double *ms_update_avg, int64_t *n_launches) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(upload_sync(c, c->stream));
  double sc = 0, su = 0;
  int64_t n = 0;
  for (size_t i = 0; i < c->ev_used; i++) {
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, c->ev_compress[i].a, c->ev_compress[i].b) != hipSuccess) continue;
    if (hipEventElapsedTime(&b, c->ev_update[i].a, c->ev_update[i].b) != hipSuccess) continue;
    sc += a, su += b, n++;
  }
  if (ms_compress_avg) *ms_compress_avg = n ? sc / n : 0.0;
  if (ms_update_avg) *ms_update_avg = n ? su / n : 0.0;
  if (n_launches) *n_launches = n;
  if (reset) c->ev_used = 0;
  return OVGPU_OK;
}
