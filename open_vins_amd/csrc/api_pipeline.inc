// api_pipeline.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): the stages of an update (triangulate, per-feature system, compression, EKF) and UpdaterMSCKF's entry points: ovgpu_triangulate / refine, ovgpu_msckf_update / compress, ovgpu_get_state.
// ---------------------------------------------------------------------------
// pipeline stages (all asynchronous on ctx->stream)
// ---------------------------------------------------------------------------
static int enqueue_triangulate(ovgpu_ctx *c, const double *seed_pA = nullptr, const int32_t *seed_anchor = nullptr) {
  const Batch b = batch_of(c);
  if (b.F == 0) return OVGPU_OK;
  TriParams p;
  p.seed_pA = seed_pA, p.seed_anchor = seed_anchor, p.anchor_pre = c->anchor_pre.p;
  p.F = b.F, p.C = c->C, p.K = c->K;
  p.meas_offsets = b.meas_offsets, p.meas_cc = b.meas_cc, p.uvn = b.uvn, p.tab_cc = c->tab_cc.p;
  p.p_FinA = b.pA, p.p_FinG = b.pG, p.anchor_meas = c->anchor.p, p.status = b.status;
  p.opt = c->dopt;
  const size_t lds = (size_t)c->K * c->C * 12 * sizeof(double);
  if (lds > (size_t)c->lds_limit) { // the kernel stages the whole pose table in LDS: refused here, before anything is launched (OVG_MAX_CLONES x OVG_MAX_CAMS would be 6 MB)
    return set_err(OVGPU_ERR_CAPACITY, "k_triangulate: the pose table of K = " + std::to_string(c->K) + " cameras x C = " + std::to_string(c->C) + " clones (96 bytes a pair, " +
                                           std::to_string(lds) + " bytes) exceeds the LDS limit of " + std::to_string(c->lds_limit) + " bytes");
  }
  // Features (wavefronts) per workgroup.  The prior block's factorisation is dispatched a few microseconds BEHIND this kernel and needs whole
  // compute units (k_chol_fused: 16 wavefronts x 128 registers, 90 KB of LDS per block): with four features per workgroup every CU holds a
  // piece of this kernel and the factorisation only becomes resident when the first CUs drain, ~30 us later.  Where the batch allows it the
  // workgroups are made large enough to leave six CUs untouched (2000 features: 250 workgroups of 8) — provided that still uses three
  // quarters of the chip (measured at 2000 features: 8 -> -1 %; 16 = 125 workgroups: the kernel itself 45 -> 80 us).
  int wpb = c->tri_waves;
  if (wpb == 0) {
    wpb = 4;
    const int room = c->num_cu - 6;
    for (int w = 4; w <= 8 && room > 0; w *= 2) {
      const int blocks = (b.F + w - 1) / w;
      if (blocks <= room) {
        if (4 * blocks >= 3 * room) wpb = w;
        break;
      }
    }
  }
  hipLaunchKernelGGL(with_max_lds<k_triangulate>(c), dim3((b.F + wpb - 1) / wpb), dim3(64 * wpb), lds, c->stream, p);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// ---- the per-feature stage: the kernel is picked once (select_feat_kernel) and launched in one place (launch_feat_kernel)
struct FeatLaunch {
  FeatKernel kernel = FK_GENERAL; // the kernel that runs
  FeatKernel code = FK_GENERAL;   // ... and what "last_feature_kernel" reports: the kernel the batch was laid out for ("featy_big" runs
                                  // k_feat_y_big on a batch laid out for a one-pass shape, which keeps that shape's code)
  bool f32 = false; // the stack leaves as floats (options.gram_fp32): k_feat_y<.., F32 = true>, k_feat_y_big<8, 17, true>
  bool ch = false;  // k_feat_y<.., CH = true>: the run table, the next slot requested a feature ahead ("featy_chains")
  bool alt = false; // the kernel's other shape: k_feat_y_big<8, 5> ("featy_big" = 2), k_system_t<true> (Jacobian records in global memory)
  int cb = 0;       // columns per block of the fused MSCKF kernels' sweep; 0: another kernel
  int nt = 0, nta = 0; // the fused MSCKF kernels' LDS carve: tile rows of the longest track the launch walks, and of its gate matrix ...
  int ist = 0;         // ... against the tile rows per feature of the batch's instance lists, which a length class does not shorten
  const int32_t *inst = nullptr; // the lists at `cb` columns
  int slot0 = 0;       // the first slot record of the launch (a length class: its range's; the kernels walk p.F records from there)
  size_t lds = 0;   // dynamic LDS bytes, by the kernel header's own layout function
  int grid = 1;
  int err = OVGPU_OK;
  const char *msg = nullptr;
};
// one row of launch_feat_kernel's switch per instantiation
static constexpr int feat_key(FeatKernel k, bool f32 = false, bool ch = false, bool alt = false) { return 8 * k + (f32 ? 1 : 0) + (ch ? 2 : 0) + (alt ? 4 : 0); }

// The kernel of this launch: from the plan of the batch in force (F features), what p asks for — L (the whitened route; never with f_one >= 0),
// SLAM rows, per-feature sigma / multiplier —, f_one, and the launch-time switches "featy_big", "featy_chains", options.gram_fp32 and lm_fast_on.
// k: the launch of ONE length class of the plan ("feat_classes"; enqueue_system has decided that the pipeline runs by classes), m_first the track
// length at the class's first slot in the batch in force — the class's kernel, carve and grid as planned, held against that track.
static FeatLaunch select_feat_kernel(const ovgpu_ctx *c, const SysParams &p, int F, int f_one, const FeatPlan::Class *k = nullptr, int m_first = 0) {
  const FeatPlan &pl = c->plan;
  const size_t limit = (size_t)c->lds_limit;
  FeatLaunch s;
  size_t need; // what the batch in force takes of the kernel's LDS, against s.lds: what the batch was laid out for
  if (k) {
    s.code = s.kernel = k->kernel, s.lds = k->lds, s.grid = k->grid;
    s.err = OVGPU_ERR_INVALID, s.msg = "internal: a length class of the per-feature stage does not hold the tracks of its slot range";
    if (k->kernel == FK_GENERAL) {
      s.alt = pl.rows_global;
      need = m_first <= p.m_max ? pl.sys_lds : limit + 1;
    } else {
      const int nt = featcls::tile_rows(m_first), nta = featcls::gate_tile_rows(m_first);
      s.cb = k->kernel == FK_FEATY_BIG ? 32 : feat::FY_CB, s.nt = k->nt, s.nta = k->nta, s.ist = pl.nt, s.slot0 = k->begin;
      s.inst = s.cb == feat::FY_CB && pl.cls_mixed_width() ? c->fs_inst64.p : c->fs_inst.p;
      s.f32 = c->want_stack_f32, s.ch = !s.f32 && c->featy_chains && k->kernel != FK_FEATY_BIG;
      // the carve is the class's, the lists' stride the batch's: a track of the range that needs more tile rows than either would leave its LDS block
      if (featcls::kernel_of_length(std::max(m_first, 2)) != (int)k->kernel || nt > k->nt || nta > k->nta || k->nt > pl.nt) need = limit + 1;
      else need = k->kernel == FK_FEATY_BIG ? feat::featyb_lds_layout(nt, 8).total : feat::featy_lds_layout(nt, nta, k->kernel == FK_FEATY_4 ? 4 : 8, s.cb).total;
    }
    if (need <= s.lds && s.lds <= limit) s.err = OVGPU_OK, s.msg = nullptr;
    return s;
  }
  // the MSCKF fast path: whitened output, one noise level (k_feat.h); a global representation, or an anchored one on its own record kernel
  // (with landmarks resident — the empty active set, set_row_layout — only for ovgpu_msckf_update_lm: every other entry keeps the general kernel)
  // (a plan by length classes that holds a general class — enqueue_system runs it as ONE kernel when a launch-time switch rules the classes out —
  //  is the general kernel's then, as the single-kernel rule has a batch whose longest track no fused kernel holds)
  if (p.Lw && pl.msckf != FK_GENERAL && !pl.cls_general() && (c->L == 0 || (c->lm_fast_on && pl.lm_fast_ok)) && !p.slam && !p.feat_sigma && !p.feat_chi2mult) {
    s.code = pl.msckf, s.kernel = featy_block_rows(c) ? FK_FEATY_BIG : pl.msckf, s.cb = featy_block_cols(c);
    s.nt = pl.nt, s.nta = pl.nta, s.ist = pl.nt, s.inst = c->fs_inst.p;
    if (s.kernel == FK_FEATY_BIG) { // block row by block row (k_featy_big.h), one workgroup per CU; <8, 5> has no float32 twin
      s.alt = c->featy_big == 2, s.f32 = c->want_stack_f32 && !s.alt;
      s.lds = feat::featyb_lds_layout(pl.nt, 8).total;
      s.grid = fused_feat_grid(c, FK_FEATY_BIG, s.lds, F);
      s.err = OVGPU_ERR_CAPACITY, s.msg = "k_feat_y_big: track too long for its LDS block";
    } else { // as many workgroups per CU as its registers (<4, 9, 2>: two; <8, 17, 1>: one) and its LDS block allow, the features dealt round-robin over them
      s.f32 = c->want_stack_f32, s.ch = !s.f32 && c->featy_chains;
      s.lds = feat::featy_lds_layout(pl.nt, pl.nta, pl.nw(), s.cb).total;
      s.grid = fused_feat_grid(c, s.kernel, s.lds, F);
      s.err = OVGPU_ERR_INVALID, s.msg = "internal: the MSCKF fast path was selected for a batch the fused kernel does not hold";
    }
    need = s.lds;
  } else if (p.slam && p.Lw && pl.slam != FK_GENERAL) {
    // UpdaterSLAM::update on the whitened route, a batch laid out for it under ovgpu_debug_option "slam_fused": the fused kernel (k_slam_y.h).
    // Everything else — the Householder repeat and the other routes without L, the delayed initialisation, a batch it does not hold — keeps k_system_t.
    const bool lng = pl.slam >= FK_SLAMY_LONG, proj = pl.slam == FK_SLAMY_PROJ || pl.slam == FK_SLAMY_LONG_PROJ;
    s.code = s.kernel = pl.slam;
    if (pl.slam >= FK_SLAMY_BIG) { // block row by block row (k_slam_y_big.h): the carve of the tile rows the batch was laid out for
      const int nt = (2 * p.m_max + 15) / 16;
      need = nt <= pl.slam_nt ? slamy::slamyb_lds_layout(pl.slam_nt, pl.slam == FK_SLAMY_BIG_PROJ).total : limit + 1;
    } else need = slamy::slamy_lds_layout(p.m_max, proj, lng ? slamy::SLY_CB_L : slamy::SLY_CB).total;
    s.lds = pl.slam_lds;
    s.grid = std::max(1, std::min(F, c->num_cu));
    s.err = OVGPU_ERR_INVALID, s.msg = "internal: k_slam_y was selected for a batch it does not hold";
  } else {
    s.alt = pl.rows_global, s.lds = need = pl.sys_lds, s.grid = f_one >= 0 ? 1 : pl.sys_grid;
  }
  if (need <= s.lds && s.lds <= limit) s.err = OVGPU_OK, s.msg = nullptr; // (else: the batch in force is not the one the plan was made for)
  return s;
}

// The one launch of the per-feature stage: a row per instantiation
static int launch_feat_kernel(ovgpu_ctx *c, const FeatLaunch &s, const SysParams &p) {
  const dim3 grid(s.grid), slam_block(64 * slamy::SLY_NW);
  const int nt = s.nt, nta = s.nta, ist = s.ist;
  const double *sr = c->fs_rows.p, *sV = c->fs_V.p, *stq = c->fs_tq.p;
  const int32_t *sm = c->fs_minfo.p, *sin = s.inst, *ssl = c->fs_slots.p + (size_t)8 * s.slot0, *runs = c->raw_runs.p;
  double *bws = c->featyb_ws.p;
  switch (feat_key(s.kernel, s.f32, s.ch, s.alt)) {
    case feat_key(FK_GENERAL): hipLaunchKernelGGL(with_max_lds<k_system_t<false>>(c), grid, dim3(SYS_NT), s.lds, c->stream, p); break;
    case feat_key(FK_GENERAL, false, false, true): hipLaunchKernelGGL(with_max_lds<k_system_t<true>>(c), grid, dim3(SYS_NT), s.lds, c->stream, p); break;
#define X(NW, TPW, OCC, F32, CB, CH) case feat_key(NW == 4 ? FK_FEATY_4 : FK_FEATY_8, F32, CH): hipLaunchKernelGGL((with_max_lds<feat::k_feat_y<NW, TPW, OCC, F32, CB, CH>>(c)), grid, dim3(64 * NW), s.lds, c->stream, p, nt, nta, sr, sm, sV, stq, sin, ssl, runs, ist); break;
    OVG_FEATY_SHAPES(X)
#undef X
    case feat_key(FK_FEATY_BIG): hipLaunchKernelGGL((with_max_lds<feat::k_feat_y_big<8, 17>>(c)), grid, dim3(512), s.lds, c->stream, p, nt, sr, sm, sV, stq, sin, ssl, bws, ist); break;
    case feat_key(FK_FEATY_BIG, true): hipLaunchKernelGGL((with_max_lds<feat::k_feat_y_big<8, 17, true>>(c)), grid, dim3(512), s.lds, c->stream, p, nt, sr, sm, sV, stq, sin, ssl, bws, ist); break;
    case feat_key(FK_FEATY_BIG, false, false, true): hipLaunchKernelGGL((with_max_lds<feat::k_feat_y_big<8, 5>>(c)), grid, dim3(512), s.lds, c->stream, p, nt, sr, sm, sV, stq, sin, ssl, bws, ist); break;
    case feat_key(FK_SLAMY): hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y<false>>(c)), grid, slam_block, s.lds, c->stream, p); break;
    case feat_key(FK_SLAMY_PROJ): hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y<true>>(c)), grid, slam_block, s.lds, c->stream, p); break;
    case feat_key(FK_SLAMY_LONG): hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y<false, slamy::SLY_TPW_L, slamy::SLY_CB_L, slamy::SLY_MMAX_L>>(c)), grid, slam_block, s.lds, c->stream, p); break;
    case feat_key(FK_SLAMY_LONG_PROJ): hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y<true, slamy::SLY_TPW_L, slamy::SLY_CB_L, slamy::SLY_MMAX_L>>(c)), grid, slam_block, s.lds, c->stream, p); break;
    case feat_key(FK_SLAMY_BIG):
    case feat_key(FK_SLAMY_BIG_PROJ): { // the records kernel in front on the same stream, a workgroup per feature slot of the launch's range
      const slamy::SlamYBigStore st{c->slyb_rows.p, c->slyb_minfo.p, c->slyb_V.p, c->slyb_hq.p, c->slyb_inst.p};
      const dim3 rgrid(std::max(1, p.f_end - p.f_begin));
      const size_t rlds = slamy::slamyb_rows_lds(p.m_max);
      const int snt = c->plan.slam_nt;
      if (s.kernel == FK_SLAMY_BIG) {
        hipLaunchKernelGGL(slamy::k_slam_rows_big<false>, rgrid, dim3(256), rlds, c->stream, p, st);
        hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y_big<false>>(c)), grid, slam_block, s.lds, c->stream, p, snt, st, bws);
      } else {
        hipLaunchKernelGGL(slamy::k_slam_rows_big<true>, rgrid, dim3(256), rlds, c->stream, p, st);
        hipLaunchKernelGGL((with_max_lds<slamy::k_slam_y_big<true>>(c)), grid, slam_block, s.lds, c->stream, p, snt, st, bws);
      }
      break;
    }
    default: return set_err(OVGPU_ERR_INVALID, "internal: the per-feature stage has no kernel in the shape selected");
  }
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// The per-feature stage's parameters from the context and the batch in force, for a launch over the whole batch on the unwhitened route
// (enqueue_system and k_init_rows' launch, api_slam.inc, start from these)
static void fill_sys_params(ovgpu_ctx *c, const Batch &b, SysParams &p) {
  p.F = b.F, p.C = c->C, p.K = c->K, p.D = c->D, p.LD = c->LD, p.N = c->N;
  p.meas_offsets = b.meas_offsets, p.meas_cc = b.meas_cc, p.uv = b.uv;
  p.tab_clone = c->tab_clone.p, p.tab_cam = c->tab_cam.p, p.intr = c->intr.p, p.fisheye = c->fisheye.p;
  p.clone_col = c->clone_col.p, p.calib_col = c->calib_col.p, p.intr_col = c->intr_col.p;
  p.col_cov = c->col_cov.p, p.col_kind = c->col_kind.p, p.col_var = c->col_var.p, p.col_sub = c->col_sub.p;
  p.P = c->P.p, p.p_FinG = b.pG, p.p_FinA = b.pA, p.anchor_meas = c->anchor.p;
  p.status = b.status, p.chi2 = b.chi2, p.chi2_thresh = b.chi2_thr;
  p.chi2_table = c->chi2_table.p, p.chi2_table_len = c->chi2_table_len;
  p.row_off = b.row_off, p.Hbig = c->Hbig.p, p.ws = c->gate_ws.p, p.ws_stride = c->plan.gate_ws_stride;
  p.Hbig32 = nullptr, p.LDF = 0;
  p.m_lds_max = c->plan.m_lds_max, p.m_max = std::max(b.m_max, 1), p.row_stride = c->row_stride;
  p.opt = c->dopt;
  p.dbg = c->dbg_cycles.p ? c->dbg_cycles.p : qr_dbg_buffer();
  p.slam = c->slam_rows ? 1 : 0;
  p.p_fej = c->pFej.p, p.feat_lm = c->feat_lm.p, p.feat_lmcol = c->feat_lmcol.p, p.feat_lmcov = c->feat_lmcov.p, p.feat_anchor = c->feat_anchor.p;
  p.lm_size = 3, p.init_dof_less = 0, p.lm_rep = nullptr;
  p.feat_sigma = b.have_sigma ? b.feat_sigma : nullptr, p.feat_chi2mult = b.have_mult ? b.feat_mult : nullptr;
  if (p.slam) { // the landmarks' representation, not the MSCKF features'; single depth = MSCKF inverse depth Jacobians (UpdaterSLAM.cpp:338-341)
    p.lm_rep = c->lm_repd.p; // per landmark: k_system reads the representation and the size from the landmark each feature observes
  }
  p.f_begin = 0, p.f_end = b.F, p.init = 0, p.init_out = nullptr, p.init_flag = nullptr, p.init_keep = 0, p.order = b.sys_order;
  p.rows_used = c->rows_used.p;
  p.Lw = nullptr;
  p.skip = c->featy_skip;
  // The Gram route's stack as unprojected rows in regions by column reach (ovgpu_types.h: RawStack; the whitened stack only ever feeds the Gram kernels):
  // the one-pass fused kernels on a batch laid out by ovgpu_set_features, float64 stack.  enqueue_system decides, once the kernel shape is known.
  p.raw.on = 0;
}

// ... narrowed to feature f_one in StateHelper::initialize mode with the landmark representation init_rep
static void sys_params_init_mode(ovgpu_ctx *c, SysParams &p, int f_one, int init_rep) {
  p.order = nullptr;
  p.rows_used = nullptr;
  p.f_begin = f_one, p.f_end = f_one + 1, p.init = 1, p.init_out = c->init_ws.p, p.init_flag = c->init_ctr.p + 2;
  p.init_keep = c->init_export ? 1 : 0; // ovgpu_slam_init_systems: the host decides the gate again, rejected features are exported too
  p.opt.feat_rep = init_rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH : init_rep; // UpdaterSLAM.cpp:151-155
  p.init_dof_less = init_rep == OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE ? 2 : 0;
}

// f_one >= 0: only that feature, in StateHelper::initialize mode with the landmark representation init_rep
// whiten: the rows leave as [H L | r] with L = c->Lw (the prior block's factor must be complete on this stream)
static int enqueue_system(ovgpu_ctx *c, int f_one = -1, int init_rep = 0, bool whiten = false) {
  const Batch b = batch_of(c);
  if (b.F == 0) return OVGPU_OK;
  SysParams p;
  fill_sys_params(c, b, p);
  c->stack_is_f32 = false;
  p.Lw = (whiten && f_one < 0) ? c->Lw.p : nullptr;
  c->last_stack_raw = false;
  if (f_one < 0) c->last_feat_kernel = FK_GENERAL;
  if (f_one < 0) HIPCHK(ctrl_zero(c, CTRL_ROWS, c->rows_used.p, 2 * sizeof(int32_t), c->stream));
  if (f_one >= 0) sys_params_init_mode(c, p, f_one, init_rep);
  // ovgpu_debug_option "feat_classes": a batch laid out by length classes runs a kernel per class when this launch is one the fused kernels take at
  // all (the whitened route, one noise level, no landmark column) and no launch-time switch rules the classes out — "featy_big", or options.gram_fp32
  // next to a general class, whose kernel writes no float stack.  Otherwise the single-kernel rule holds (select_feat_kernel).  Every class is
  // selected and held against its carve HERE, in front of the first launch: a refused class refuses the pipeline.
  const FeatPlan &pl = c->plan;
  const bool by_class = f_one < 0 && pl.n_classes >= 2 && p.Lw && !c->featy_big && (c->L == 0 || (c->lm_fast_on && pl.lm_fast_ok)) && !p.slam && !p.feat_sigma &&
                        !p.feat_chi2mult && !(pl.cls_general() && c->want_stack_f32) && (int)b.h_order.size() == b.F;
  FeatLaunch sc[featcls::FC_MAX];
  for (int k = 0; by_class && k < pl.n_classes; k++) {
    const int f0 = pl.cls[k].begin < b.F && pl.cls[k].end <= b.F ? b.h_order[pl.cls[k].begin] : -1;
    if (f0 < 0) return set_err(OVGPU_ERR_INVALID, "internal: a length class lies outside the batch in force");
    sc[k] = select_feat_kernel(c, p, b.F, -1, &pl.cls[k], b.h_offsets[f0 + 1] - b.h_offsets[f0]);
    if (sc[k].err != OVGPU_OK) return set_err(sc[k].err, sc[k].msg);
  }
  // (by classes: `s` is the longest FUSED class's launch — what the head below is sized and switched by)
  const FeatLaunch s = by_class ? sc[pl.cls_general() ? 1 : 0] : select_feat_kernel(c, p, b.F, f_one);
  if (s.err != OVGPU_OK) return set_err(s.err, s.msg);
  if (s.cb) { // the head of the MSCKF fast path
    p.row_stride = 48; // the fused kernels' records (fs_rows holds M * c->row_stride >= 48 M doubles): a 72-double stride — an anchored feat_rep_msckf, anchored
                       // landmarks, an earlier delayed initialisation — is the general kernel's alone
    HIPCHK(ctrl_zero(c, CTRL_COUNTER, c->feat_counter.p, sizeof(int32_t), c->stream));
    p.work_counter = c->feat_counter.p;
    // rows (per measurement) -> gate (needs P only) -> projected whitened rows (need L and z).  The prior block's factorisation and
    // the reflector / z kernel behind it run on the second stream NEXT TO the gate; only the output kernel waits for them.
    // The fused form (k_featy.h): rows (clone-major) -> reflectors -> [prior block's factor L joins] -> sweep Y = H L once per feature:
    // projected rows to the stack, gate matrix as Y Y^T + s^2 I on the matrix cores, Cholesky, chi2
    feat::FeatStore st{c->fs_rows.p, c->fs_minfo.p, c->fs_V.p, c->fs_z.p, c->fs_meas_feat.p, c->fs_w.p, c->fs_pos.p};
    if (s.f32) { // options.gram_fp32: the rows leave as floats, stride 32 ceil(LD / 32) (k_gram32.h)
      c->stack_ldf = ((c->LD + 31) / 32) * 32;
      HIPCHK(c->Hbig32.reserve((size_t)(std::max<int64_t>(b.rows_total, 1) + 32) * c->stack_ldf));
      // k_gram_f32 copies whole 32-row stages: the rows behind the last feature's must read as zeros
      HIPCHK(hipMemsetAsync(c->Hbig32.p + (size_t)b.rows_total * c->stack_ldf, 0, sizeof(float) * 32 * c->stack_ldf, c->stream));
      p.Hbig32 = c->Hbig32.p, p.LDF = c->stack_ldf;
      c->stack_is_f32 = true;
    }
    if (p.opt.feat_rep >= OVGPU_REP_ANCHORED_3D) hipLaunchKernelGGL(feat::k_feat_rows_anchored, dim3((b.M + 255) / 256), dim3(256), 0, c->stream, p, st, b.M);
    else hipLaunchKernelGGL(feat::k_feat_rows_sorted, dim3((b.M + 255) / 256), dim3(256), 0, c->stream, p, st, b.M);
    // (by classes: every class a one-pass kernel — the longest fused one is, and there is no general class)
    if (c->raw_enable && c->raw_tables_ok && !c->raw_veto && s.kernel != FK_FEATY_BIG && !s.f32 && s.cb == feat::FY_CB && !(by_class && pl.cls_general())) {
      p.raw.on = 1, p.raw.ncls = c->raw_ncls, p.raw.H = c->Hraw.p, p.raw.dst = c->raw_dst.p, p.raw.j0 = c->raw_j0;
      for (int k = 0; k <= RAW_NEG; k++) p.raw.base[k] = c->raw_base[k], p.raw.ld[k] = c->raw_ld[k], p.raw.rcol[k] = c->raw_rcol[k];
      c->last_stack_raw = true;
    }
    if (c->inst_cb != s.cb || c->inst_D != c->D) { // (a switch thrown after the batch was laid out)
      const int rci = enqueue_instance_lists(c, s.cb);
      if (rci != OVGPU_OK) return rci;
    }
    if (by_class && pl.cls_mixed_width() && c->inst64_D != c->D) { // (likewise the one-pass classes' lists next to a block-row class)
      const int rci = enqueue_instance_lists64(c);
      if (rci != OVGPU_OK) return rci;
    }
    SysParams pv = p; // k_feat_vt's block holds the longest track the fused kernels take: the batch's, or by classes the longest fused class's (a general-class track returns at once)
    if (by_class) pv.m_max = std::max(pl.m_fused, 1);
    hipLaunchKernelGGL(with_max_lds<feat::k_feat_vt>(c), dim3((b.F + 3) / 4), dim3(256), (size_t)4 * (14 * pv.m_max + 64) * sizeof(double), c->stream, pv, st, c->fs_tq.p);
  }
  if (p.Lw && c->prior_on_side) { // the general kernel and k_slam_y read L from their first instruction on, the fused MSCKF kernels behind k_feat_vt
    // (L and the carried columns come out of one launch since round 5)
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->prior_on_side = false; // this stream is behind the factorisation from here on: the update's second half needs no wait of its own (a wait on a
                              // completed event still costs the queue ~6 us in front of the second factorisation)
  }
  if (s.kernel == FK_FEATY_BIG && c->plan.msckf != FK_FEATY_BIG) HIPCHK(c->featyb_ws.reserve((size_t)s.grid * feat::featyb_ws_doubles(c->plan.nt))); // ("featy_big": the batch was not laid out for it)
  if (s.kernel >= FK_SLAMY) c->slam_fused_batches++, c->slam_fused_attempt++;
  if (s.kernel == FK_GENERAL) p.rows_ws = s.alt ? c->sys_rows_ws.p : nullptr;
  if (f_one < 0) {
    c->last_feat_kernel = by_class ? sc[0].code : s.code; // (by classes: the kernel of the batch's longest track)
    c->last_feat_classes = 0;
    for (int k = 0; k < featcls::FC_MAX; k++) c->last_class_features[k] = 0;
    if (!by_class && s.code <= FK_FEATY_BIG) c->last_feat_classes = 1 << s.code, c->last_class_features[s.code] = b.F;
  }
  if (!by_class) return launch_feat_kernel(c, s, p);
  // a launch per class, longest class first, on this stream: the deal inside a launch is what it was, the slots it walks are the class's
  c->feat_class_batches++, c->feat_class_attempt++;
  for (int k = 0; k < pl.n_classes; k++) {
    SysParams pk = p;
    pk.f_begin = pl.cls[k].begin, pk.f_end = pl.cls[k].end; // (the general kernel's range over p.order; a fused kernel walks pk.F slot records from the range's first: launch_feat_kernel)
    if (sc[k].kernel != FK_GENERAL) pk.F = pk.f_end - pk.f_begin;
    if (sc[k].kernel == FK_GENERAL) // (its own records at its own stride: the head above set the fused kernels' 48)
      pk.rows_ws = sc[k].alt ? c->sys_rows_ws.p : nullptr, pk.row_stride = c->row_stride, pk.raw.on = 0, pk.Hbig32 = nullptr, pk.LDF = 0;
    c->last_feat_classes |= 1 << sc[k].code, c->last_class_features[sc[k].code] = pk.f_end - pk.f_begin;
    const int rc = launch_feat_kernel(c, sc[k], pk);
    if (rc != OVGPU_OK) return rc;
  }
  return OVGPU_OK;
}

// merges triangles Rws[0..G) pairwise until Rws[0] holds the result
static bool tree_can_pipeline(const ovgpu_ctx *c, int G) {
  const int NT = (c->LD + 15) / 16;
  return c->tree_pipelined && NT <= 16 && G - 1 <= c->num_cu;
}

// leaves_live: the leaf kernel is running concurrently (other stream) and publishes its last append panel by panel
static int enqueue_merge_tree(ovgpu_ctx *c, int G, bool leaves_live = false, hipStream_t on = nullptr) {
  const int D = c->D, LD = c->LD;
  const int NT = (LD + 15) / 16;
  if (G <= 1) return OVGPU_OK;
  hipStream_t ts = on ? on : c->stream;
  c->tsqr_last_qh = NT <= 8 ? 16 : (NT <= 14 ? 28 : (NT <= 16 ? 32 : 0));
  if (c->tree_pipelined && NT <= 16 && G - 1 <= c->num_cu) {
    c->tsqr_last_tree = leaves_live ? 1 : 2;
    // ---- one launch for the whole tree, software-pipelined across the levels (k_qr_tree)
    DevBuf<QrTreeNode> *slot = nullptr;
    if (c->tree_G == G && c->tree_nodes_overlap == leaves_live) slot = &c->tree_nodes;
    else if (c->tree_G2 == G && c->tree_nodes2_overlap == leaves_live) slot = &c->tree_nodes2;
    if (!slot) {
      slot = (c->tree_G == 0) ? &c->tree_nodes : &c->tree_nodes2; // the first tree built stays, the second slot is replaced
      std::vector<QrTreeNode> nodes;
      std::vector<int32_t> writer(G, -1); // node that produces the current content of a slot
      if (leaves_live)
        for (int i = 0; i < G; i++) writer[i] = -(i + 2); // leaf i, still running
      for (int stride = 1; stride < G; stride <<= 1)
        for (int i = 0; i + stride < G; i += 2 * stride) {
          QrTreeNode n;
          n.a_slot = i, n.b_slot = i + stride, n.dep_a = writer[i], n.dep_b = writer[i + stride];
          writer[i] = (int32_t)nodes.size();
          nodes.push_back(n);
        }
      HIPCHK(slot->reserve(nodes.size()));
      if (!c->tree_err.p) {
        HIPCHK(c->tree_err.reserve(1));
        HIPCHK(hipMemsetAsync(c->tree_err.p, 0, sizeof(int32_t), c->stream));
      }
      HIPCHK(hipMemcpyAsync(slot->p, nodes.data(), nodes.size() * sizeof(QrTreeNode), hipMemcpyHostToDevice, c->stream));
      HIPCHK(upload_sync(c, c->stream)); // the host vector goes out of scope
      if (slot == &c->tree_nodes) c->tree_G = G, c->tree_nodes_overlap = leaves_live;
      else c->tree_G2 = G, c->tree_nodes2_overlap = leaves_live;
    }
    HIPCHK(c->tree_flags.reserve((size_t)G));
    const int n_nodes = G - 1;
    if (!leaves_live) HIPCHK(hipMemsetAsync(c->tree_flags.p, 0, sizeof(int32_t) * (n_nodes + 1), ts)); // (overlap: zeroed before the fork)
    QrTreeParams q;
    q.D = D, q.LD = LD, q.NT = NT, q.tri = c->Rws.p, q.nodes = slot->p;
    q.progress = c->tree_flags.p, q.leaf_progress = leaves_live ? c->leaf_flags.p : nullptr, q.error = c->tree_err.p;
    q.spin_limit = 4000000; // ~ seconds: only a lost node gets there
    q.dbg = tree_dbg_buffer();
    if (NT <= 8) return launch_qr_tree<16>(c, n_nodes, q, ts);
    if (NT <= 14) return launch_qr_tree<28>(c, n_nodes, q, ts);
    return launch_qr_tree<32>(c, n_nodes, q, ts);
  }
  c->tsqr_last_tree = 3;
  for (int stride = 1; stride < G; stride <<= 1) {
    const int pairs = (G - stride + 2 * stride - 1) / (2 * stride); // i = 0, 2s, 4s, ... with i + s < G
    if (pairs <= 0) break;
    if (NT <= 16) {
      QrNodeParams q;
      q.D = D, q.LD = LD, q.NT = NT;
      q.acc = c->Rws.p, q.acc_stride = 2 * (int64_t)stride;
      q.src = c->Rws.p + (size_t)stride * D * LD, q.src_stride = 2 * (int64_t)stride * D * LD;
      q.rows_per_node = D, q.rows_total = D, q.zero_init = 0, q.dbg = qr_dbg_buffer(), q.progress = nullptr;
      int rc;
      // a merge node needs QH >= 4 NW quads per register array (NW = ceil(NT / 2) waves)
      if (NT <= 8) rc = launch_qr_node<16, true>(c, pairs, q);
      else if (NT <= 14) rc = launch_qr_node<28, true>(c, pairs, q);
      else rc = launch_qr_node<32, true>(c, pairs, q);
      if (rc != OVGPU_OK) return rc;
    } else {
      const int nt = ((LD + 63) / 64) * 64;
      QrAppendParams q;
      q.D = D, q.LD = LD;
      q.dst = c->Rws.p, q.dst_wg_stride = 2 * (int64_t)stride;
      q.src = c->Rws.p + (size_t)stride * D * LD, q.src_wg_stride = 2 * (int64_t)stride * D * LD;
      q.src_rows_per_wg = D, q.src_rows_total = D, q.triangular = 1, q.zero_dst = 0;
      hipLaunchKernelGGL(k_qr_append<QR_B>, dim3(pairs), dim3(nt), 0, c->stream, q);
      HIPCHK(hipGetLastError());
    }
  }
  return OVGPU_OK;
}

// G = [H | r]^T [H | r] on the matrix cores (k_gram.h): partial Gram matrices per workgroup, ordered sum; factor = true (mode A)
// adds its diagonally pivoted Cholesky factor
static int enqueue_gram_factor(ovgpu_ctx *c);
// Row shares of k_gram_blk (gridDim.x; gridDim.y is the block pair) over a stack of `nchunks` stages of 32 rows.  Up to 24 tile columns, at most six
// pairs: one share per compute unit, as ever (the reduction sums the shares in order: another count is other bits).  At 25 .. 32 tile columns the
// stack is read TEN times, and every workgroup leaves 64 partial tiles (128 KB) whatever it summed: a share per compute unit would be 2560 workgroups
// and 335 MB of partials, written and read again, against a stack of a few dozen MB.  The kernel's two staged windows take 135 KB of LDS, so a
// compute unit holds one workgroup: num_cu / 10 shares (rounded down) put all ten passes on the device in ONE round of workgroups, every compute unit
// streaming a tenth of the rows per pass it owns, and the partials stay at 32 MB.
static int gram_blk_row_shares(const ovgpu_ctx *c, int NT, int64_t nchunks) {
  int shares = c->num_cu;
  if (NT > gram::GR_NT_BLK) shares = std::max(1, c->num_cu / (gram::GR_NT_WIDE / gram::GB_T * (gram::GR_NT_WIDE / gram::GB_T + 1) / 2));
  return (int)std::max<int64_t>(1, std::min<int64_t>(shares, nchunks));
}
// What enqueue_compress_gram reserves of c->gram_part, in doubles, for NT tile columns and a stack of `nchunks` stages, whichever of its kernels runs:
// the one-pass kernels and k_gram_wide leave a triangle of NT (NT + 1) / 2 partial tiles per share, k_gram_blk (17 .. 32 tile columns, and every count
// of a gram_fp32 context) 64 per share and block pair.  ovgpu_slam_update_chunked sizes the buffer by this in front of its first launch.
static size_t gram_part_doubles(const ovgpu_ctx *c, int NT, int64_t nchunks) {
  const size_t G = (size_t)std::max<int64_t>(1, std::min<int64_t>(c->num_cu, nchunks));
  size_t need = NT <= gram::GR_NT_BLK ? G * (size_t)(NT * (NT + 1) / 2) * 256 : 0;
  if (NT > gram::GR_NT || c->gram_fp32) {
    const size_t NB = (size_t)(NT + gram::GB_T - 1) / gram::GB_T, pairs = NB * (NB + 1) / 2;
    need = std::max(need, pairs * (size_t)gram_blk_row_shares(c, NT, nchunks) * gram::GB_T * gram::GB_T * 256);
  }
  return need;
}
// The Gram route's capacity in tile columns of [H | r] for the updates of this context: 32 under ovgpu_debug_option "gram_wide" on a float64 context
// with the whitened stack (DESIGN.md §7), 24 otherwise.  The speculative prior, the local-Gram, sharded and multi entries keep gram::GR_NT_BLK
// whatever the switch says; mode A (factor_gram) has a switch of its own (mode_a_tile_cap).
static int gram_route_tile_cap(const ovgpu_ctx *c) { return c->gram_wide_on >= 1 && c->whiten && !c->gram_fp32 ? gram::GR_NT_WIDE : gram::GR_NT_BLK; }
// ... and for mode A's pivoted factor (factor_gram, enqueue_pipeline_body): 32 under ovgpu_debug_option "mode_a_wide" on a float64 context with the
// whitened stack (k_pchol_wide.h, k_unwhiten_blk<32>), 24 otherwise.  The two switches are independent of each other.
static int mode_a_tile_cap(const ovgpu_ctx *c) { return c->mode_a_wide_on >= 1 && c->whiten && !c->gram_fp32 ? gram::GR_NT_WIDE : gram::GR_NT_BLK; }
// ... and the lower edge, in tile columns of [H | r], of the panelled pivoted factor under ovgpu_debug_option "mode_a_panel" (include/ovgpu.h names it at
// ovgpu_msckf_compress): from here to gram::GR_NT_BLK the switch sends the factor to k_pchol_panel / k_pchol_schur instead of the rank-one k_gram_pchol<NB>.
// Measured (DESIGN.md section 7): at 15 and 16 tile columns the rank-one k_gram_pchol<8> — no spills at eight blocks — is as fast as seven or eight panels with
// their launch boundaries, so the edge sits at 17, where the Gram kernel, the prior's factorisation and the un-whitening change as well.
constexpr int MODE_A_PANEL_MIN_NT = 17; // D = 256
// Mode A's factor comes here on a float64 context with the whitened stack only (factor_gram, enqueue_pipeline_body), so the level and the width decide.
static bool mode_a_panel_factor(const ovgpu_ctx *c, int NTf) { return c->mode_a_panel_on >= 1 && NTf >= MODE_A_PANEL_MIN_NT && NTf <= gram::GR_NT_BLK; }
static int enqueue_compress_gram(ovgpu_ctx *c, bool factor = true) {
  const int D = c->D, LD = c->LD, NT = (LD + 15) / 16, NP = NT * (NT + 1) / 2, LG = 16 * NT;
  const int64_t rows_total = batch_of(c).rows_total;
  const int64_t nchunks = (rows_total + gram::GR_ROWS - 1) / gram::GR_ROWS;
  const int G = (int)std::max<int64_t>(1, std::min<int64_t>(c->num_cu, nchunks));
  if (NT <= gram::GR_NT_BLK) HIPCHK(c->gram_part.reserve((size_t)G * NP * 256)); // (beyond: k_gram_blk's own, smaller reserve below)
  HIPCHK(c->gram_G.reserve((size_t)LG * LG));
  if (c->stack_is_f32) { // the fp32 stack of options.gram_fp32: one pass per part of the macro-tile triangle (k_gram32.h)
    const int LDF = c->stack_ldf, NTM = LDF / 32, P = gram32::gram32_parts(NTM), slots = P * gram32::G32_NW * gram32::G32_MAXT;
    if (c->gram32_ntm != NTM || c->gram32_P != P) {
      std::vector<int32_t> tab((size_t)slots);
      gram32::gram32_tile_table(NTM, P, tab.data());
      HIPCHK(c->gram32_tiles.reserve((size_t)slots));
      HIPCHK(hipMemcpyAsync(c->gram32_tiles.p, tab.data(), sizeof(int32_t) * slots, hipMemcpyHostToDevice, c->stream));
      HIPCHK(upload_sync(c, c->stream)); // (the staging vector goes; once per column count)
      c->gram32_ntm = NTM, c->gram32_P = P;
    }
    // workgroups per part: no more than G32_ROWS_WG rows each; on a short stack as many as keep every compute unit busy (>= 4 stages each)
    const int64_t by_rows = (rows_total + gram32::G32_ROWS_WG - 1) / gram32::G32_ROWS_WG;
    const int64_t by_cus = std::min<int64_t>((2 * c->num_cu + P - 1) / P, (rows_total + 127) / 128);
    const int Gw = (int)std::max<int64_t>(1, std::max(by_rows, by_cus));
    HIPCHK(c->gram32_part.reserve((size_t)P * Gw * gram32::G32_NW * gram32::G32_MAXT * 1024));
    gram32::Gram32Params q;
    q.H = c->Hbig32.p, q.part = c->gram32_part.p, q.tiles = c->gram32_tiles.p, q.rows_total = rows_total, q.LDF = LDF, q.LD = LD;
    hipLaunchKernelGGL(with_max_lds<gram32::k_gram_f32>(c), dim3(Gw, P), dim3(gram32::G32_NTH), gram32::gram32_lds_bytes(LDF), c->stream, q);
    hipLaunchKernelGGL(gram32::k_gram_f32_reduce, dim3(slots, 4), dim3(256), 0, c->stream, (const int32_t *)c->gram32_tiles.p, Gw,
                       (const float *)c->gram32_part.p, c->gram_G.p, LG);
    HIPCHK(hipGetLastError());
    c->last_gram_kernel = 5, c->last_gram_workgroups = Gw;
    return factor ? set_err(OVGPU_ERR_CAPACITY, "the fp32 Gram variant feeds the on-device update only") : OVGPU_OK;
  }
  if (c->last_stack_raw) { // the unprojected stack, region by region (k_gram.h: k_gram_regions), the dropped rows' region subtracted in the reduction
    HIPCHK(c->gram_part.reserve((size_t)std::max(c->gram_wg_tiles, 1) * 256));
    const int waves = c->gram_read_ahead ? c->gram_waves : 4; // (two wavefronts per SIMD exist with the reads ahead only)
    const auto kern = !c->gram_read_ahead ? with_max_lds<gram::k_gram_regions<false>>(c)
                      : waves == 8        ? with_max_lds<gram::k_gram_regions<true, 8>>(c)
                                          : with_max_lds<gram::k_gram_regions<true>>(c);
    hipLaunchKernelGGL(kern, dim3(c->gram_wg_n), dim3(64 * waves), gram::gram_lds_bytes(), c->stream, (const double *)c->Hraw.p, (const gram::GramRegionWG *)c->gram_wg.p,
                       c->gram_part.p);
    hipLaunchKernelGGL(gram::k_gram_regions_reduce, dim3(NP, 256 / gram::RR_E), dim3(gram::RR_E * gram::RR_G), 0, c->stream, NT, D, c->raw_rs,
                       (const gram::GramRegionWG *)c->gram_wg.p, c->gram_wg_n, (const double *)c->gram_part.p, c->gram_G.p);
    HIPCHK(hipGetLastError());
    c->last_gram_kernel = 4;
    return factor ? enqueue_gram_factor(c) : OVGPU_OK;
  }
  gram::GramParams g;
  g.LD = LD, g.NT = NT, g.rows_total = rows_total, g.H = c->Hbig.p, g.part = c->gram_part.p;
  if (NT == gram::GR_NT + 7 && !c->gram_fp32 && !c->gram_blocks_only) { // configs[4]'s 23 tile columns: two passes over the stack (k_gram_wide)
    const int Gw = G; // (every workgroup of either kernel writes its own tiles of partial blockIdx.x)
    hipLaunchKernelGGL(with_max_lds<gram::k_gram_wide_top<7>>(c), dim3(Gw), dim3(256), gram::gram_wide_top_lds_bytes(), c->stream, g);
    hipLaunchKernelGGL(with_max_lds<gram::k_gram_wide_win<7>>(c), dim3(Gw), dim3(256), gram::gram_lds_bytes(), c->stream, g);
    hipLaunchKernelGGL(gram::k_gram_reduce, dim3(NP), dim3(1024), 0, c->stream, NT, Gw, c->gram_part.p, c->gram_G.p);
    HIPCHK(hipGetLastError());
    c->last_gram_kernel = 3;
    return factor ? enqueue_gram_factor(c) : OVGPU_OK; // (the pivoted factor: k_gram_pchol<9 .. 12> up to 383 columns, k_pchol_wide.h beyond)
  }
  if (NT > gram::GR_NT || c->gram_fp32) { // more than 255 columns (configs[4]), or its fp32 variant: 8 x 8-tile blocks of the grid, one block pair per blockIdx.y
    const int NB = (NT + gram::GB_T - 1) / gram::GB_T, pairs = NB * (NB + 1) / 2;
    const int Gb = gram_blk_row_shares(c, NT, nchunks);
    HIPCHK(c->gram_part.reserve((size_t)pairs * Gb * gram::GB_T * gram::GB_T * 256));
    g.part = c->gram_part.p;
    if (!c->gram_fp32) hipLaunchKernelGGL(with_max_lds<gram::k_gram_blk<false>>(c), dim3(Gb, pairs), dim3(256), gram::gram_blk_lds_bytes(), c->stream, g, NB);
    else hipLaunchKernelGGL(with_max_lds<gram::k_gram_blk<true>>(c), dim3(Gb, pairs), dim3(256), gram::gram_blk_lds_bytes() / 2, c->stream, g, NB);
    hipLaunchKernelGGL(gram::k_gram_blk_reduce, dim3(gram::GB_T * gram::GB_T, pairs), dim3(256), 0, c->stream, NB, NT, Gb, c->gram_part.p, c->gram_G.p);
    HIPCHK(hipGetLastError());
    c->last_gram_kernel = 2, c->last_gram_workgroups = Gb;
    return factor ? enqueue_gram_factor(c) : OVGPU_OK; // (the pivoted factor: k_gram_pchol<9 .. 12> up to 383 columns, k_pchol_wide.h beyond)
  }
  switch ((NT + 1) / 2) {
  case 1: launch_gram<2>(c, G, g, c->stream, c->gram_il); break;
  case 2: launch_gram<4>(c, G, g, c->stream, c->gram_il); break;
  case 3: launch_gram<6>(c, G, g, c->stream, c->gram_il); break;
  case 4: launch_gram<8>(c, G, g, c->stream, c->gram_il); break;
  case 5: launch_gram<10>(c, G, g, c->stream, c->gram_il); break;
  case 6: launch_gram<12>(c, G, g, c->stream, c->gram_il); break;
  case 7: launch_gram<14>(c, G, g, c->stream, c->gram_il); break;
  default:
    if (NT == 15) launch_gram<15>(c, G, g, c->stream, c->gram_il); // (the one odd count with a grid of its own: configs[3], D = 236)
    else launch_gram<16>(c, G, g, c->stream, c->gram_il);
    break;
  }
  hipLaunchKernelGGL(gram::k_gram_reduce, dim3(NP), dim3(1024), 0, c->stream, NT, G, c->gram_part.p, c->gram_G.p);
  HIPCHK(hipGetLastError());
  c->last_gram_kernel = 1;
  return factor ? enqueue_gram_factor(c) : OVGPU_OK;
}

// diagonally pivoted Cholesky of c->gram_G into c->Rws (k_gram_pchol): the stable factor of a semi-definite matrix (mode A)
static int enqueue_gram_factor(ovgpu_ctx *c) {
  const int D = c->D, LD = c->LD, LG = 16 * ((LD + 15) / 16);
  HIPCHK(c->gram_dropped.reserve(2)); // [0] the dropped rows, [1] k_pchol_wide.h's stop word
  const double tol = 1e-15;
  // round 6: blocked — the upper block triangle as 16 x 16 tiles in the registers of 7 wavefronts, one matrix instruction per tile and four
  // pivots, the pivot-by-pivot work in one wavefront (k_pchol.h); up to 14 tile columns (223 Jacobian columns: configs[0..2]).  Beyond — 17 tiles
  // per wavefront in nine wavefronts' 168 registers — the kernel spills, and the rank-one kernel stays.
  const int NTf = (LD + 15) / 16;
  // 25 .. 32 tile columns ("mode_a_wide"): panels of 32 pivots around Schur steps, in place on c->gram_G (k_pchol_wide.h); under "mode_a_panel" 17 .. 24
  // tile columns as well (both kernels are generic in LG, and every Gram reduction of this route writes the full symmetric square)
  if (NTf > gram::GR_NT_BLK || mode_a_panel_factor(c, NTf)) {
    if (NTf > gram::GR_NT_WIDE) return set_err(OVGPU_ERR_CAPACITY, "the pivoted Gram factor holds at most 511 Jacobian columns");
    HIPCHK(c->pchol_dots.reserve((size_t)gram::PW_LGMAX + 8));
    gram::PcholWideParams q;
    q.D = D, q.LD = LD, q.LG = LG, q.G = c->gram_G.p, q.out = c->Rws.p, q.dots = c->pchol_dots.p, q.ctl = c->gram_dropped.p, q.tol = tol;
    // every launch of the largest panel count up front: the panel that stops tells the later ones through ctl[PW_DONE]
    const int panels = gram::pchol_wide_panels(D), tiles = (LG / 16) * (LG / 16);
    for (int pn = 0; pn < panels; pn++) {
      q.k0 = pn * gram::PW_NB;
      hipLaunchKernelGGL(with_max_lds<gram::k_pchol_panel>(c), dim3(1), dim3(gram::PW_LGMAX), gram::pchol_wide_lds_bytes(), c->stream, q);
      if (pn + 1 < panels) hipLaunchKernelGGL(gram::k_pchol_schur, dim3((tiles + 3) / 4), dim3(256), 0, c->stream, q);
    }
    HIPCHK(hipGetLastError());
    c->last_factor_kernel = 3;
    return OVGPU_OK;
  }
  if (c->pchol_blocked && NTf <= 14) {
    if (NTf <= 8) launch_gram_pchol_blk<4, 9, 2>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol);
    else launch_gram_pchol_blk<7, 15, 4>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol);
    HIPCHK(hipGetLastError());
    c->last_factor_kernel = NTf <= 8 ? 1 : 2;
    return OVGPU_OK;
  }
  switch ((LD + 31) / 32) {
  case 1: launch_gram_pchol<1>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 2: launch_gram_pchol<2>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 3: launch_gram_pchol<3>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 4: launch_gram_pchol<4>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 5: launch_gram_pchol<5>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 6: launch_gram_pchol<6>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 7: launch_gram_pchol<7>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 8: launch_gram_pchol<8>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 9: launch_gram_pchol<9>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 10: launch_gram_pchol<10>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 11: launch_gram_pchol<11>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  case 12: launch_gram_pchol<12>(c->stream, D, LD, LG, c->gram_G.p, c->Rws.p, c->gram_dropped.p, tol); break;
  default: return set_err(OVGPU_ERR_CAPACITY, "the pivoted Gram factor holds at most 383 Jacobian columns");
  }
  HIPCHK(hipGetLastError());
  c->last_factor_kernel = 32 + (LD + 31) / 32;
  return OVGPU_OK;
}

// Householder TSQR of the stack: leaf nodes + merge tree (k_tsqr_pw.h, k_tsqr.h)
static int enqueue_compress(ovgpu_ctx *c) {
  const int D = c->D, LD = c->LD;
  const int NT = (LD + 15) / 16;
  const int W = c->W;
  const int64_t rows_total = batch_of(c).rows_total;
  c->tsqr_last_W = W, c->tsqr_last_rpn = c->rows_per_node, c->tsqr_last_tree = 0, c->tsqr_last_qh = 0;
  c->tsqr_last_leaf = NT <= 15 ? 0 : (NT == 16 ? 1 : 2);
  if (NT <= 16) {
    QrNodeParams q;
    q.D = D, q.LD = LD, q.NT = NT;
    q.acc = c->Rws.p, q.acc_stride = 1;
    q.src = c->Hbig.p, q.src_stride = 0;
    q.rows_per_node = c->rows_per_node, q.rows_total = rows_total, q.zero_init = 1, q.dbg = qr_dbg_buffer(), q.progress = nullptr;
    // The merge tree can run NEXT TO the leaf kernel (second stream): leaf nodes publish the panels of their last append
    // as they finish, level-1 merge nodes pick them up.  Both kernels run 256-VGPR waves, two per SIMD, so a leaf and a
    // merge workgroup do NOT share a CU: the overlap pays only while leaves + merge nodes (2W-1) fit the chip one per CU
    // (measured with W=203: 53 merge nodes start with the leaves, the other 149 when the leaves retire -> no gain).
    // Leaves never wait, so a merge node that got its CU first only spins until they come.
    const bool want_overlap = c->tree_overlap < 0 ? (2 * W - 1 <= c->num_cu) : c->tree_overlap != 0;
    const bool overlap = want_overlap && NT <= 15 && W > 1 && tree_can_pipeline(c, W);
    if (overlap) {
      HIPCHK(c->leaf_flags.reserve(W));
      HIPCHK(c->tree_flags.reserve((size_t)W));
      HIPCHK(hipMemsetAsync(c->leaf_flags.p, 0, sizeof(int32_t) * W, c->stream));
      HIPCHK(hipMemsetAsync(c->tree_flags.p, 0, sizeof(int32_t) * W, c->stream));
      q.progress = c->leaf_flags.p;
      HIPCHK(hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    const int rc = NT <= 15 ? launch_qr_leaf_pw<QR_LEAF_Q>(c, W, q) : launch_qr_node<QR_LEAF_Q, false>(c, W, q);
    if (rc != OVGPU_OK) return rc;
    if (overlap) {
      const int rt = enqueue_merge_tree(c, W, true, c->stream2);
      if (rt != OVGPU_OK) return rt;
      HIPCHK(hipEventRecord(c->ev_join, c->stream2));
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
      return OVGPU_OK;
    }
  } else {
    const int nt = ((LD + 63) / 64) * 64;
    QrAppendParams q;
    q.D = D, q.LD = LD;
    q.dst = c->Rws.p, q.dst_wg_stride = 1;
    q.src = c->Hbig.p, q.src_wg_stride = c->rows_per_node * LD;
    q.src_rows_per_wg = c->rows_per_node, q.src_rows_total = rows_total, q.triangular = 0, q.zero_dst = 1;
    hipLaunchKernelGGL(k_qr_append<QR_B>, dim3(W), dim3(nt), 0, c->stream, q);
    HIPCHK(hipGetLastError());
  }
  return enqueue_merge_tree(c, W);
}

struct EkfJob {
  const double *R = nullptr;          // system rows [rows x LD]; nullptr: the compressed triangle in c->Rws
  int rows = -1;                      // -1: c->D (upper triangular)
  const int32_t *col_cov = nullptr;   // nullptr: the context's column map
  double sigma2 = -1.0;               // < 0: the context's sigma_pix^2
  const int32_t *pred = nullptr;      // device flag: skip everything when 0
  double *dx = nullptr;               // nullptr: c->dx
  bool keep_flags = false;            // do not clear the sticky error flags (a chain of updates)
};

struct CholSource { // where the factorisation reads [A | C] (k_chol.h CH_SRC_*); MATRIX: p.A
  int src = chol::CH_SRC_MATRIX;
  const TformParams *t = nullptr;
};
static int enqueue_chol_carry(ovgpu_ctx *c, const EkfParams &p, hipStream_t s, double *Lt, const CholSource &from = CholSource());

static int enqueue_ekf(ovgpu_ctx *c, const EkfJob &job = EkfJob()) {
  { // (this update uses the work matrices and flag words of a prior-block factorisation that may still be on the second stream)
    const int rdp = drop_pending_prior(c);
    if (rdp != OVGPU_OK) return rdp;
  }
  c->last_update_tform = false;
  EkfParams p;
  const bool tri = job.R == nullptr;
  p.N = c->N, p.D = tri ? c->D : job.rows, p.DC = c->D, p.LD = c->LD, p.LA = p.D + c->N + 1, p.tri = tri ? 1 : 0, p.pred = job.pred;
  p.R = tri ? c->Rws.p : job.R, p.col_cov = job.col_cov ? job.col_cov : c->col_cov.p, p.P = c->P.p, p.Mt = c->Mt.p, p.A = c->Aaug.p, p.Y = c->Yaug.p;
  p.dx = job.dx ? job.dx : c->dx.p, p.flags = c->flags.p;
  p.sigma2 = job.sigma2 >= 0.0 ? job.sigma2 : c->dopt.sigma_pix_sq;
  hipStream_t s = c->stream;
  if (!job.keep_flags) HIPCHK(ctrl_zero(c, CTRL_FLAGS, c->flags.p, 4 * sizeof(int32_t), s));
  const int tm = (p.D + 15) / 16, tn = (p.N + 15) / 16;
  hipLaunchKernelGGL(k_ekf_mt, dim3((tm * tn + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_ekf_s, dim3((tm * tm + 3) / 4), dim3(256), 0, s, p);
  // Cholesky of S carried through [Mt | c]
  {
    const int rcc = enqueue_chol_carry(c, p, s, nullptr);
    if (rcc != OVGPU_OK) return rcc;
  }
  hipLaunchKernelGGL(k_ekf_dx, dim3((p.N + 255) / 256), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_ekf_pupdate, dim3((tn * tn + 3) / 4), dim3(256), 0, s, p);
  const int n = std::max(c->C, c->K);
  hipLaunchKernelGGL(k_boxplus, dim3((n + 255) / 256), dim3(256), 0, s, c->C, c->K, p.dx, c->clone_cov.p, c->calib_cov.p, c->intr_cov.p,
                     c->clone_qp.p, c->calib_qp.p, c->intr.p, job.pred);
  if (c->lm_fast_on && c->L > 0) // ovgpu_msckf_update_lm on the Householder route (k_tail.h; p.pred is the box-plus's job.pred, p.pred_not is null)
    hipLaunchKernelGGL(k_lm_correct, dim3((3 * c->L + 255) / 256), dim3(256), 0, s, p, c->L, (const int32_t *)c->lm_repd.p, (const int32_t *)c->lm_cov.p, c->lm_val.p);
  HIPCHK(hipGetLastError());
  return launch_build_tables(c);
}

// EKF update straight from the Gram matrix in c->gram_G (k_ekf.h, "whitened by the prior"): two Cholesky-with-carry passes
// through k_ekf_chol_step — P_DD carrying P(D, :), then T = I + U1 G U1^T / sigma^2 carrying [B | U1 g / sigma^2]
static bool chol_pipe_usable(const ovgpu_ctx *c, int D) { return !c->no_chol_pipe && D <= 16 * chol::CH_TMAX && D >= 1; }
// chol::k_chol_fused on `s` with the progress words and inverse-diagonal tiles of `slot` (two factorisations may be in flight on the two
// streams); the caller has set q.D, q.LA, q.flags, what is factored and its predicates, and has seen to the slot's progress words.
// ONE launch (round 5): block 0 factors, the others carry the columns next to it (k_chol.h).  Until round 4 the carried columns were a
// kernel of their own that had to run NEXT TO the factor kernel, i.e. on a helper stream behind an event, with a second event to join
// it: each hand-over cost the stream ~6-13 us whichever side carried it (profiles/r05_c_timeline_*: 13 us between k_gram_reduce and
// the second factorisation, 14 us behind k_tf_tail).
static int chol_next_slot(ovgpu_ctx *c) { return (c->chol_slot++) & 1; }
static int launch_chol_fused(ovgpu_ctx *c, chol::CholParams &q, int slot, hipStream_t s) {
  q.prog = c->chol_prog.p + CHOL_PROG_STRIDE * slot, q.uinv = c->chol_uinv.p + (size_t)slot * 16 * 256, q.err = q.flags + 2, q.dbg = c->dbg_cycles.p;
  q.spin_limit = c->chol_spin_limit, q.n_arrive = chol::chol_tile_waves((q.D + 15) / 16);
  c->last_uinv = q.uinv;
  const int carried = (q.LA - q.D + 15) / 16;
  hipLaunchKernelGGL(with_max_lds<chol::k_chol_fused>(c), dim3(1 + (carried + chol::CH_FC - 1) / chol::CH_FC), dim3(64 * (chol::CH_FW + 1)), chol::chol_lds_bytes(), s, q);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// Beyond 256 columns, up to 512: two panels of k_chol_fused around a Schur step, four launches (k_chol_wide.h).  The work matrix is assembled
// (CH_SRC_MATRIX: reading at the source stays tied to one panel), so is only ONE factorisation in flight — the speculative prior stays off up here —
// and the panels take the two sets of step words and inverse tiles.  options.no_single_launch_cholesky and the repeat after a time-out
// (c->no_chol_pipe) select the step-wise kernels here exactly as they do below 256 columns.
static bool chol_wide_usable(const ovgpu_ctx *c, int D) { return !c->no_chol_pipe && c->chol_wide && D > chol::CW_D1 && D <= 2 * chol::CW_D1; }
static int enqueue_chol_wide(ovgpu_ctx *c, const EkfParams &p, hipStream_t s, double *Lt) {
  const int D2 = p.D - chol::CW_D1, LA2 = p.LA - chol::CW_D1;
  HIPCHK(c->chol_uinv.reserve((size_t)2 * 16 * 256));
  HIPCHK(c->chol_wide_A.reserve((size_t)D2 * LA2));
  HIPCHK(c->chol_wide_Y.reserve((size_t)D2 * LA2));
  HIPCHK(ctrl_zero(c, CTRL_PROG0, c->chol_prog.p, 16 * sizeof(int32_t), s));
  HIPCHK(ctrl_zero(c, CTRL_PROG1, c->chol_prog.p + CHOL_PROG_STRIDE, 16 * sizeof(int32_t), s));
  int32_t *go = c->ctrl.p + 4; // a spare word of the control block, written by k_chol_schur before anybody reads it
  chol::CholParams q;
  q.D = chol::CW_D1, q.LA = p.LA, q.A = p.A, q.Y = p.Y, q.Lt = nullptr, q.flags = p.flags, q.diag0 = p.diag0, q.pivot_tol = p.pivot_tol, q.pred = p.pred;
  q.src = chol::CH_SRC_MATRIX, q.pred_not = p.pred_not; // (q.N stays 0: only the read-at-source forms use it)
  int rc = launch_chol_fused(c, q, 0, s);
  if (rc != OVGPU_OK) return rc;
  chol::CholWideParams w;
  w.D = p.D, w.LA = p.LA, w.A = p.A, w.Y = p.Y, w.Ac = c->chol_wide_A.p, w.Yc = c->chol_wide_Y.p, w.Lt = Lt, w.flags = p.flags, w.go = go;
  w.pred = const_cast<int32_t *>(p.pred), w.pred_not = p.pred_not;
  const int TR = (D2 + 15) / 16, TC = (LA2 + 15) / 16;
  const int tiles = TR * TC - TR * (TR - 1) / 2; // on or right of the diagonal tile
  hipLaunchKernelGGL(chol::k_chol_schur, dim3((tiles + 3) / 4), dim3(256), 0, s, w);
  // the second panel judges every pivot against its own original diagonal entry, like the first
  q.D = D2, q.LA = LA2, q.A = c->chol_wide_A.p, q.Y = c->chol_wide_Y.p, q.diag0 = p.diag0 ? p.diag0 + chol::CW_D1 : nullptr, q.pred = go, q.pred_not = nullptr;
  if ((rc = launch_chol_fused(c, q, 1, s)) != OVGPU_OK) return rc;
  const int64_t elems = (int64_t)D2 * LA2 + (Lt ? (int64_t)p.D * p.D : 0);
  hipLaunchKernelGGL(chol::k_chol_place, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, w);
  HIPCHK(hipGetLastError());
  // The inverse tiles are two panels' own: panel 1 left tiles 0 .. 15 in slot 0, panel 2 the tiles of U22 in slot 1, which follows slot 0 in memory —
  // CW_D1 is exactly sixteen tiles, so c->chol_uinv is uinv[32][256] in tile order, what k_unwhiten_blk<32> reads (mode A beyond 383 columns).  Only
  // the prior block's factorisation (the one that wants L) says so: the second factorisation of mode B overwrites both slots, and nothing reads its tiles.
  c->last_uinv = Lt ? c->chol_uinv.p : nullptr;
  c->chol_wide_count++;
  return OVGPU_OK;
}

static int enqueue_chol_carry(ovgpu_ctx *c, const EkfParams &p, hipStream_t s, double *Lt, const CholSource &from) {
  if (chol_pipe_usable(c, p.D)) {
    // one launch: the factor workgroup's chain stays inside a compute unit, the carried columns follow through flags (k_chol.h)
    HIPCHK(c->chol_uinv.reserve((size_t)2 * 16 * 256));
    const int slot = chol_next_slot(c);
    chol::CholParams q;
    q.D = p.D, q.LA = p.LA, q.A = p.A, q.Y = p.Y, q.Lt = Lt, q.flags = p.flags, q.diag0 = p.diag0, q.pivot_tol = p.pivot_tol, q.pred = p.pred;
    q.src = from.src, q.N = p.N, q.pred_not = p.pred_not;
    if (from.src != chol::CH_SRC_MATRIX) {
      const TformParams &t = *from.t;
      q.col_cov = t.col_cov, q.P = t.P, q.G = t.G, q.LG = t.LG, q.inv_sigma2 = t.inv_sigma2, q.Y1 = t.Y1;
    }
    HIPCHK(ctrl_zero(c, slot ? CTRL_PROG1 : CTRL_PROG0, c->chol_prog.p + CHOL_PROG_STRIDE * slot, 16 * sizeof(int32_t), s));
    return launch_chol_fused(c, q, slot, s);
  }
  if (from.src != chol::CH_SRC_MATRIX) return set_err(OVGPU_ERR_INVALID, "the step-wise factorisation needs its work matrix assembled");
  if (chol_wide_usable(c, p.D)) return enqueue_chol_wide(c, p, s, Lt);
  const int TM = (p.D + 15) / 16, TL = (p.LA + 15) / 16;
  for (int kb = 0; kb < p.D; kb += 16) {
    const int tb = kb / 16;
    int jobs = TL - tb; // writers of the finished rows
    for (int it = tb + 1; it < TM; it++) jobs += TL - it;
    hipLaunchKernelGGL(k_ekf_chol_step, dim3((jobs + 3) / 4), dim3(256), 0, s, p, kb);
  }
  if (Lt) {
    TformParams t;
    t.D = p.D, t.LA = p.LA, t.Y1 = p.Y, t.Lw = Lt;
    hipLaunchKernelGGL(k_tf_lt, dim3((unsigned)((p.D * p.D + 255) / 256)), dim3(256), 0, s, t);
  }
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// part 1: P_DD = U1^T U1 carrying P(D, :), and L = U1^T for the per-feature kernel.  Depends on the prior only; side = true puts it
//         on c->stream2 behind ev_fork, ev_join marks its end (c->prior_on_side)
// part 2: everything that needs the Gram matrix in c->gram_G (c->gram_is_whitened says of which stack); part 3: both, on the context's stream
static int enqueue_ekf_gram(ovgpu_ctx *c, int part, bool side = false) {
  const int D = c->D, N = c->N, LA = D + N + 1;
  HIPCHK(c->Yaug2.reserve((size_t)D * LA));
  HIPCHK(c->gram_rho.reserve(std::max(N, D)));
  HIPCHK(c->Lw.reserve((size_t)D * (D + 8))); // (8 rows of zeros behind the last)
  if (c->Lw_D != D) { // the factorisation writes the lower triangle only
    HIPCHK(hipMemsetAsync(c->Lw.p, 0, sizeof(double) * D * (D + 8), c->stream));
    c->Lw_D = D;
  }
  EkfParams p;
  p.N = N, p.D = D, p.DC = D, p.LD = c->LD, p.LA = LA, p.tri = 1, p.pred = nullptr;
  p.R = nullptr, p.col_cov = c->col_cov.p, p.P = c->P.p, p.Mt = c->Mt.p, p.A = c->Aaug.p, p.Y = c->Yaug.p;
  p.dx = c->dx.p, p.flags = c->flags.p, p.sigma2 = c->dopt.sigma_pix_sq;
  TformParams t;
  t.N = N, t.D = D, t.LA = LA, t.LG = 16 * ((c->LD + 15) / 16), t.col_cov = c->col_cov.p, t.G = c->gram_G.p, t.P = c->P.p;
  t.A = c->Aaug.p, t.Y1 = c->Yaug.p, t.W = c->Mt.p, t.inv_sigma2 = 1.0 / c->dopt.sigma_pix_sq, t.go = c->flags.p + 3, t.diag0 = c->gram_rho.p;
  t.whitened = c->gram_is_whitened ? 1 : 0, t.Lw = c->Lw.p;
  hipStream_t s = c->stream;
  const int tm = (D + 15) / 16, tn = (N + 15) / 16;
  int rc = OVGPU_OK;
  if (part & 1) {
    if (c->prior_on_side) HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0)); // a factorisation nobody joined still owns the work matrices
    HIPCHK(ctrl_zero(c, CTRL_FLAGS, c->flags.p, 4 * sizeof(int32_t), s));
    hipStream_t sp = s;
    c->prior_on_side = false;
    if (side && part == 1) { // everything enqueued so far (the previous update's tail reads these buffers) precedes the side stream's work
      HIPCHK(hipEventRecord(c->ev_fork, s));
      HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
      sp = c->stream2;
      c->prior_on_side = true;
    }
    const int64_t elems = (int64_t)D * LA;
    const bool at_source = c->fuse_chol_inputs && chol_pipe_usable(c, D); // the factorisation gathers [P_DD | P(D, :) | 0] itself
    if (!at_source) hipLaunchKernelGGL(k_tf_gather, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, sp, t);
    p.diag0 = c->gram_rho.p, p.pivot_tol = c->prior_pivot_tol;
    CholSource from;
    if (at_source) from.src = chol::CH_SRC_PRIOR, from.t = &t;
    c->last_uinv = nullptr;
    if ((rc = enqueue_chol_carry(c, p, sp, c->Lw.p, from)) != OVGPU_OK) return rc; // Y1 = [U1 | B | 0] in c->Yaug, L = U1^T in c->Lw
    c->prior_uinv = c->last_uinv;
    p.diag0 = nullptr;
    if (c->prior_on_side) HIPCHK(hipEventRecord(c->ev_join, sp));
    c->prior_pending = true;
  }
  if (part & 2) {
    if (c->prior_on_side) HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0));
    c->prior_pending = false, c->prior_on_side = false;
    p.pred = c->flags.p + 3; // a prior block that is not positive definite: skip, the host falls back (finish_update)
    CholSource from;
    if (t.whitened && c->fuse_chol_inputs && chol_pipe_usable(c, D)) {
      // [I + G / s^2 | B | g / s^2] is read at the source by the factorisation (no k_tf_abh), everything from here on is predicated on
      // the first factorisation's flag itself, and the tail follows the carried columns' kernel on this stream
      from.src = chol::CH_SRC_WHITENED, from.t = &t;
      p.pred = nullptr, p.pred_not = c->flags.p;
    } else if (t.whitened) {
      hipLaunchKernelGGL(k_tf_abh, dim3((D + 3) / 4), dim3(256), 0, s, t, (const int32_t *)c->flags.p, c->flags.p + 3);
    } else {
      hipLaunchKernelGGL(k_tf_go, dim3(1), dim3(1), 0, s, (const int32_t *)c->flags.p, c->flags.p + 3);
      hipLaunchKernelGGL(k_tf_w, dim3((tm * tm + 3) / 4), dim3(256), 0, s, t);
      hipLaunchKernelGGL(k_tf_t, dim3((tm * tm + 3) / 4), dim3(256), 0, s, t);
      hipLaunchKernelGGL(k_tf_bh, dim3((D + 3) / 4), dim3(256), 0, s, t);
    }
    p.Y = c->Yaug2.p;
    if ((rc = enqueue_chol_carry(c, p, s, nullptr, from)) != OVGPU_OK) return rc; // Y2 = [C | C^-T B | C^-T h] in c->Yaug2
    // covariance tiles + (dx -> box-plus -> pose tables) in one launch (k_tail.h; measured on one box: 1.227 -> 1.197 ms at 2000 features,
    // 0.737 -> 0.704 ms at 800, against the four separate launches)
    TailTables tt;
    tt.C = c->C, tt.K = c->K, tt.clone_cov = c->clone_cov.p, tt.calib_cov = c->calib_cov.p, tt.intr_cov = c->intr_cov.p;
    tt.clone_qp = c->clone_qp.p, tt.calib_qp = c->calib_qp.p, tt.intr = c->intr.p, tt.clone_fej = c->clone_fej.p;
    tt.tab_clone = c->tab_clone.p, tt.tab_cam = c->tab_cam.p, tt.tab_cc = c->tab_cc.p;
    const int nb = (tn * tn + 3) / 4;
    hipLaunchKernelGGL(k_tf_tail, dim3(nb + 1), dim3(256), 0, s, p, (const double *)c->Yaug.p, tt, nb);
    if (c->lm_fast_on && c->L > 0) // ovgpu_msckf_update_lm: the resident landmarks follow dx (k_tail.h)
      hipLaunchKernelGGL(k_lm_correct, dim3((3 * c->L + 255) / 256), dim3(256), 0, s, p, c->L, (const int32_t *)c->lm_repd.p, (const int32_t *)c->lm_cov.p, c->lm_val.p);
    HIPCHK(hipGetLastError());
    c->last_update_tform = true;
    return OVGPU_OK;
  }
  return OVGPU_OK;
}

// The prior block's factorisation started by ovgpu_set_features (api_state.inc), when the resident state and the options say that the next update will
// take the Gram route: on the second stream, next to the feature upload, the batch's integer tables and the triangulation.
static int enqueue_speculative_prior(ovgpu_ctx *c) {
  if (!c->speculative_prior || c->prior_pending || !c->have_state || c->poses_only || c->D < 1) return OVGPU_OK;
  if (!(c->stream2 && c->ev_fork && c->ev_join && c->prior_overlap)) return OVGPU_OK;
  if (c->compress_gram != 1 || (c->D + 1 + 15) / 16 > gram::GR_NT_BLK || !c->whiten || !chol_pipe_usable(c, c->D)) return OVGPU_OK;
  // landmarks with columns: the batch is a SLAM call's, which would drop the factorisation and wait for it (need_prior, enqueue_pipeline_body).  Under the
  // empty active set the batch is an MSCKF update's (ovgpu_msckf_update_lm, ovgpu_msckf_update): it joins the factorisation as a landmark-free state's does
  if ((c->L != 0 && !c->lm_empty_set) || c->force_tsqr) return OVGPU_OK;
  const int rc = enqueue_ekf_gram(c, 1, true);
  if (rc != OVGPU_OK) return rc;
  // The update that follows would zero three more views of the control block one by one, each a launch of its own on its critical path (row
  // counters and the work counter between the triangulation and the Jacobian records, the step flags in front of its own factorisation: 15 us of a
  // frame, tools/gpu_frame_timeline.sh).  They are one contiguous range with the set of step flags the next factorisation takes: zeroed here, on the
  // context's stream, next to the uploads; ctrl_zero skips a view that is marked and clears its mark.
  if (c->prior_pending && c->ctrl.p) {
    const int next = c->chol_slot & 1;
    int32_t *lo = next ? c->rows_used.p : c->chol_prog.p;                                 // set 1: words 24 .. 47, set 0: words 8 .. 26
    const size_t n = next ? (size_t)(8 + 16) : (size_t)(16 + 3);
    HIPCHK(hipMemsetAsync(lo, 0, n * sizeof(int32_t), c->stream));
    c->ctrl_pre = CTRL_ROWS | CTRL_COUNTER | (next ? CTRL_PROG1 : CTRL_PROG0);
  }
  return OVGPU_OK;
}

static EventPair *next_events(ovgpu_ctx *c, std::vector<EventPair> &v, size_t idx) {
  if (idx >= v.size()) {
    if (v.size() >= 8192) return nullptr;
    v.resize(idx + 1);
  }
  EventPair &e = v[idx];
  if (!e.a) {
    if (e.a.create() != hipSuccess || e.b.create() != hipSuccess) return nullptr;
  }
  return &e;
}

enum { STAGE_LOCAL = 1, STAGE_EKF = 2 };

// factor_stays: the compressed factor is consumed on the device (EKF update, cross-GPU merge) and never shown to the caller
static int enqueue_pipeline_body(ovgpu_ctx *c, int stages, bool slam, bool factor_stays, bool gram_only);
static int enqueue_pipeline(ovgpu_ctx *c, int stages, bool slam = false, bool factor_stays = false, bool gram_only = false) {
  // one memset for the control block instead of one per flag word (unless side-stream work of an earlier call still owns part of it)
  c->ctrl_clean = 0;
  if (c->have_state && !c->prior_on_side && !c->prior_pending && c->ctrl.p) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(c->ctrl.p, 0, CTRL_INTS * sizeof(int32_t), c->stream));
    c->ctrl_clean = CTRL_FLAGS | CTRL_ROWS | CTRL_COUNTER | CTRL_PROG0 | CTRL_PROG1;
    c->ctrl_pre = 0;
  }
  const int rc = enqueue_pipeline_body(c, stages, slam, factor_stays, gram_only);
  c->ctrl_clean = 0;
  return rc;
}
static int enqueue_pipeline_body(ovgpu_ctx *c, int stages, bool slam, bool factor_stays, bool gram_only) {
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features was never called (or the state changed since)");
  HIPCHK(hipSetDevice(c->device));
  if (c->slam_rows != slam) { // the batch was laid out for the other updater
    const int rcl = set_row_layout(c, slam);
    if (rcl != OVGPU_OK) return rcl;
  }
  const Batch b = batch_of(c);
  EventPair *eu = nullptr, *ec = nullptr, *es = nullptr;
  bool tform = false;
  if (c->timing && (c->timing_period <= 1 || c->timing_seq++ % c->timing_period == 0)) {
    eu = next_events(c, c->ev_update, c->ev_used);
    ec = next_events(c, c->ev_compress, c->ev_used);
    es = next_events(c, c->ev_system, c->ev_used);
    if (eu && ec && es) c->ev_used++;
    else eu = ec = es = nullptr;
  }
  c->timed_this_update = eu != nullptr; // fill_times: an update that recorded no events reports no stage times (not an earlier update's)
  if (eu) HIPCHK(hipEventRecord(eu->a, c->stream));
  int rc = OVGPU_OK;
  // (the Gram matrix alone — the local-Gram and sharded entries — keeps the 24 tile columns of its callers' checks)
  const int tile_cap = gram_only ? gram::GR_NT_BLK : gram_route_tile_cap(c);
  const bool fits = (c->LD + 15) / 16 <= tile_cap && b.F > 0;
  tform = !gram_only && c->compress_gram == 1 && !c->force_tsqr && fits && (stages & STAGE_EKF) != 0 && (stages & STAGE_LOCAL) != 0;
  // Mode A through the Gram matrix: whitened rows -> Gram matrix -> its Cholesky factor -> un-whitened (k_unwhiten): a compressed (H, r)
  // of the reference's form at the cost of the Gram route instead of the Householder TSQR's (4.0 ms host to host at 2000 features).
  // The whitened Gram matrix is positive SEMI-definite (gauge directions, weakly observed calibration), so the factorisation decides:
  //   diagonally pivoted (k_gram_pchol, the DEFAULT and OVGPU_COMPRESS_PCHOLQR): backward stable whatever the rank — a 52-frame loop of
  //     mode A stays at 1e-13 of the oracle-driven one (the UNPIVOTED factor, rounds 3-5's OVGPU_COMPRESS_CHOLQR, drifted 6e-6 and left the tree), snapshots at dx 1e-12 / P 1e-12 (tests/test_closed_loop.py::test_mode_a_closed_loop,
  //     tests/test_gpu_parity.py::test_mode_a_pivoted_factor_shapes).
  // compress_route = OVGPU_COMPRESS_TSQR keeps the Householder triangle; so do SLAM stacks (unless ovgpu_debug_option "slam_mode_a" is in force: then
  // ovgpu_slam_compress comes here on the MSCKF entry's terms), more than 383 columns (511 under "mode_a_wide": mode_a_tile_cap), the fp32 Gram
  // variant, an un-whitened stack and a prior block whose own factorisation fails (compress_impl repeats the call then).
  const bool factor_gram = c->factor_from_gram && !gram_only && c->mode_a_factor != 0 && !c->force_tsqr && b.F > 0 && (c->LD + 15) / 16 <= mode_a_tile_cap(c) &&
                           (stages & STAGE_EKF) == 0 && (stages & STAGE_LOCAL) != 0 && c->whiten && !c->gram_fp32 && (!slam || c->slam_mode_a_on >= 1); // (SLAM stacks: Householder by default, "slam_mode_a")
  c->factor_from_gram = false, c->last_factor_from_gram = factor_gram;
  c->last_gram_kernel = c->last_factor_kernel = c->last_unwhiten_kernel = 0, c->last_gram_workgroups = 0;
  c->force_tsqr = false;
  // The prior block's factorisation needs nothing from the measurements: it runs on the second stream next to the
  // triangulation.  With the whitened stack (default) the per-feature kernel reads its factor L, so it joins before that kernel;
  // otherwise only the update itself waits for it.
  const bool need_prior = (tform || factor_gram || (gram_only && fits)) && (stages & STAGE_LOCAL) != 0;
  const bool whiten = need_prior && c->whiten;
  const bool side = need_prior && c->stream2 != nullptr && c->ev_fork != nullptr && c->ev_join != nullptr && c->prior_overlap;
  // Round 6: ovgpu_set_features starts this factorisation itself, ahead of its own uploads and of the batch's integer tables (it needs the state
  // alone: P and the column map of ovgpu_set_state) — a factorisation that is still pending here is that one (every call that changes the covariance
  // clears prior_pending), and the update only joins it.  One that this pipeline has no use for is joined and dropped: it owns the work matrices.
  if (need_prior && !c->prior_pending && (rc = enqueue_ekf_gram(c, 1, side)) != OVGPU_OK) return rc;
  if (!need_prior && c->prior_pending && (rc = drop_pending_prior(c)) != OVGPU_OK) return rc;
  if (c->layout_every_update) { // (a developer / bench switch: api_state.inc, enqueue_batch_tables) — behind the fork, where ovgpu_set_features has them
    const int rct = enqueue_batch_tables(c, true);
    if (rct != OVGPU_OK) return rct;
  }
  if (stages & STAGE_LOCAL) {
    if (c->given_tri) {
      // the gate overwrites status; restore the caller's per-feature status for this run
      if (b.F > 0) HIPCHK(hipMemcpyAsync(b.status, c->given_status.p, sizeof(int32_t) * b.F, hipMemcpyDeviceToDevice, c->stream));
    } else if ((rc = enqueue_triangulate(c)) != OVGPU_OK) return rc;
    if (es) HIPCHK(hipEventRecord(es->a, c->stream));
    c->want_stack_f32 = c->gram_fp32 && whiten && (gram_only || tform) && (c->LD + 31) / 32 <= 12;
    // Mode A factors the Gram matrix itself and un-whitens the factor by L^-1: it needs the SMALL pivots to the accuracy the projected rows give them
    // (first-order cancellation).  The unprojected stack's difference of two Gram matrices is enough for T = I + G / s^2 (the update; 500-frame loop at
    // cond(P_DD) 2-4e10: 3.5e-14 either way) and not for the factor (1.0e-8 against 3.0e-14): mode A keeps the projected stack.
    c->raw_veto = factor_gram;
    rc = enqueue_system(c, -1, 0, whiten);
    c->want_stack_f32 = false, c->raw_veto = false;
    if (rc != OVGPU_OK) return rc;
    if (es) HIPCHK(hipEventRecord(es->b, c->stream));
    if (need_prior) c->gram_is_whitened = whiten;
    if (ec) HIPCHK(hipEventRecord(ec->a, c->stream));
    if (gram_only || tform) { // Gram matrix only: summed across GPUs (sharded update) or consumed by the prior-whitened EKF update
      if ((c->LD + 15) / 16 > tile_cap)
        return set_err(OVGPU_ERR_CAPACITY, tile_cap == gram::GR_NT_WIDE ? "the Gram route holds at most 511 Jacobian columns" : "the Gram route holds at most 383 Jacobian columns");
      rc = enqueue_compress_gram(c, false);
      if (rc == OVGPU_OK && tform && (c->LD + 15) / 16 > gram::GR_NT_BLK) c->gram_wide_updates++, c->gram_wide_attempt++;
    } else if (factor_gram) {
      rc = enqueue_compress_gram(c, true); // R = pivoted chol(Gram of the whitened stack) with [R^-T g] as last column -> c->Rws
      if (rc == OVGPU_OK) {
        if (c->prior_on_side) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
        c->prior_pending = false, c->prior_on_side = false;
        // (nothing happens when the prior block's factorisation failed: flags[0]; the call is repeated through the Householder route then)
        const int NTd = (c->D + 15) / 16;
        const bool wide = NTd > gram::GR_NT_BLK || (c->LD + 15) / 16 > gram::GR_NT_BLK; // "mode_a_wide": 384 .. 511 columns, eight accumulator slots per wavefront
        // "slam_mode_a": the SLAM entry at 17 .. 24 tile columns of D (257 .. 383 columns, where a state with landmarks sits) takes the blocked form
        // as well, six accumulator slots per wavefront; ovgpu_msckf_compress keeps k_unwhiten<24> there
        // "mode_a_panel": so does ovgpu_msckf_compress
        const bool mid = !wide && NTd > 16 && ((slam && c->slam_mode_a_on >= 1) || c->mode_a_panel_on >= 1);
        bool own_tiles = false;
        if (wide || mid) {
          const double *tiles = c->unwhiten_blocked ? c->prior_uinv : nullptr;
          if (!tiles) { // the prior was factored step-wise: the diagonal tiles' inverses out of U1 itself
            HIPCHK(c->uinv_tiles.reserve((size_t)gram::GR_NT_WIDE * 256));
            hipLaunchKernelGGL(gram::k_uinv_tiles, dim3(NTd), dim3(64), 0, c->stream, c->D, (const double *)c->Yaug.p, c->D + c->N + 1, c->uinv_tiles.p, (const int32_t *)c->flags.p);
            tiles = c->uinv_tiles.p, own_tiles = true;
          }
          if (wide)
            hipLaunchKernelGGL(k_unwhiten_blk<32>, dim3(NTd), dim3(256), 0, c->stream, c->D, c->LD, c->Rws.p, (const double *)c->Yaug.p, c->D + c->N + 1, tiles,
                               (const int32_t *)nullptr, (const int32_t *)c->flags.p);
          else
            hipLaunchKernelGGL(k_unwhiten_blk<24>, dim3(NTd), dim3(256), 0, c->stream, c->D, c->LD, c->Rws.p, (const double *)c->Yaug.p, c->D + c->N + 1, tiles,
                               (const int32_t *)nullptr, (const int32_t *)c->flags.p);
          if (wide) c->mode_a_wide_compressions++;
        } else if (NTd <= 16 && c->unwhiten_blocked && c->prior_uinv)
          hipLaunchKernelGGL(k_unwhiten_blk<16>, dim3(NTd), dim3(256), 0, c->stream, c->D, c->LD, c->Rws.p, (const double *)c->Yaug.p, c->D + c->N + 1,
                             c->prior_uinv, (const int32_t *)nullptr, (const int32_t *)c->flags.p);
        else if (NTd <= 16)
          hipLaunchKernelGGL(k_unwhiten<16>, dim3(NTd), dim3(64), 0, c->stream, c->D, c->LD, c->Rws.p, (const double *)c->Yaug.p, c->D + c->N + 1,
                             (const int32_t *)nullptr, (const int32_t *)c->flags.p);
        else
          hipLaunchKernelGGL(k_unwhiten<24>, dim3(NTd), dim3(64), 0, c->stream, c->D, c->LD, c->Rws.p, (const double *)c->Yaug.p, c->D + c->N + 1,
                             (const int32_t *)nullptr, (const int32_t *)c->flags.p);
        HIPCHK(hipGetLastError());
        if (wide) c->last_unwhiten_kernel = own_tiles ? 5 : 4;
        else if (mid) c->last_unwhiten_kernel = own_tiles ? 7 : 6;
        else c->last_unwhiten_kernel = NTd > 16 ? 3 : (c->unwhiten_blocked && c->prior_uinv ? 1 : 2);
        if (slam) c->slam_mode_a_compressions++;
        if (mode_a_panel_factor(c, (c->LD + 15) / 16)) c->mode_a_panel_compressions++;
      }
    } else {
      rc = enqueue_compress(c);
    }
    if (rc != OVGPU_OK) return rc;
    if (ec) HIPCHK(hipEventRecord(ec->b, c->stream));
  }
  if (stages & STAGE_EKF) {
    if ((rc = tform ? enqueue_ekf_gram(c, 2) : enqueue_ekf(c)) != OVGPU_OK) return rc;
    c->last_route = tform ? OVGPU_COMPRESS_GRAM : OVGPU_COMPRESS_TSQR;
  }
  if (eu) HIPCHK(hipEventRecord(eu->b, c->stream));
  return OVGPU_OK;
}

// Results on their way to the caller: asynchronous copies into the page-locked landing zone, ONE synchronisation, then memcpy to the
// caller's (pageable) arrays.  Round 6: the per-feature outputs and the update's outputs (flags, dx, P') of ovgpu_msckf_update share one
// synchronisation (round 5: two — read_feature_outputs, then finish_update: ~25 us of the host-to-host time per frame): with `tail_bytes`
// read_feature_outputs only ENQUEUES its copies, reserves the zone for both and leaves the landing offsets in `pend`; finish_update, which
// synchronises anyway, lands its own copies behind them (`base`) and completes the pending per-feature outputs.
struct PendingFeatOut {
  bool active = false;
  int32_t *feat_status = nullptr;
  double *chi2 = nullptr, *chi2_thresh = nullptr, *p_FinG = nullptr;
  ovgpu_update_stats *stats = nullptr;
  size_t o_st = 0, o_c2 = 0, o_th = 0, o_pg = 0, o_gb = 0, end = 0;
};
static void unpack_feature_outputs(ovgpu_ctx *c, const PendingFeatOut &q) {
  const Batch b = batch_of(c);
  const int F = b.F;
  int32_t *feat_status = q.feat_status;
  double *chi2 = q.chi2, *chi2_thresh = q.chi2_thresh, *p_FinG = q.p_FinG;
  ovgpu_update_stats *stats = q.stats;
  std::vector<int32_t> st(F);
  if (F > 0) {
    std::memcpy(st.data(), c->down.at(q.o_st), sizeof(int32_t) * F);
    if (chi2) std::memcpy(chi2, c->down.at(q.o_c2), sizeof(double) * F);
    if (chi2_thresh) std::memcpy(chi2_thresh, c->down.at(q.o_th), sizeof(double) * F);
    if (p_FinG) std::memcpy(p_FinG, c->down.at(q.o_pg), sizeof(double) * 3 * F);
    if (stats) std::memcpy(&stats->n_gate_bound, c->down.at(q.o_gb), sizeof(int32_t));
  }
  const double qnan = std::nan("");
  int n_used = 0;
  int64_t rows = 0;
  const HostSpan<int32_t> &offs = b.h_offsets;
  for (int f = 0; f < F; f++) {
    if (st[f] == OVGPU_FEAT_USED) {
      n_used++;
      // SLAM stacks all 2m rows (2m - 2 for a single-depth landmark)
      const int ldof = (c->slam_rows && (int)b.h_feat_lm.size() == F) ? lm_dof(c->h_lm_rep[b.h_feat_lm[f]]) : 3;
      rows += 2 * (offs[f + 1] - offs[f]) - (c->slam_rows ? 3 - ldof : 3);
    }
    // the gate is only reached by features that triangulated
    if (st[f] != OVGPU_FEAT_USED && st[f] != OVGPU_FEAT_CHI2_REJECTED) {
      if (chi2) chi2[f] = qnan;
      if (chi2_thresh) chi2_thresh[f] = qnan;
    }
  }
  if (feat_status) std::memcpy(feat_status, st.data(), sizeof(int32_t) * F);
  if (stats) {
    stats->n_used = n_used;
    stats->n_rows = (int32_t)rows;
    stats->D = c->D;
    stats->n_rows_comp = rows > 0 ? c->D : 0;
  }
}
static int read_feature_outputs(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, ovgpu_update_stats *stats,
                                PendingFeatOut *pend = nullptr, size_t tail_bytes = 0) {
  const Batch b = batch_of(c);
  const int F = b.F;
  PendingFeatOut q;
  q.feat_status = feat_status, q.chi2 = chi2, q.chi2_thresh = chi2_thresh, q.p_FinG = p_FinG, q.stats = stats;
  if (F > 0) { // through the page-locked landing zone: a device-to-PAGEABLE copy is staged by the runtime, one blocking call per array
    LandLayout l;
    q.o_st = l.add(sizeof(int32_t) * F), q.o_c2 = l.add(sizeof(double) * F), q.o_th = l.add(sizeof(double) * F);
    q.o_pg = l.add(sizeof(double) * 3 * F), q.o_gb = l.add(64);
    q.end = l.end;
    HIPCHK(c->down.reserve(q.end + tail_bytes)); // (for both: finish_update's part lands behind q.end)
    HIPCHK(c->down.get(q.o_st, b.status, sizeof(int32_t) * F));
    if (stats) HIPCHK(c->down.get(q.o_gb, c->rows_used.p + 1, sizeof(int32_t)));
    if (chi2) HIPCHK(c->down.get(q.o_c2, b.chi2, sizeof(double) * F));
    if (chi2_thresh) HIPCHK(c->down.get(q.o_th, b.chi2_thr, sizeof(double) * F));
    if (p_FinG) HIPCHK(c->down.get(q.o_pg, b.pG, sizeof(double) * 3 * F));
  } else if (tail_bytes) {
    HIPCHK(c->down.reserve(tail_bytes));
  }
  if (pend) { // the caller's finish_update synchronises and completes
    q.active = true;
    *pend = q;
    return OVGPU_OK;
  }
  HIPCHK(upload_sync(c, c->stream));
  unpack_feature_outputs(c, q);
  return OVGPU_OK;
}

static void fill_times(ovgpu_ctx *c, ovgpu_update_stats *stats) {
  if (!stats || !c->timing || c->ev_used == 0 || !c->timed_this_update) return; // stats->ms_* stay 0
  float ms = 0.f;
  EventPair &eu = c->ev_update[c->ev_used - 1];
  EventPair &ec = c->ev_compress[c->ev_used - 1];
  if (hipEventElapsedTime(&ms, eu.a, eu.b) == hipSuccess) stats->ms_total = ms;
  if (hipEventElapsedTime(&ms, ec.a, ec.b) == hipSuccess) stats->ms_compress = ms;
  if (hipEventElapsedTime(&ms, eu.a, ec.a) == hipSuccess) stats->ms_system = ms; // triangulate + system
  if (hipEventElapsedTime(&ms, ec.b, eu.b) == hipSuccess) stats->ms_update = ms;
}

int ovgpu_triangulate(ovgpu_ctx *c, double *p_FinA, double *p_FinG, int32_t *anchor_meas, int32_t *status) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || !c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "state / features not set");
  HIPCHK(hipSetDevice(c->device));
  int rc = enqueue_triangulate(c);
  if (rc != OVGPU_OK) return rc;
  const Batch b = batch_of(c);
  const int F = b.F;
  hipStream_t s = c->stream;
  if (F > 0) {
    if (p_FinA) HIPCHK(hipMemcpyAsync(p_FinA, b.pA, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (p_FinG) HIPCHK(hipMemcpyAsync(p_FinG, b.pG, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (anchor_meas) HIPCHK(hipMemcpyAsync(anchor_meas, c->anchor.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, b.status, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}

int ovgpu_refine(ovgpu_ctx *c, const double *p_FinA_in, const int32_t *anchor_meas_in, double *p_FinA, double *p_FinG, int32_t *status) {
  if (!c || !p_FinA_in || !anchor_meas_in) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || !c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "state / features not set");
  HIPCHK(hipSetDevice(c->device));
  const Batch b = batch_of(c);
  const int F = b.F;
  hipStream_t s = c->stream;
  HIPCHK(c->seed_pA.reserve((size_t)3 * std::max(F, 1)));
  HIPCHK(c->seed_anchor.reserve(std::max(F, 1)));
  if (F > 0) {
    HIPCHK(upload(c->seed_pA.p, p_FinA_in, sizeof(double) * 3 * F, s));
    HIPCHK(upload(c->seed_anchor.p, anchor_meas_in, sizeof(int32_t) * F, s));
  }
  const int rc = enqueue_triangulate(c, c->seed_pA.p, c->seed_anchor.p);
  if (rc != OVGPU_OK) return rc;
  if (F > 0) {
    if (p_FinA) HIPCHK(hipMemcpyAsync(p_FinA, b.pA, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (p_FinG) HIPCHK(hipMemcpyAsync(p_FinG, b.pG, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, b.status, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}

int ovgpu_get_triangulation(ovgpu_ctx *c, double *p_FinA, double *p_FinG, int32_t *anchor_meas) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || !(c->have_feats || c->tri_readable)) return set_err(OVGPU_ERR_NO_STATE, "state / features not set");
  HIPCHK(hipSetDevice(c->device));
  const Batch b = batch_of(c);
  const int F = b.F;
  hipStream_t s = c->stream;
  if (F > 0) {
    if ((p_FinA && !b.pA) || (p_FinG && !b.pG) || (anchor_meas && !c->anchor.p)) return set_err(OVGPU_ERR_NO_STATE, "no triangulation has run on these features");
    if (p_FinA) HIPCHK(hipMemcpyAsync(p_FinA, b.pA, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (p_FinG) HIPCHK(hipMemcpyAsync(p_FinG, b.pG, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, s));
    if (anchor_meas) HIPCHK(hipMemcpyAsync(anchor_meas, c->anchor.p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}

int ovgpu_set_triangulation(ovgpu_ctx *c, const double *p_FinA, const double *p_FinG, const int32_t *anchor_meas, const int32_t *status) {
  if (!c || !p_FinG) return set_err(OVGPU_ERR_INVALID, "null argument");
  if (!c->have_state || !c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "state / features not set");
  if (c->dopt.feat_rep >= OVGPU_REP_ANCHORED_3D && (!p_FinA || !anchor_meas))
    return set_err(OVGPU_ERR_INVALID, "anchored representations need p_FinA and anchor_meas");
  HIPCHK(hipSetDevice(c->device));
  const Batch b = batch_of(c);
  const int F = b.F;
  hipStream_t s = c->stream;
  std::vector<int32_t> st(F, OVGPU_FEAT_USED);
  for (int f = 0; f < F; f++) {
    if (status) st[f] = status[f];
    if (b.h_offsets[f + 1] - b.h_offsets[f] < 2) st[f] = OVGPU_FEAT_TOO_FEW_MEAS;
    if (anchor_meas && st[f] == OVGPU_FEAT_USED && (anchor_meas[f] < b.h_offsets[f] || anchor_meas[f] >= b.h_offsets[f + 1]))
      return set_err(OVGPU_ERR_INVALID, "anchor_meas outside the feature's measurements");
  }
  HIPCHK(c->given_status.reserve(F));
  if (F > 0) {
    HIPCHK(upload(b.pG, p_FinG, sizeof(double) * 3 * F, s));
    if (p_FinA) HIPCHK(upload(b.pA, p_FinA, sizeof(double) * 3 * F, s));
    if (anchor_meas) HIPCHK(upload(c->anchor.p, anchor_meas, sizeof(int32_t) * F, s));
    HIPCHK(upload(c->given_status.p, st.data(), sizeof(int32_t) * F, s));
  }
  HIPCHK(upload_sync(c, s));
  c->given_tri = true;
  c->given_has_anchor = anchor_meas != nullptr;
  return OVGPU_OK;
}

// The pipelined merge tree bounds every wait; a node that ran into the bound (it can only happen when the nodes were not
// all resident) leaves a sticky flag behind.  Called after a stream synchronisation.
static int check_tree_error(ovgpu_ctx *c) {
  if (!c->tree_err.p) return OVGPU_OK;
  int32_t e = 0;
  HIPCHK(hipMemcpy(&e, c->tree_err.p, sizeof(e), hipMemcpyDeviceToHost));
  if (e) return set_err(OVGPU_ERR_HIP, "TSQR merge tree: a node timed out waiting for its inputs (set OVGPU_TSQR_PIPELINE=0)");
  return OVGPU_OK;
}

// The four flag words of an update (or of a chain of them) as the call's result: a follower's time-out comes first (c->chol_timed_out,
// OVGPU_ERR_HIP; stats->status is left alone), then a pivot that failed, then a negative diagonal.  The texts are the call site's own.
struct FlagText {
  std::string timed_out, not_spd, neg_diag;
};
#define CHOL_TIMED_OUT "single-launch Cholesky: a follower workgroup timed out waiting for the factor workgroup"
#define CHOL_STEPWISE_HINT " (options.no_single_launch_cholesky = 1 selects the step-wise kernels)"
static const FlagText UPDATE_FLAG_TEXT{CHOL_TIMED_OUT "; the state was not modified" CHOL_STEPWISE_HINT, "innovation covariance not SPD",
                                       "negative covariance diagonal after the update"};
static int decode_update_flags(ovgpu_ctx *c, const int32_t fl[4], ovgpu_update_stats *stats, const FlagText &where) {
  c->chol_timed_out = fl[2] != 0;
  if (fl[2]) return set_err(OVGPU_ERR_HIP, where.timed_out);
  const int status = fl[0] ? OVGPU_ERR_NOT_SPD : (fl[1] ? OVGPU_ERR_NEGATIVE_DIAGONAL : OVGPU_OK);
  if (stats) stats->status = status;
  if (status != OVGPU_OK) return set_err(status, fl[0] ? where.not_spd : where.neg_diag);
  return OVGPU_OK;
}

// with_lm: the resident landmark values land behind P' (ovgpu_msckf_update_lm)
struct UpdateLanding { // where finish_update's arrays land, behind `base`
  size_t o_fl, o_dx, o_P, o_lm, n_lm, end;
  UpdateLanding(const ovgpu_ctx *c, size_t base, bool with_lm) {
    const size_t N = (size_t)c->N;
    LandLayout l(base);
    o_fl = l.add(64), o_dx = l.add(sizeof(double) * N), o_P = l.add(sizeof(double) * N * N);
    n_lm = with_lm ? sizeof(double) * 3 * (size_t)c->L : 0, o_lm = l.add(n_lm);
    end = l.end;
  }
};
static size_t finish_update_bytes(const ovgpu_ctx *c, bool with_lm = false) { return UpdateLanding(c, 0, with_lm).end; }
static int finish_update(ovgpu_ctx *c, double *dx, double *P_out, ovgpu_update_stats *stats, const PendingFeatOut *pend = nullptr, double *lm_out = nullptr) {
  int32_t flags[4] = {0, 0, 0, 0};
  {
    const size_t N = (size_t)c->N;
    const UpdateLanding u(c, (pend && pend->active) ? pend->end : 0, lm_out && c->L > 0); // behind the per-feature outputs still in flight
    HIPCHK(c->down.reserve(u.end)); // (no-op with `pend`: read_feature_outputs reserved both zones)
    HIPCHK(c->down.get(u.o_fl, c->flags.p, sizeof(flags)));
    if (dx) HIPCHK(c->down.get(u.o_dx, c->dx.p, sizeof(double) * N));
    if (P_out) HIPCHK(c->down.get(u.o_P, c->P.p, sizeof(double) * N * N));
    if (u.n_lm) HIPCHK(c->down.get(u.o_lm, c->lm_val.p, u.n_lm));
    HIPCHK(upload_sync(c, c->stream)); // (one gather launch for everything registered, then the synchronisation)
    if (pend && pend->active) unpack_feature_outputs(c, *pend);
    std::memcpy(flags, c->down.at(u.o_fl), sizeof(flags));
    if (dx) std::memcpy(dx, c->down.at(u.o_dx), sizeof(double) * N);
    if (P_out) std::memcpy(P_out, c->down.at(u.o_P), sizeof(double) * N * N);
    if (u.n_lm) std::memcpy(lm_out, c->down.at(u.o_lm), u.n_lm);
  }
  const int status = decode_update_flags(c, flags, stats, UPDATE_FLAG_TEXT);
  if (c->chol_timed_out) return status;
  fill_times(c, stats);
  return status != OVGPU_OK ? status : check_tree_error(c);
}

// Runs `attempt` (enqueue -> read back -> finish_update) and repeats it when the failure is one that left the resident state untouched:
//  * OVGPU_ERR_NOT_SPD on the Gram-form update: that form factors the PRIOR block, which a semi-definite prior (e.g. two perfectly
//    correlated variables) fails; every kernel behind that factorisation was skipped.  Repeat through the Householder route, whose
//    S = R P R^T + sigma^2 I is positive definite for any valid covariance;
//  * a follower of the single-launch Cholesky timed out (k_chol.h: the factor workgroup was not co-scheduled; the kernels behind
//    the factorisation were switched off on the device).  Repeat with the step-wise kernels, which have no cross-workgroup wait.
extern "C++" {
// retry_timeout = false (a rank of a multi-rank update): the time-out is a scheduling event LOCAL to one rank, so a local repeat
// would issue a collective the peers never match; the error is returned instead and the caller repeats collectively.
template <class Attempt> static int update_with_fallbacks(ovgpu_ctx *c, ovgpu_update_stats *stats, Attempt attempt, bool retry_timeout = true) {
  bool tried_householder = false, tried_steps = !retry_timeout;
  const bool user_no_pipe = c->no_chol_pipe;
  int rc;
  for (;;) {
    c->chol_timed_out = false;
    c->slam_fused_attempt = 0, c->gram_wide_attempt = 0, c->feat_class_attempt = 0;
    rc = attempt();
    if (rc == OVGPU_ERR_NOT_SPD && c->last_update_tform && !c->chol_timed_out && !tried_householder) {
      tried_householder = true, c->force_tsqr = true;
    } else if (c->chol_timed_out && !tried_steps) {
      tried_steps = true, c->no_chol_pipe = true, c->chol_timeouts++;
    } else {
      break;
    }
    c->slam_fused_batches -= c->slam_fused_attempt; // the attempt does not stand: "slam_fused_batches" counts the pipelines of the attempt that is the update
    c->gram_wide_updates -= c->gram_wide_attempt;   // ... and "gram_wide_updates" the update itself
    c->feat_class_batches -= c->feat_class_attempt; // ... and "feat_class_batches" as "slam_fused_batches"
    if (stats) std::memset(stats, 0, sizeof(*stats));
  }
  if (rc != OVGPU_OK) c->gram_wide_updates -= c->gram_wide_attempt; // an update that ends in an error does not stand either
  c->gram_wide_attempt = 0;
  c->no_chol_pipe = user_no_pipe;
  return rc;
}
} // extern "C++"

int ovgpu_msckf_update(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out,
                       ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return update_with_fallbacks(c, stats, [&]() {
    int rc = enqueue_pipeline(c, STAGE_LOCAL | STAGE_EKF);
    if (rc != OVGPU_OK) return rc;
    PendingFeatOut pend; // one synchronisation for the per-feature outputs and dx / P'
    if ((rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, stats, &pend, finish_update_bytes(c))) != OVGPU_OK) return rc;
    return finish_update(c, dx, P_out, stats, &pend);
  });
}

// UpdaterMSCKF::update on a state whose SLAM landmarks stay resident and current (include/ovgpu.h).  The landmarks have no column under the empty
// active set, so the batch, the column map and every kernel are a landmark-free state's of the same N (enqueue_system, set_row_layout); k_lm_correct
// (k_tail.h) follows the tail on the same predicates, and the corrected values come back with dx and P'.
int ovgpu_msckf_update_lm(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out, double *lm_out,
                          ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  // every check in front of the first launch: a refused call leaves the state, the landmarks and the resident batch as they were
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  if (!c->have_feats) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_features was never called (or the state changed since)");
  if (c->L > 0 && !c->lm_empty_set)
    return set_err(OVGPU_ERR_INVALID, "ovgpu_msckf_update_lm: the batch was laid out with landmark columns; call ovgpu_set_active_landmarks(ctx, NULL, 0) after "
                                      "ovgpu_set_landmarks and hand the MSCKF batch to ovgpu_set_features again");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const bool with_lm = lm_out != nullptr && c->L > 0;
  c->lm_fast_on = c->L > 0;
  const int rc = update_with_fallbacks(c, stats, [&]() {
    int rc2 = enqueue_pipeline(c, STAGE_LOCAL | STAGE_EKF);
    if (rc2 != OVGPU_OK) return rc2;
    PendingFeatOut pend; // one synchronisation for the per-feature outputs, dx / P' and the landmarks
    if ((rc2 = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, stats, &pend, finish_update_bytes(c, with_lm))) != OVGPU_OK) return rc2;
    return finish_update(c, dx, P_out, stats, &pend, with_lm ? lm_out : nullptr);
  });
  c->lm_fast_on = false;
  return rc;
}

int ovgpu_msckf_update_async(ovgpu_ctx *c) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  c->async_pending = true;
  return enqueue_pipeline(c, STAGE_LOCAL | STAGE_EKF);
}

static int compress_impl(ovgpu_ctx *c, bool slam, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, int32_t *D_out,
                         int32_t *rows_out, int32_t *col_cov_id, double *H, double *r, ovgpu_update_stats *stats) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  ovgpu_update_stats local;
  int rc;
  const double *tri = nullptr;
  int32_t dropped = 0;
  const int64_t wide0 = c->mode_a_wide_compressions, slam0 = c->slam_mode_a_compressions, fused0 = c->slam_fused_batches, panel0 = c->mode_a_panel_compressions, classes0 = c->feat_class_batches;
  for (int attempt = 0;; attempt++) {
    c->factor_from_gram = attempt == 0; // the whitened Gram matrix's factor (pivoted by default) where it applies; Householder TSQR otherwise
    if ((rc = enqueue_pipeline(c, STAGE_LOCAL, slam)) != OVGPU_OK) return rc;
    // The compressed system, the factorisation flags and the pivoted factor's rank follow the pipeline on its stream into page-locked
    // staging and arrive with the synchronisation of read_feature_outputs (three blocking copies from pageable memory cost 60 us).
    const size_t n_tri = (size_t)c->D * c->LD;
    HIPCHK(c->h_tri.reserve(n_tri + 4));
    int32_t *h_words = reinterpret_cast<int32_t *>(c->h_tri.p + n_tri); // [0..3] flags, [4] dropped rows
    std::memset(h_words, 0, 8 * sizeof(int32_t));
    if (n_tri > 0) HIPCHK(hipMemcpyAsync(c->h_tri.p, c->Rws.p, sizeof(double) * n_tri, hipMemcpyDeviceToHost, c->stream));
    if (c->last_factor_from_gram) {
      HIPCHK(hipMemcpyAsync(h_words, c->flags.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(h_words + 4, c->gram_dropped.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    std::memset(&local, 0, sizeof(local));
    if ((rc = read_feature_outputs(c, feat_status, chi2, chi2_thresh, p_FinG, &local)) != OVGPU_OK) return rc;
    tri = c->h_tri.p, dropped = h_words[4];
    if (!c->last_factor_from_gram) break;
    if (!h_words[0] && !h_words[2]) break;
    // the prior block is not (numerically) positive definite, or its single-launch factorisation was not co-scheduled: the whitened
    // route has nothing to offer; repeat through the Householder TSQR on the raw rows (which needs no factor of the prior)
    c->force_tsqr = true;
    c->mode_a_wide_compressions = wide0, c->slam_mode_a_compressions = slam0, c->slam_fused_batches = fused0, c->mode_a_panel_compressions = panel0, c->feat_class_batches = classes0; // (the attempt does not stand)
    if (attempt > 0) return set_err(OVGPU_ERR_NOT_SPD, "prior block of the involved variables not positive definite");
  }
  const int D = c->D, LD = c->LD;
  int rows = local.n_rows > 0 ? D : 0;
  if (rows > 0 && c->last_factor_from_gram) rows = std::max(0, D - dropped); // the pivoted factor stops at the numerical rank: its zero rows stay behind
  if (H)
    for (int i = 0; i < rows; i++) std::memcpy(H + (size_t)i * D, tri + (size_t)i * LD, sizeof(double) * D);
  if (r)
    for (int i = 0; i < rows; i++) r[i] = tri[(size_t)i * LD + D];
  if (col_cov_id) std::memcpy(col_cov_id, c->h_col_cov.data(), sizeof(int32_t) * D);
  if (D_out) *D_out = D;
  if (rows_out) *rows_out = rows;
  c->last_route = c->last_factor_from_gram ? OVGPU_COMPRESS_PCHOLQR : OVGPU_COMPRESS_TSQR;
  local.n_rows_comp = rows;
  fill_times(c, &local);
  if (stats) *stats = local;
  return check_tree_error(c);
}

int ovgpu_msckf_compress(ovgpu_ctx *c, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, int32_t *D_out, int32_t *rows_out,
                         int32_t *col_cov_id, double *H, double *r, ovgpu_update_stats *stats) {
  return compress_impl(c, false, feat_status, chi2, chi2_thresh, p_FinG, D_out, rows_out, col_cov_id, H, r, stats);
}

int ovgpu_get_state(ovgpu_ctx *c, double *P, double *clone_q_p, double *calib_q_p, double *intrinsics) {
  if (!c) return set_err(OVGPU_ERR_INVALID, "null ctx");
  if (!c->have_state || c->poses_only) return set_err(OVGPU_ERR_NO_STATE, "ovgpu_set_state was never called");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (P) HIPCHK(hipMemcpyAsync(P, c->P.p, sizeof(double) * c->N * c->N, hipMemcpyDeviceToHost, s));
  if (clone_q_p) HIPCHK(hipMemcpyAsync(clone_q_p, c->clone_qp.p, sizeof(double) * 7 * c->C, hipMemcpyDeviceToHost, s));
  if (calib_q_p) HIPCHK(hipMemcpyAsync(calib_q_p, c->calib_qp.p, sizeof(double) * 7 * c->K, hipMemcpyDeviceToHost, s));
  if (intrinsics) HIPCHK(hipMemcpyAsync(intrinsics, c->intr.p, sizeof(double) * 8 * c->K, hipMemcpyDeviceToHost, s));
  HIPCHK(upload_sync(c, s));
  return OVGPU_OK;
}
