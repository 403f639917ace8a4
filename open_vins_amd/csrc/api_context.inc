// api_context.inc — part of ovgpu_api.hip (ONE translation unit, included in order; not a stand-alone header): the context (ovgpu_ctx: device buffers, route switches, events), error plumbing, page-locked staging, launch helpers shared by every entry point.
using namespace ovg;

static thread_local std::string g_err = "";
static int set_err(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess) {                                                                                  \
      return set_err(OVGPU_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(_e) + " (" __FILE__ ":" + \
                                        std::to_string(__LINE__) + ")");                                     \
    }                                                                                                        \
  } while (0)

namespace {

// The two allocation policies of OwnedBuf (dev_buf.h).  Each counts what it has handed out and not taken back, process-wide: allocations and
// bytes as requested (ovgpu_debug_option "live_allocations" / "live_allocation_bytes" report the sums).
struct AllocCount {
  std::atomic<int64_t> n{0}, bytes{0};
  void add(size_t b) { n.fetch_add(1, std::memory_order_relaxed), bytes.fetch_add((int64_t)b, std::memory_order_relaxed); }
  void sub(size_t b) { n.fetch_sub(1, std::memory_order_relaxed), bytes.fetch_sub((int64_t)b, std::memory_order_relaxed); }
};
struct DeviceAlloc {
  using Err = hipError_t;
  static constexpr Err ok = hipSuccess;
  static inline AllocCount live;
  static Err alloc(void **p, size_t bytes) {
    const Err e = hipMalloc(p, bytes);
    if (e == hipSuccess) live.add(bytes);
    return e;
  }
  static void free(void *p, size_t bytes) { (void)hipFree(p), live.sub(bytes); }
  static Err copy(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice); }
};
// page-locked host staging (read-backs that complete with the stream's next synchronisation instead of one blocking copy each)
struct PinnedAlloc {
  using Err = hipError_t;
  static constexpr Err ok = hipSuccess;
  static inline AllocCount live;
  static Err alloc(void **p, size_t bytes) {
    const Err e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) live.add(bytes);
    return e;
  }
  static void free(void *p, size_t bytes) { (void)hipHostFree(p), live.sub(bytes); }
};
template <class T> using DevBuf = OwnedBuf<T, DeviceAlloc>;
template <class T> using PinBuf = OwnedBuf<T, PinnedAlloc>;

// Owning handles of an event and of a stream: empty until create(), destroyed with their owner, read as the plain handle.
struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  ~Event() { if (h) (void)hipEventDestroy(h); }
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  Event(Event &&o) noexcept : h(o.h) { o.h = nullptr; } // (the vectors of stage timers grow)
  hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&h, flags); }
  operator hipEvent_t() const { return h; }
};
struct Stream {
  hipStream_t h = nullptr;
  Stream() = default;
  ~Stream() { if (h) (void)hipStreamDestroy(h); }
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  operator hipStream_t() const { return h; }
};

// a window into another buffer's allocation (the words of the control block): nothing to reserve, grow or release
template <class T>
struct DevView {
  T *p = nullptr;
};

// a host array somebody else owns
template <class T>
struct HostSpan {
  const T *p = nullptr;
  size_t n = 0;
  const T &operator[](size_t i) const { return p[i]; }
  size_t size() const { return n; }
};
template <class T>
static HostSpan<T> span_of(const std::vector<T> &v) { return HostSpan<T>{v.data(), v.size()}; }

// What a pipeline stage runs on: the resident feature batch, or a slice of it (a chunk of ovgpu_slam_update_chunked).  A value that owns
// nothing: the context's DevBufs and vectors own the arrays, batch_of() composes this from them at the moment of the call, and a stage reads
// every one of these fields from the Batch it took at its top, never from the context.
struct Batch {
  int F = 0, M = 0, m_max = 0;
  int64_t rows_total = 0;
  HostSpan<int32_t> h_offsets, h_order, h_feat_lm; // meas_offsets, sys_order and the lm_index the batch was handed, on the host
  HostSpan<int64_t> h_row_off;
  bool have_sigma = false, have_mult = false;
  int32_t *meas_offsets = nullptr, *sys_order = nullptr, *status = nullptr;
  uint16_t *meas_cc = nullptr;
  float *uv = nullptr, *uvn = nullptr;
  int64_t *row_off = nullptr;
  double *pA = nullptr, *pG = nullptr, *chi2 = nullptr, *chi2_thr = nullptr, *feat_sigma = nullptr, *feat_mult = nullptr;
};

struct EventPair {
  Event a, b;
};

} // namespace

enum { CTRL_FLAGS = 1, CTRL_ROWS = 2, CTRL_COUNTER = 4, CTRL_PROG0 = 8, CTRL_PROG1 = 16, CTRL_INTS = 64, CHOL_PROG_STRIDE = 24 };

// The per-feature kernels.  The values are the codes ovgpu_debug_option "last_feature_kernel" reports (include/ovgpu.h): this is their one list.
enum FeatKernel : int {
  FK_GENERAL = 0,         // k_system_t (k_system.h): every batch can end up here
  FK_FEATY_4 = 1,         // k_feat_y<4, 9> (k_featy.h), the MSCKF fast path's one-pass kernel
  FK_FEATY_8 = 2,         // k_feat_y<8, 17>
  FK_FEATY_BIG = 3,       // k_feat_y_big (k_featy_big.h): gate matrices beyond a compute unit's registers, block row by block row
  FK_SLAMY = 4,           // k_slam_y<false> (k_slam_y.h): SLAM batches under ovgpu_debug_option "slam_fused"
  FK_SLAMY_PROJ = 5,      // k_slam_y<true>: with the projection of single-depth landmarks
  FK_SLAMY_LONG = 6,      // the long shapes of the two: 63 .. 126 observations ("slam_fused" = 3)
  FK_SLAMY_LONG_PROJ = 7,
  FK_SLAMY_BIG = 8,       // k_slam_y_big<false> (k_slam_y_big.h): 127 .. 232 observations, block row by block row ("slam_fused_big")
  FK_SLAMY_BIG_PROJ = 9,  // k_slam_y_big<true>
};

// What the batch in force and the switches at layout time determine about the per-feature stage: a value, made by plan_feature_stage
// (api_state.inc) and kept as c->plan; enqueue_system's selector (api_pipeline.inc) picks the launch from it and the launch-time switches.
struct FeatPlan {
  // the general kernel's carve (k_system.h) — always filled in: a single feature (f_one >= 0), the routes without L and per-feature sigma on an
  // MSCKF batch end up there whatever else the batch was laid out for
  bool rows_global = false;   // k_system_t<true>: the longest track's Jacobian records do not fit LDS and live in c->sys_rows_ws
  int m_lds_max = 0;          // the longest track whose gate matrix is LDS-resident; longer ones keep theirs in c->gate_ws
  size_t sys_lds = 0;         // its dynamic LDS bytes
  int sys_grid = 1;
  int64_t gate_ws_stride = 0; // doubles per workgroup of c->gate_ws; 0: no track needs it
  // the fused kernel of the MSCKF fast path the batch was laid out for (FK_FEATY_4 / _8 / _BIG), or FK_GENERAL: none
  FeatKernel msckf = FK_GENERAL;
  int nt = 0, nta = 0;        // tile rows of the longest track (2 m rows) and of its gate matrix (2 m + 4 rows)
  int nw() const { return msckf == FK_FEATY_4 ? 4 : 8; } // wavefronts per workgroup
  bool lm_fast_ok = false;    // ... with landmarks resident under the empty active set: ovgpu_msckf_update_lm may take it (lm_fast_on)
  // the fused kernel a SLAM batch was laid out for (FK_SLAMY ..), or FK_GENERAL: none — and its LDS bytes
  FeatKernel slam = FK_GENERAL;
  size_t slam_lds = 0;
  int slam_nt = 0;            // FK_SLAMY_BIG / _PROJ: tile rows of the longest track, the carve's and the scratch's parameter
  // ovgpu_debug_option "feat_classes" = 1: the length classes of an MSCKF batch (feat_classes.h), longest first — a kernel each over its own slot
  // range.  n_classes >= 2 or none at all: a batch of one class is the single-kernel rule's.  Then `msckf`, `nt` and `nta` above describe the
  // longest FUSED track (the stride of the instance lists, k_feat_vt's block) and a general class, if there is one, is cls[0].
  struct Class {
    FeatKernel kernel = FK_GENERAL;
    int begin = 0, end = 0;   // slots of b.h_order
    int m_max = 0;            // the class's longest track, and the carve it sizes:
    int nt = 0, nta = 0;      // tile rows as above (fused classes)
    size_t lds = 0;           // dynamic LDS bytes
    int grid = 1;
  };
  int n_classes = 0;
  Class cls[4];
  int m_fused = 0;            // the longest track of a fused class
  bool cls_general() const { return n_classes > 0 && cls[0].kernel == FK_GENERAL; }
  bool cls_mixed_width() const { return n_classes > 0 && msckf == FK_FEATY_BIG && cls[n_classes - 1].kernel != FK_FEATY_BIG; } // instance lists at both block widths
  const char *error = nullptr; // no kernel holds the batch's longest track (OVGPU_ERR_CAPACITY)
};

struct LoopComm;
// ---- the page-locked arena and landing zone (host_link.h): their two kernels and the HIP port -----------------------------------------
__global__ void __launch_bounds__(256) k_upload_scatter(const unsigned char *__restrict__ arena, UpBatch b) {
  const UpSeg sg = b.seg[blockIdx.y];
  const unsigned char *src = arena + sg.off;
  unsigned char *dst = static_cast<unsigned char *>(sg.dst);
  const uint32_t nvec = ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) ? sg.bytes >> 4 : 0;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src);
  u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) d4[i] = __builtin_nontemporal_load(s4 + i);
  for (uint32_t i = (nvec << 4) + blockIdx.x * 256 + threadIdx.x; i < sg.bytes; i += gridDim.x * 256) dst[i] = src[i];
}

// the HIP port of Uplink / Landing (host_link.h): everything on the stream the context hands them
struct HipLink {
  using Err = hipError_t;
  static constexpr Err ok = hipSuccess, refused = hipErrorInvalidValue;
  using Stream = hipStream_t;
  using Pinned = PinnedAlloc;
  static unsigned char *device_alias(unsigned char *host) { // (page-locked host memory is mapped into the device's address space)
    void *dev = nullptr;
    return hipHostGetDevicePointer(&dev, host, 0) == hipSuccess ? static_cast<unsigned char *>(dev) : nullptr;
  }
  static Err h2d(Stream s, void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); }
  static Err d2h(Stream s, void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); }
  static Err scatter(Stream s, const unsigned char *arena, const UpBatch &b) {
    hipLaunchKernelGGL(k_upload_scatter, dim3(UP_BLOCKS, b.n), dim3(256), 0, s, arena, b);
    return hipGetLastError();
  }
  static Err gather(Stream s, unsigned char *zone, const UpBatch &b); // (behind k_download_gather, below)
  static Err sync(Stream s) { return hipStreamSynchronize(s); }
};

struct ovgpu_ctx {
  int device = 0;
  Stream stream;
  ovgpu_options opts{};
  DevOptions dopt{};
  int lds_limit = 160 * 1024;
  int num_cu = 256;

  // ---- state
  bool have_state = false;
  bool poses_only = false; // ovgpu_set_camera_poses: only the FeatureInitializer entry points are usable
  int N = 0, C = 0, K = 0, D = 0, LD = 0;
  DevBuf<double> P, P0, clone_qp, clone_qp0, clone_fej, calib_qp, calib_qp0, intr, intr0;
  DevBuf<uint8_t> fisheye;
  DevBuf<int32_t> clone_cov, calib_cov, intr_cov, clone_col, calib_col, intr_col, col_cov;
  DevBuf<uint8_t> col_kind, col_sub;
  DevBuf<uint16_t> col_var;
  DevBuf<double> tab_clone, tab_cam, tab_cc;
  std::vector<int32_t> h_col_cov;
  struct HVar { int cov, size, kind, index; };
  std::vector<HVar> h_vars; // clones + calibrated camera variables of the resident state (landmarks are merged in by build_columns)
  std::vector<int32_t> h_clone_cov, h_calib_cov, h_intr_cov; // covariance ids as the kernels see them (-1: not estimated)
  DevBuf<double> prop_w, prop_in; // EKFPropagation workspaces
  DevBuf<int32_t> prop_ids;
  // the batched anchor change (k_anchor_change_all, k_cov_propagate_multi): entry table | gmap | rowg, the ragged ids, Phi | value | fej, W | G
  DevBuf<int32_t> anc_tab, anc_ids;
  DevBuf<double> anc_phi, anc_w;
  std::vector<int32_t> h_anc_tab; // the table's host source (outlives the call that uploads it)
  // ovgpu_state_marginalize_batched (k_marg_plan, k_cov_remove_many, k_records_compact): blocks | clone flags | landmark flags from the host, the index
  // lists behind them; the record arrays' second buffers (each swaps with its array, as Ppad does with P)
  DevBuf<int32_t> marg_tab, lm_anchor_b, lm_repd_b;
  DevBuf<double> clone_qp_b, clone_fej_b, lm_val_b, lm_fej_b;
  // ovgpu_slam_update_chunked (k_slam_chunks.h): the call's integer table (chunk_first | every chunk's sorted column set | lm_index | every chunk's
  // feature order) and row offsets from the host, the rebased meas_offsets the device writes, the per-chunk results (dx rows, flag words | gate
  // counters) and the entry state kept aside for the restore-and-chain path
  DevBuf<int32_t> chk_tab, chk_offs, chk_flags;
  DevBuf<int64_t> chk_rowoff;
  DevBuf<double> chk_dx, chk_save;
  int chunk_fail_inject = -1;   // ovgpu_debug_option "slam_chunked_fail_chunk": this chunk's flag word reads as failed after the pass (one-shot; tests of the restore-and-chain path)
  int64_t chunk_fallbacks = 0;  // ovgpu_debug_option "slam_chunked_fallbacks": how often ovgpu_slam_update_chunked put the entry state back and ran the chain
  int init_fused = 1;           // ovgpu_debug_option "delayed_init_fused", a level.  0: ovgpu_slam_delayed_init_fused runs the chain's step for every candidate;
                                // 1: the fused step behind k_system_t's gate; 2: the fused step behind k_init_rows, the gate taken from the step's own factorisation
  int64_t init_fused_steps = 0, init_chain_steps = 0; // "delayed_init_fused_steps" / "delayed_init_chain_steps": candidates of ovgpu_slam_delayed_init_fused by the step they took
  int64_t init_rows_steps = 0;  // "delayed_init_rows_steps": those of the fused steps that ran at level 2
  int init_fused_long = 0;      // ovgpu_debug_option "delayed_init_fused_long".  1: the fused step holds tracks of up to INITF_M_MAX_LONG = 232 measurements (k_init_fused.h); 0: of up to 64
  int64_t init_long_steps = 0;  // "delayed_init_long_steps": those of the fused steps whose candidate held more than 64 measurements
  // SLAM landmarks (ovgpu_set_landmarks); L > 0 switches the per-feature kernel to the UpdaterSLAM rules
  int L = 0;
  // the resident landmarks' representations, one each (Landmark::_feat_representation: StateOptions::feat_rep_slam, or feat_rep_aruco for
  // ArUco corners; one for all before round 5), mirror of lm_repd
  std::vector<int32_t> h_lm_rep;
  std::vector<int32_t> h_feat_lm;  // lm_index of the batch the last ovgpu_slam_update / _compress was handed (row counts of a mixed-dof batch)
  std::vector<int32_t> h_feat_rep; // ovgpu_set_feature_reps: the representation each feature of the batch is initialised in (empty: the call's feat_rep)
  std::vector<int32_t> h_lm_cov, h_lm_col, h_lm_anchor; // h_lm_anchor: packed (camera << 10 | clone) or -1, mirror of lm_anchor
  DevBuf<double> pFej, lm_val, lm_fej; // landmark values in representation coordinates (ov_type::Landmark::value / fej)
  DevBuf<int32_t> feat_lm, feat_lmcol, feat_lmcov, feat_anchor, lm_cov, lm_col, lm_anchor, lm_repd, lm_index;
  // ovgpu_set_active_landmarks: the landmarks that get Jacobian columns in the calls that follow (UpdaterSLAM.cpp:300-340 builds Hx_order from
  // what the batch touches); without one every resident landmark has a column block
  bool active_given = false;
  std::vector<uint8_t> h_lm_active;  // [L] 1: named by the active set
  std::vector<HVar> h_sorted;        // h_vars and the resident landmarks by covariance id (build_columns); layout_columns walks it, no sort per call
  DevBuf<int32_t> var_tab, active_idx; // device copy of h_sorted (4 ints per variable) and the uploaded lm_index of the set: k_active_columns' inputs
  bool var_tab_ok = false;           // var_tab holds h_sorted
  bool cols_over = false;            // the column set asked for has more than 511 columns: no landmark has a column and the SLAM entry points refuse
  std::string cols_over_msg;
  bool slam_rows = false; // row layout of the uploaded batch: 2m rows per feature (SLAM update) or 2m - 3 (MSCKF, delayed init)
  // ovgpu_msckf_update_lm: resident landmarks that have NO column (the empty active set) are extra rows of P, as the IMU block is — the column map
  // is a landmark-free state's and so is every kernel of the MSCKF update
  bool lm_empty_set = false;      // L > 0 and ovgpu_set_active_landmarks(ctx, NULL, 0) holds (layout_columns)
  FeatPlan plan;                  // the per-feature stage of the batch in force (size_feature_stage)
  FeatKernel last_feat_kernel{FK_GENERAL}; // ovgpu_debug_option "last_feature_kernel": what the last batch pipeline was laid out for and ran
  bool anchored_fast = true;      // ovgpu_debug_option "anchored_fast": batches of an anchored feat_rep_msckf are laid out for the fused per-feature kernels too (set_row_layout)
  bool lm_fast_on = false;        // ovgpu_msckf_update_lm is running: the one entry that takes them with landmarks resident (enqueue_system)
  // the fused per-feature kernel of UpdaterSLAM::update (k_slam_y.h), behind a switch that is off by default
  int slam_fused = 0;             // ovgpu_debug_option "slam_fused", a level: 0 off; 1 SLAM batches whose observed landmarks are all 3-dof are laid out for k_slam_y<false>; 2 also the ones that observe a single-depth landmark, for k_slam_y<true>; 3 also the batches whose longest track holds 63 .. 126 observations, for the long shapes (plan_feature_stage)
  int slam_fused_big = 0;         // ovgpu_debug_option "slam_fused_big", a level: 0 off; 1 (and above) under "slam_fused" = 3 a batch whose longest track holds 127 .. 232 observations (slamy::SLY_MMAX_B) is laid out for the block-row shapes k_slam_y_big (plan_feature_stage)
  int64_t slam_fused_batches = 0; // ovgpu_debug_option "slam_fused_batches": pipelines that took k_slam_y, counted once per update: the pipelines of an attempt that update_with_fallbacks repeats (Householder route, step-wise Cholesky) are taken off again
  int slam_fused_attempt = 0;     // ... of them, the ones of the update attempt that is running (update_with_fallbacks)
  // device-resident FeatureDatabase (ovgpu_tracks_*)
  int trk_max = 0, trk_obs = 0;
  int trk_group_order = OVGPU_GROUPS_REFERENCE; // camera groups of an assembled batch (k_tracks.h, ovgpu_tracks_group_order)
  std::vector<std::vector<int8_t>> trk_h_cams;  // per slot: the cameras in order of FIRST insertion (what an unordered_map remembers)
  DevBuf<int8_t> trk_order;
  DevBuf<int32_t> trk_count, trk_cam, trk_slot_in, trk_cam_in, trk_sel, trk_nvalid, trk_flag;
  DevBuf<double> trk_time, trk_clone_times, trk_aux;
  DevBuf<float> trk_uv, trk_uvn, trk_uv_in, trk_uvn_in;
  std::unordered_map<int64_t, int32_t> trk_slot_of;
  // ovgpu_retriangulate: the running linear systems of the active tracks, two generations (k_retri.h)
  std::unordered_map<int64_t, int32_t> retri_slot_of;
  DevBuf<double> retri_sys[2], retri_pos, retri_uvd;
  DevBuf<int32_t> retri_int, marg_idx, seed_anchor;
  DevBuf<double> marg_out, seed_pA;
  DevBuf<float> retri_f;
  int retri_gen = 0;
  std::vector<int32_t> trk_free, trk_h_count;
  std::vector<int64_t> trk_h_id;
  // UpdaterSLAM::delayed_init
  DevBuf<double> Ppad, init_ws, dx_seq;
  DevBuf<int32_t> init_ctr, feat_slot;
  // ovgpu_slam_init_systems: the chain runs on scratch copies and exports every feature's system (k_init_export)
  bool init_export = false;         // the chain in flight is the speculative one: rejected features keep their rows
  DevBuf<double> isx_arena, isx_save; // exported H_x | H_f | res of all features; the values the chain moves (clones, calibration, landmarks)
  DevBuf<int32_t> isx_cols;         // per feature: the context's column of every H_x column, in Hx_order
  std::vector<int32_t> h_isx_cols;

  // ---- features: the resident batch's owners.  Stages read them through batch_of()
  const Batch *view = nullptr; // the batch in force when it is not the whole resident one (BatchScope: a chunk of ovgpu_slam_update_chunked)
  bool have_feats = false;
  bool tri_readable = false; // ovgpu_slam_delayed_init ended: the column map changed, so its batch cannot feed another update (have_feats = false),
                             // but what its triangulation stage left (pA / pG / anchor of the same F features) is still what ovgpu_get_triangulation documents
  bool given_tri = false; // positions supplied by ovgpu_set_triangulation
  bool given_has_anchor = false; // ... together with the anchor measurements
  std::vector<int32_t> h_given_status;
  DevBuf<int32_t> given_status;
  int F = 0, M = 0, m_max = 0;
  int64_t rows_total = 0;
  DevBuf<int32_t> meas_offsets;
  DevBuf<uint16_t> meas_cc;
  DevBuf<float> uv, uvn;
  DevBuf<int64_t> row_off;
  DevBuf<double> pA, pG, chi2, chi2_thr;
  int layout_every_update = 0; // ovgpu_debug_option "layout_every_update": the per-batch integer tables (enqueue_batch_tables) are built again at the head of every update
  int inst_cb = 0, inst_D = 0; // the column-block width / column count the batch's instance lists (fs_inst, k_batch_layout) were built for; 0 = not built
  DevBuf<int32_t> anchor_pre; // per feature: the anchor measurement by the reference's rule, found when the batch is laid out (k_batch_layout)
  DevBuf<int32_t> anchor, status, sys_order; // sys_order: feature indices by descending track length
  DevBuf<double> feat_sigma, feat_mult;      // per-feature noise / gate multiplier (ovgpu_set_feature_options)
  bool have_feat_sigma = false, have_feat_mult = false;
  DevBuf<double> chi2_table;
  int chi2_table_len = 0;
  std::vector<double> h_chi2_table;
  std::vector<int32_t> h_offsets;
  std::vector<int64_t> h_row_off;

  // ---- workspaces
  DevBuf<double> Hbig, gate_ws, Rws, Mt, Aaug, Yaug, dx;
  DevView<int32_t> flags;
  int W = 1;
  int64_t rows_per_node = 128;
  // read-only ovgpu_debug_option names "tsqr_leaves", "tsqr_rows_per_node", "tsqr_last_leaf_kernel", "tsqr_last_tree", "tsqr_last_qh": what the last
  // Householder compression (stand-alone or on the update route) launched, kept on the host by enqueue_compress / enqueue_merge_tree
  int tsqr_last_W = 0;            // leaves
  int64_t tsqr_last_rpn = 0;      // rows per leaf
  int tsqr_last_leaf = -1;        // 0 pw::k_qr_node (k_tsqr_pw.h), 1 k_qr_node<.., false> (k_tsqr.h), 2 k_qr_append (k_compress.h); -1: none yet
  int tsqr_last_tree = 0;         // 0 no merge, 1 k_qr_tree next to the leaves, 2 k_qr_tree behind them, 3 one launch per level
  int tsqr_last_qh = 0;           // quads per register array of the merge kernels (16 / 28 / 32); 0: k_qr_append, or no merge
  DevBuf<QrTreeNode> tree_nodes, tree_nodes2; // merge trees of the pipelined launch, cached per leaf count (two: the local
                                              // compression and the cross-GPU merge alternate in the sharded update)
  int tree_G2 = 0;
  // leaf / tree overlap: the merge tree runs on a second stream next to the leaf kernel's last append
  Stream stream2; // (round 5: the single-launch Cholesky's carried columns are blocks of the same launch — the helper stream and the events around it are gone)
  Event ev_rows;
  bool gram_il = true;              // ovgpu_debug_option "gram_interleaved": k_gram_il (staging between the matrix instructions) instead of k_gram
  bool gram_blocks_only = false;    // ovgpu_debug_option "gram_blocks_only": the block variant (k_gram_blk) also where k_gram_wide applies
  bool fuse_chol_inputs = true;     // ovgpu_debug_option "fuse_chol_inputs": the factorisations read their inputs at the source (no k_tf_gather / k_tf_abh)
  Event ev_fork, ev_join;
  DevBuf<int32_t> leaf_flags; // [W] panels of the last append finished by each leaf node
  int tree_overlap = -1; // -1: only when leaves and merge nodes all get a CU of their own; 0 / 1 force it (OVGPU_TSQR_OVERLAP)
  bool tree_nodes_overlap = false, tree_nodes2_overlap = false; // dependency flavour the cached trees were built with
  DevBuf<int32_t> tree_flags;    // [nodes] progress counters
  DevBuf<int32_t> tree_err;      // [1] sticky: a node of the pipelined tree ran into its wait bound
  int tree_G = 0;
  bool tree_pipelined = true;
  // measurement compression of the on-device update (OVGPU_COMPRESS = gram | tsqr):
  //   1 gram    the Gram matrix of the stack on the matrix cores (k_gram.h) + the EKF update in prior-whitened form (k_ekf.h)
  //   0 tsqr    Householder TSQR + the reference-shaped update; always used when the factor itself leaves the device (mode A,
  //             ovgpu_measurement_compress) and beyond 383 columns
  int compress_gram = 1;
  DevBuf<double> gram_part, gram_G, gram_rho, Yaug2, Lw; // Lw: L = U1^T of the prior block (k_tf_lt), read by the per-feature kernel
  double prior_pivot_tol = 1e-13; // options.prior_pivot_tol
  int last_route = OVGPU_COMPRESS_GRAM; // route of the last update (ovgpu_last_update_route)
  bool whiten = true;           // options.gram_no_whiten == 0: the stack is whitened by the prior BEFORE its Gram matrix is formed
  bool gram_is_whitened = false; // c->gram_G / the Gram buffer handed out by the last local stage is the whitened stack's
  bool prior_on_side = false;   // the pending prior-block factorisation runs on stream2 (ev_join marks its end)
  // the fused form of the MSCKF fast path (k_featy.h): rows, projection, stack and gate in one kernel, gate matrix as a SYRK of the whitened rows
  int featy_skip = 0;              // ovgpu_debug_option "featy_skip": ablation bit mask (timing experiments only)
  DevBuf<double> fs_tq;
  DevBuf<int32_t> fs_inst;
  // "feat_classes": a batch with a block-row class AND a one-pass class keeps its instance lists once per block width — fs_inst at 32 columns (the
  // longest fused track's, as ever), fs_inst64 at 64 — built by a second pass of k_batch_layout wherever the first is (enqueue_batch_tables)
  DevBuf<int32_t> fs_inst64;
  int inst64_D = 0;                // the column count fs_inst64 was built for; 0 = not built
  int feat_classes = 0;            // ovgpu_debug_option "feat_classes", a level: 0 one kernel per batch, picked from its longest track; 1 an MSCKF batch laid out for the fast path runs a kernel per length class (plan_feature_stage, feat_classes.h)
  int64_t feat_class_batches = 0;  // ovgpu_debug_option "feat_class_batches": pipelines that launched more than one class, counted once per update as "slam_fused_batches" is
  int feat_class_attempt = 0;      // ... of them, the ones of the update attempt that is running (update_with_fallbacks)
  int last_feat_classes = 0;       // ovgpu_debug_option "last_feature_classes": bit mask over FeatKernel codes 0 .. 3 of the kernels the last batch pipeline launched
  int last_class_features[4] = {0, 0, 0, 0}; // "last_class_features_0" .. "_3": features in the class of that code
  DevBuf<double> featyb_ws;       // k_featy_big.h, k_slam_y_big.h: row panels of the earlier passes, per workgroup
  // k_slam_y_big.h: what its records kernel leaves for it (slamy::SlamYBigStore)
  DevBuf<double> slyb_rows, slyb_V, slyb_hq;
  DevBuf<int32_t> slyb_minfo, slyb_inst;
  int featy_big = 0;               // ovgpu_debug_option "featy_big": 1 = the multi-pass kernel also for tracks the one-pass kernels hold,
                                   // 2 = with 5 tiles per wavefront (several passes on short tracks: tests)
  bool no_feat_kernel = false;  // options.no_fast_feature_kernel
  // the unprojected stack of the Gram route (ovgpu_types.h: RawStack; k_gram.h: k_gram_regions)
  bool raw_enable = true;          // ovgpu_debug_option "raw_stack"
  bool gram_read_ahead = true;     // k_gram_regions<PF>: operand reads a k-step ahead (ovgpu_debug_option "gram_read_ahead")
  int gram_waves = 8;              // k_gram_regions<PF, NW>: wavefronts per workgroup, 8 (two per SIMD) or 4 (ovgpu_debug_option "gram_waves"); without the reads ahead always 4
  bool featy_chains = true;        // k_feat_y<.., CH>: the run table, the next slot requested a feature ahead (ovgpu_debug_option "featy_chains"; k_featy.h)
  int raw_work_const = 12;         // per-row cost of a region beside its tiles, in tiles (ovgpu_debug_option "raw_work_const"; see raw_stack_layout)
  bool raw_veto = false;           // this pipeline's stack feeds mode A's factorisation: projected rows (api_pipeline.inc)
  bool raw_one_region = false;     // (developer experiment, ovgpu_debug_option "raw_stack" = 2: every row in the top region)
  bool raw_cols_ok = false;        // the column map allows it: calibration columns left of every clone's, no landmarks, 6 .. 15 tile columns (build_columns)
  bool raw_tables_ok = false;      // the resident batch has its region tables (ovgpu_set_features)
  int raw_j0 = 0;                  // columns left of it are stored projected (RawStack::j0)
  int raw_ncls = 0, raw_ntc[RAW_MAXCLS + 1] = {0}, raw_ld[RAW_MAXCLS + 1] = {0}, raw_rcol[RAW_MAXCLS + 1] = {0};
  int64_t raw_base[RAW_MAXCLS + 1] = {0}, raw_rows[RAW_MAXCLS + 1] = {0};
  std::vector<uint8_t> h_cls_of_clone;
  DevBuf<uint8_t> cls_of_clone;
  DevBuf<int32_t> raw_featbase, raw_dst, raw_runs; // raw_runs: per feature FY_RUNREC records of 16 bytes (k_batch_layout, for k_feat_y<.., CH = true>)
  DevBuf<double> Hraw;
  DevBuf<gram::GramRegionWG> gram_wg; // one record per workgroup of k_gram_regions
  int gram_wg_n = 0, gram_wg_tiles = 0;
  gram::GramRegionSum raw_rs;      // the regions that have workgroups, for k_gram_regions_reduce
  bool last_stack_raw = false;     // the last pipeline's Gram matrix came from the unprojected stack
  DevView<int32_t> feat_counter;
  DevBuf<int32_t> fs_minfo, fs_meas_feat, fs_pos; // fs_*: the row store of the fast path (feat::FeatStore); fs_pos: each measurement's clone-major position (k_batch_layout)
  DevBuf<int32_t> fs_slots;   // [F][8] the fused kernels' schedule: per slot (features by descending track length) feature, first measurement, count, rows, row offset
  std::vector<int32_t> h_order; // the same order on the host
  std::vector<uint16_t> h_cc;   // packed (camera, clone) codes of the batch being uploaded (kept: no allocation per call)
  DevBuf<double> fs_rows, fs_V, fs_z, fs_w;
  void *comm = nullptr;        // ncclComm_t of this rank (ovgpu_comm_init_rank / ovgpu_multi_create)
  struct LoopComm *loop = nullptr; // several ranks on ONE device (ovgpu_multi_create with a repeated device): the collective is emulated
  int comm_rank = 0, comm_world = 1;
  DevBuf<double> comm_buf;     // gathered triangles of the Householder exchange
  DevView<int32_t> chol_prog;  // [2][16] per-step flags of the single-launch Cholesky (k_chol.h), one set per factorisation in flight
  // flags (4), rows_used (1), feat_counter (1) and chol_prog (32) are views into ONE block, zeroed by one memset at the start of a
  // pipeline call; ctrl_clean says which of them have not been touched since (bits CTRL_*), so that the places that used to zero
  // them one by one (five 5-us launches per update) skip it
  DevBuf<int32_t> ctrl;
  unsigned ctrl_clean = 0;
  unsigned ctrl_pre = 0;       // views zeroed AHEAD of the pipeline call that will use them (enqueue_speculative_prior) and not touched since: ctrl_zero skips them once
  DevBuf<double> chol_uinv;    // [2][16][256]
  DevBuf<double> chol_wide_A, chol_wide_Y; // [D - 256][LA - 256] each: the compact Schur complement and its factorisation (k_chol_wide.h: the second panel beyond 256 columns)
  bool chol_wide = true;          // ovgpu_debug_option "chol_wide": 0 = the step-wise kernels beyond 256 columns (1: two panels of k_chol_fused, measured faster on every leg: DESIGN.md §7)
  int64_t chol_wide_count = 0;    // ovgpu_debug_option "chol_wide_factorisations": factorisations enqueued on the two-panel path
  int gram_wide = 0;              // ovgpu_debug_option "gram_wide": 1 = the whitened Gram route of mode B holds 32 tile columns of [H | r] (D <= 511) instead of 24 (gram_route_tile_cap, api_pipeline.inc); default 0
  int gram_wide_on = 0;           // ... the level in force: taken over by ovgpu_set_state and by a batch handed over (end_feature_batch: ovgpu_set_features, ovgpu_tracks_to_features), nowhere else
  int64_t gram_wide_updates = 0;  // ovgpu_debug_option "gram_wide_updates": updates that took the Gram route at 25 .. 32 tile columns AND stand: counted where the Gram kernel is enqueued, taken off again for an attempt that is repeated or that ends in an error (update_with_fallbacks, ovgpu_slam_update_chunked)
  int gram_wide_attempt = 0;      // ... of them, the ones of the update attempt that is running (update_with_fallbacks)
  int mode_a_wide = 0;            // ovgpu_debug_option "mode_a_wide": 1 = mode A's pivoted Gram route (ovgpu_msckf_compress) holds 32 tile columns of [H | r] (D <= 511) instead of 24 (mode_a_tile_cap, api_pipeline.inc); default 0; independent of "gram_wide"
  int mode_a_wide_on = 0;         // ... the level in force: taken over exactly where gram_wide_on is
  int64_t mode_a_wide_compressions = 0; // ovgpu_debug_option "mode_a_wide_compressions": compressions that took the pivoted route at 25 .. 32 tile columns AND stand (compress_impl takes an attempt it repeats through the Householder route off again)
  int slam_mode_a = 0;            // ovgpu_debug_option "slam_mode_a", a level: 0 off; 1 (and above) ovgpu_slam_compress takes mode A's pivoted Gram route on the terms ovgpu_msckf_compress does (factor_gram, enqueue_pipeline_body), the per-feature stage the kernel "slam_fused" lays the batch out for, and at 17 .. 24 tile columns of D the blocked un-whitening k_unwhiten_blk<24>
  int slam_mode_a_on = 0;         // ... the level in force: taken over exactly where mode_a_wide_on is
  int64_t slam_mode_a_compressions = 0; // ovgpu_debug_option "slam_mode_a_compressions": SLAM compressions that took the pivoted route AND stand (compress_impl takes an attempt it repeats through the Householder route off again)
  int mode_a_panel = 0;           // ovgpu_debug_option "mode_a_panel", a level: 0 off; 1 (and above) mode A's pivoted Gram route factors 17 .. 24 tile columns of [H | r] (D = 256 .. 383) with k_pchol_panel / k_pchol_schur instead of the rank-one k_gram_pchol<NB> (mode_a_panel_factor, api_pipeline.inc), and ovgpu_msckf_compress un-whitens 17 .. 24 tile columns of D with k_unwhiten_blk<24>
  int mode_a_panel_on = 0;        // ... the level in force: taken over exactly where mode_a_wide_on is
  int64_t mode_a_panel_compressions = 0; // ovgpu_debug_option "mode_a_panel_compressions": compressions that took the panelled factor at 17 .. 24 tile columns AND stand (compress_impl takes an attempt it repeats through the Householder route off again)
  DevBuf<double> pchol_dots;      // [512 + 8] k_pchol_wide.h: the running diagonal and the first pivot between the panels' launches
  DevBuf<double> uinv_tiles;      // [32][256] k_uinv_tiles: U_JJ^-1 of a prior block that was factored step-wise, for k_unwhiten_blk<32>
  PinBuf<double> h_tri;        // mode A: the compressed system on its way to the caller ([D x LD] + one word of flags per double behind it)
  int chol_slot = 0;
  bool no_chol_pipe = false;   // options.no_single_launch_cholesky
  int tri_waves = 0;           // features per workgroup of k_triangulate; 0 = by the batch (enqueue_triangulate); ovgpu_debug_option "tri_waves" forces 1 .. 16
  int feat_shape = 0;          // options.feature_kernel_shape
  Uplink<HipLink> up;    // page-locked upload arena of ovgpu_set_state / ovgpu_set_features; ovgpu_debug_option "upload_kernel" 0 = one hipMemcpyAsync per array (rounds 4-5)
  Landing<HipLink> down; // page-locked landing zone of the results (status, chi2, p_FinG, dx, P'): one gather launch, one synchronisation, memcpy to the caller
  const double *chi2_table_dev = nullptr; // what the device's chi2 table holds: buffer and length at its last upload
  int chi2_table_dev_len = 0;
  bool gram_fp32 = false;      // options.gram_fp32
  bool want_stack_f32 = false; // this pipeline: gram_fp32 on the prior-whitened Gram route -> the fused per-feature kernels may store floats
  bool stack_is_f32 = false;   // ... and did: the stack is c->Hbig32 [rows_total][stack_ldf] (k_gram32.h reads it)
  int stack_ldf = 0;
  DevBuf<float> Hbig32, gram32_part;
  DevBuf<int32_t> gram32_tiles;
  int gram32_ntm = 0, gram32_P = 0; // the tile table on the device is for this macro grid
  int Lw_D = -1;               // column count c->Lw was zeroed for (its upper triangle stays zero)
  DevBuf<long long> dbg_cycles; // ovgpu_debug_cycles: per-phase cycle counters of workgroup 0 of the per-feature kernel
  int tsqr_workers = 0;         // options.tsqr_workers
  bool async_pending = false;     // ovgpu_msckf_update_async since the last ovgpu_synchronize
  bool last_update_tform = false; // the last EKF stage enqueued was the Gram-form one (finish_update may fall back)
  bool force_tsqr = false;        // one-shot: the next pipeline takes the Householder route
  int chol_spin_limit = 1 << 22;  // the wait bound of k_chol_fused's follower workgroups (ovgpu_debug_option "chol_follow_spin_limit" lowers it to provoke the fall-back)
  int chol_timeouts = 0;          // how often update_with_fallbacks repeated an update with the step-wise kernels
  int mode_a_factor = 0;          // where mode A's compressed factor comes from: 0 Householder TSQR, 2 the diagonally pivoted Cholesky factor of the whitened Gram matrix (PCHOLQR)
  bool factor_from_gram = false;  // one-shot (compress_impl): the compressed factor of mode A comes from the Gram matrix of the whitened stack
  bool last_factor_from_gram = false;
  // read-only ovgpu_debug_option "last_gram_kernel" / "last_factor_kernel" / "last_unwhiten_kernel": what the last batch pipeline launched
  //   gram:     0 none, 1 k_gram_il / k_gram<NT> (launch_gram), 2 k_gram_blk, 3 k_gram_wide, 4 k_gram_regions, 5 k_gram_f32
  //   factor:   0 none (the Householder triangle), 1 k_gram_pchol_blk<4, 9, 2>, 2 k_gram_pchol_blk<7, 15, 4>, 3 k_pchol_panel + k_pchol_schur (k_pchol_wide.h), 32 + NB k_gram_pchol<NB>
  //   unwhiten: 0 none, 1 k_unwhiten_blk<16>, 2 k_unwhiten<16>, 3 k_unwhiten<24>, 4 k_unwhiten_blk<32> on the two-panel factorisation's inverse tiles, 5 k_unwhiten_blk<32> on k_uinv_tiles'
  int last_gram_kernel = 0, last_factor_kernel = 0, last_unwhiten_kernel = 0;
  int last_gram_workgroups = 0;   // read-only "last_gram_workgroups": gridDim.x of the last pipeline's k_gram_f32 (Gw) or k_gram_blk (Gb) launch, 0 for every other Gram kernel
  bool chol_timed_out = false;    // finish_update: a follower of the single-launch Cholesky gave up waiting; nothing was modified
  bool prior_pending = false; // the sharded update's local stage has started the prior block's factorisation on stream2
  bool prior_overlap = true; // options.no_prior_overlap == 0: the prior block is factored on the second stream
  const double *last_uinv = nullptr;  // U_kk^-1 tiles of the factorisation enqueue_chol_carry launched last (null: the step-wise fall-back ran)
  const double *prior_uinv = nullptr; // ... of the prior block's factorisation (k_unwhiten_blk multiplies by them instead of substituting)
  int layout_fpw = 8;                 // ovgpu_debug_option "layout_fpw": features per workgroup of k_batch_layout at most (1 .. 8; api_state.inc picks the fewest that keep the launch at 250 workgroups)
  bool unwhiten_blocked = true;       // ovgpu_debug_option "unwhiten_blocked" (0: k_unwhiten of rounds 3-5)
  bool pchol_blocked = true;     // ovgpu_debug_option "pchol_blocked": mode A's pivoted factor by k_gram_pchol_blk (k_pchol.h; 0: the rank-one kernel of rounds 3-5)
  bool speculative_prior = true; // ovgpu_debug_option "speculative_prior": ovgpu_set_features starts that factorisation (api_pipeline.inc: enqueue_speculative_prior)
  DevBuf<int32_t> gram_dropped;
  DevView<int32_t> rows_used; // rows of accepted features, counted by k_system
  DevBuf<double> sys_rows_ws;      // k_system_t<true> (plan.rows_global): its per-workgroup record workspace
  int row_stride = 48;

  // ---- timing
  std::vector<EventPair> ev_compress, ev_update, ev_system;
  size_t ev_used = 0;
  bool timed_this_update = false; // the last enqueued pipeline recorded its stage events (stage_timing_period skips most)
  bool timing = true;
  int timing_period = 1;        // ovgpu_debug_option "stage_timing_period": the stage events go into every n-th update only (each is a
  uint64_t timing_seq = 0;      // marker packet the next kernel waits for: ~3 us apiece, six per update)
};

// The batch the stages run on: the view in force, or else the whole resident batch composed from its owners NOW (no pointer outlives a
// reserve of its buffer, so none can go stale).  The one list of what a view replaces is Batch's members.
static Batch batch_of(const ovgpu_ctx *c) {
  if (c->view) return *c->view;
  Batch b;
  b.F = c->F, b.M = c->M, b.m_max = c->m_max, b.rows_total = c->rows_total;
  b.h_offsets = span_of(c->h_offsets), b.h_order = span_of(c->h_order), b.h_feat_lm = span_of(c->h_feat_lm), b.h_row_off = span_of(c->h_row_off);
  b.have_sigma = c->have_feat_sigma, b.have_mult = c->have_feat_mult;
  b.meas_offsets = c->meas_offsets.p, b.sys_order = c->sys_order.p, b.status = c->status.p, b.meas_cc = c->meas_cc.p, b.uv = c->uv.p, b.uvn = c->uvn.p;
  b.row_off = c->row_off.p, b.pA = c->pA.p, b.pG = c->pG.p, b.chi2 = c->chi2.p, b.chi2_thr = c->chi2_thr.p, b.feat_sigma = c->feat_sigma.p, b.feat_mult = c->feat_mult.p;
  return b;
}
// puts a batch in force for a scope: no return path leaves it behind
struct BatchScope {
  ovgpu_ctx *c;
  BatchScope(ovgpu_ctx *ctx, const Batch *b) : c(ctx) { c->view = b; }
  ~BatchScope() { c->view = nullptr; }
  BatchScope(const BatchScope &) = delete;
  BatchScope &operator=(const BatchScope &) = delete;
};
// no stage events for a scope (ovgpu_ctx::timing)
struct NoStageTiming {
  ovgpu_ctx *c;
  bool was;
  explicit NoStageTiming(ovgpu_ctx *ctx) : c(ctx), was(ctx->timing) { c->timing = false; }
  ~NoStageTiming() { c->timing = was; }
  NoStageTiming(const NoStageTiming &) = delete;
  NoStageTiming &operator=(const NoStageTiming &) = delete;
};

// removes element `idx` of a device array of `n` records of `w` doubles / ints (through a scratch copy: the ranges overlap)
template <class T>
static hipError_t remove_record(DevBuf<T> &a, DevBuf<T> &tmp, int n, int w, int idx, hipStream_t s) {
  const size_t tail = (size_t)(n - idx - 1) * w;
  if (tail == 0) return hipSuccess;
  hipError_t e = tmp.reserve(tail);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(tmp.p, a.p + (size_t)(idx + 1) * w, tail * sizeof(T), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(a.p + (size_t)idx * w, tmp.p, tail * sizeof(T), hipMemcpyDeviceToDevice, s);
}

static hipError_t upload(void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
}

// the landing zone's gather launch (host_link.h: Landing)
__global__ void __launch_bounds__(256) k_download_gather(unsigned char *__restrict__ arena, UpBatch b) {
  const UpSeg sg = b.seg[blockIdx.y];
  unsigned char *dst = arena + sg.off;
  const unsigned char *src = static_cast<const unsigned char *>(sg.dst);
  const uint32_t nvec = ((reinterpret_cast<uintptr_t>(src) & 15) == 0) ? sg.bytes >> 4 : 0;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src);
  u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) __builtin_nontemporal_store(s4[i], d4 + i);
  for (uint32_t i = (nvec << 4) + blockIdx.x * 256 + threadIdx.x; i < sg.bytes; i += gridDim.x * 256) dst[i] = src[i];
}
inline hipError_t HipLink::gather(hipStream_t s, unsigned char *zone, const UpBatch &b) {
  hipLaunchKernelGGL(k_download_gather, dim3(UP_BLOCKS, b.n), dim3(256), 0, s, zone, b);
  return hipGetLastError();
}

// a synchronisation of stream s that the caller needs anyway, with everything registered for upload or read-back on its way first
// (EVERY synchronisation of the context's stream goes through here — ovgpu_synchronize, the read-backs, the track store — so that the
// arena's offset returns to 0 behind any of them: a caller that only ever uses the asynchronous update would otherwise grow it for ever)
static hipError_t upload_sync(ovgpu_ctx *c, hipStream_t s) {
  if (hipError_t e = c->up.flush(); e != hipSuccess) return e;
  if (hipError_t e = c->down.flush(); e != hipSuccess) return e;
  if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
  if (s == c->stream) c->up.synced(), c->down.synced();
  return hipSuccess;
}

// profiling builds (-DQR_PROFILE): 128 cycle counters written by node 0 of the last leaf / merge launch
static long long *qr_dbg_buffer() {
#ifdef QR_PROFILE
  static long long *buf = nullptr;
  if (!buf) {
    (void)hipMalloc((void **)&buf, 128 * sizeof(long long));
    (void)hipMemset(buf, 0, 128 * sizeof(long long));
  }
  return buf;
#else
  return nullptr;
#endif
}

static long long *tree_dbg_buffer() {
#ifdef QR_PROFILE
  static long long *buf = nullptr;
  if (!buf) {
    (void)hipMalloc((void **)&buf, 1024 * sizeof(long long));
    (void)hipMemset(buf, 0, 1024 * sizeof(long long));
  }
  return buf;
#else
  return nullptr;
#endif
}

// The kernel, with its dynamic-LDS bound raised to what the device allows on the context's device: the only place that sets the attribute.  The
// bound is the workgroup's limit (c->lds_limit) less the kernel's own static LDS: a bound that does not fit next to static arrays is refused, and
// the launch after it as well (none of the kernels that come through here has any today).  HIP keeps the attribute per kernel AND per device, so the latch is one per
// kernel (this template's static) with a bit per device; the device is current at every launch site (the entry points' hipSetDevice).  Two threads
// that meet a kernel's first launch together both set it — harmless — and nobody launches before it is set.  Devices beyond 63 have no bit: set
// every time.
template <auto KERN>
static decltype(KERN) with_max_lds(const ovgpu_ctx *c) {
  static std::atomic<uint64_t> set_on{0};
  const uint64_t bit = (unsigned)c->device < 64 ? (uint64_t)1 << c->device : 0;
  if (!(set_on.load(std::memory_order_acquire) & bit)) {
    hipFuncAttributes fa{};
    const int own = hipFuncGetAttributes(&fa, (const void *)KERN) == hipSuccess ? (int)fa.sharedSizeBytes : 0;
    (void)hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_limit - own);
    set_on.fetch_or(bit, std::memory_order_release);
  }
  return KERN;
}

static constexpr int QR_B = 32;  // row block of the generic fallback kernel (D + 1 > 256 columns)
static constexpr int QR_LEAF_Q = 32; // leaf nodes fold 4 * 32 = 128 dense rows per append

template <int QH, bool TRI>
static int launch_qr_node(ovgpu_ctx *c, int nodes, const QrNodeParams &q) {
  const size_t lds = qr_node_lds_bytes(q.NT, QH);
  const int NW = (q.NT + 1) / 2;
  hipLaunchKernelGGL((with_max_lds<k_qr_node<QH, TRI>>(c)), dim3(nodes), dim3(64 * NW), lds, c->stream, q);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// leaf nodes: the "panel wave" variant (k_tsqr_pw.h), NT <= 15
template <int QH>
static int launch_qr_leaf_pw(ovgpu_ctx *c, int nodes, const QrNodeParams &q) {
  const size_t lds = pw::qr_node_lds_bytes(q.NT, QH);
  const int NW = pw::qr_node_bulk_waves(q.NT) + 1;
  hipLaunchKernelGGL((with_max_lds<pw::k_qr_node<QH, false>>(c)), dim3(nodes), dim3(64 * NW), lds, c->stream, q);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

// the whole merge tree in one pipelined launch (k_qr_tree); G - 1 nodes, all co-resident
template <int QH>
static int launch_qr_tree(ovgpu_ctx *c, int nodes, const QrTreeParams &q, hipStream_t ts) {
  const size_t lds = qr_node_lds_bytes(q.NT, QH);
  const int NW = (q.NT + 1) / 2;
  hipLaunchKernelGGL((with_max_lds<k_qr_tree<QH>>(c)), dim3(nodes), dim3(64 * NW), lds, ts, q);
  HIPCHK(hipGetLastError());
  return OVGPU_OK;
}

template <int NTC> static void launch_gram(const ovgpu_ctx *c, int G, const gram::GramParams &g, hipStream_t s, bool interleaved) {
  // staging inside the matrix-instruction stream (k_gram_il) up to 15 tile columns (15 — BASELINE configs[3]'s 237 columns — since round 6: 30
  // accumulator tiles per wavefront instead of the 34 of the 16-column grid it used to run on, a whole tile column of zeros); with 16 the 34
  // accumulator tiles + staged elements + hoisted LDS operands exceed the 512 registers of a wavefront (1.1 KB of scratch per lane) and k_gram stays
  auto kern = with_max_lds<gram::k_gram<NTC>>(c);
  if constexpr (NTC <= 15) {
    if (interleaved) kern = with_max_lds<gram::k_gram_il<NTC>>(c);
  }
  hipLaunchKernelGGL(kern, dim3(G), dim3(256), gram::gram_lds_bytes(), s, g);
}

// (this launcher keeps its own latch, once per PROCESS, and its own bound of 128 KB: the kernel has static LDS next to the dynamic part — 160 KB
// are refused — and its move to with_max_lds is left out: DESIGN.md section 7, "Context buffers free themselves")
template <int NB> static void launch_gram_pchol(hipStream_t s, int D, int LD, int LG, const double *G, double *out, int32_t *dropped, double tol) {
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void *)gram::k_gram_pchol<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_done = true;
  }
  hipLaunchKernelGGL(gram::k_gram_pchol<NB>, dim3(1), dim3(1024), gram::chol_lds_bytes(LD), s, D, LD, LG, G, out, dropped, tol);
}

template <int NW, int SL, int NQ> static void launch_gram_pchol_blk(hipStream_t s, int D, int LD, int LG, const double *G, double *out, int32_t *dropped, double tol) {
  hipLaunchKernelGGL((gram::k_gram_pchol_blk<NW, SL, NQ>), dim3(1), dim3(64 * (NW + 1)), 0, s, D, LD, LG, G, out, dropped, tol);
}

// A prior-block factorisation that is (or may still be) running on the second stream and that nobody will join: it reads the covariance and owns
// the factorisation's work matrices and flag words, so whoever is about to change the one or to use the others waits for it first.  (Since round 6
// ovgpu_set_features starts one ahead of every batch — enqueue_speculative_prior, api_pipeline.inc.)
static int drop_pending_prior(ovgpu_ctx *c) {
  if (c->prior_on_side && c->ev_join) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->prior_on_side = false;
  }
  c->prior_pending = false;
  return OVGPU_OK;
}
