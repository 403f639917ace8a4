/*
 * ovgpu.h — C ABI of the MI355X-native MSCKF / SLAM EKF feature-update path.
 *
 * This is the drop-in boundary.  Everything that crosses it is
 * plain-old-data: flat arrays, sizes and status codes.  The functions declared
 * here are what a binding inside rpng/open_vins (the C++ shim under
 * open_vins_amd/shim/) calls in place of the reference's
 * Eigen code.  Each entry point cites the reference interface it replaces
 * (paths relative to the open_vins checkout, v2.7).
 *
 * Conventions
 *   - all matrices are row-major, IEEE double unless stated (pixel
 *     measurements are float, exactly as ov_core::Feature stores them,
 *     ov_core/src/feat/Feature.h:49-55);
 *   - quaternions are JPL, stored (x,y,z,w) (ov_core/src/utils/quat_ops.h);
 *   - every function returns an ovgpu_status (0 = OK); nothing exits the
 *     process (the reference's std::exit on a negative covariance diagonal,
 *     ov_msckf/src/state/StateHelper.cpp:172-182, becomes
 *     OVGPU_ERR_NEGATIVE_DIAGONAL);
 *   - buffers are owned by the caller; the context owns its device memory;
 *   - a context is bound to one HIP device and is not re-entrant, matching the
 *     reference's single-threaded update path (SURVEY.md §8b "Threading").
 */
#ifndef OVGPU_H
#define OVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* ABI version.  Bumped whenever an entry point changes what it returns.      */
/*   3  (round 3) ovgpu_msckf_compress: the DEFAULT compressed system is the  */
/*      dense, rank x D pivoted-Cholesky factor of the whitened Gram matrix   */
/*      (rows < D possible, not triangular); the reference's upper-triangular */
/*      D x D Householder factor needs compress_route = OVGPU_COMPRESS_TSQR.  */
/*      A caller that assumes rows == D or a triangle must set that route.    */
/*   4  (round 4) perform_anchor_change: the first estimate of an             */
/*      ANCHORED_MSCKF_INVERSE_DEPTH / single-depth landmark moves as the     */
/*      reference moves it (Landmark::get_xyz(true) reads the current value); */
/*      multi-rank updates return OVGPU_ERR_HIP on a follower time-out        */
/*      instead of repeating locally; ovgpu_update_stats::ms_* are 0 for an   */
/*      update that recorded no stage events.                                 */
/*   5  (round 4) the MSCKF gate accepts a feature whose residual bound is    */
/*      under its threshold without factoring its gate matrix                 */
/*      (ovgpu_options::gate_always_factor, in the slot of the retired        */
/*      tsqr_leaf_blocked; 0 = default).  Verdicts, dx, P' unchanged; the     */
/*      chi2 OUTPUT of such a feature is the bound, an upper bound of the      */
/*      reference's statistic.  ovgpu_update_stats::_pad0 became n_gate_bound. */
/*      A caller that logs or thresholds the chi2 values itself sets           */
/*      gate_always_factor = 1.                                                */
/*   6  (round 4) the device track store answers the rest of FeatureDatabase:  */
/*      ovgpu_tracks_containing / _containing_older / _oldest_timestamp /      */
/*      _cleanup_measurements / _cleanup_measurements_exact / _get_feature.    */
/*      ovgpu_tracks_not_containing_newer reads the stored observations (per   */
/*      camera the LAST one, as the reference does) instead of the host's      */
/*      record of the last append: same answer for times appended in order.    */
/*   7  (round 5) ovgpu_landmarks_view grew a last member, feat_rep_each: the   */
/*      representation PER LANDMARK (NULL = feat_rep for all, the behaviour     */
/*      before), so that one ovgpu_slam_update stacks SLAM landmarks and ArUco   */
/*      corners kept in different representations as UpdaterSLAM.cpp:427-447     */
/*      does; ovgpu_slam_delayed_init may initialise in a representation other   */
/*      than the resident landmarks'; ovgpu_get_landmark_reps reads them back.   */
/*      A caller compiled against ABI 6 passes a shorter struct: rebuild.        */
/*   8  (round 6) OVGPU_COMPRESS_CHOLQR (= 2, the unpivoted Cholesky factor of  */
/*      the Gram matrix as a compressed system: a documented negative result)   */
/*      is gone: ovgpu_create returns OVGPU_ERR_INVALID for it.  Nothing else   */
/*      changed shape.  New: ovgpu_comm_info.                                   */
/*   9  ovgpu_set_active_landmarks: the Jacobian columns of the SLAM calls cover */
/*      the landmarks the caller names instead of every resident one.           */
/*      ovgpu_set_landmarks no longer returns OVGPU_ERR_CAPACITY when all        */
/*      landmarks together exceed 511 columns: the SLAM call whose EFFECTIVE     */
/*      column set exceeds them does.  A caller that never names a set and stays */
/*      under that bound sees what ABI 8 computed.  Nothing changed shape.       */
/*  10  ovgpu_slam_change_anchors_batched (every moving landmark in a fixed      */
/*      number of launches) and ovgpu_slam_anchor_systems(_len) (mode A of       */
/*      UpdaterSLAM::change_anchors).  Nothing changed shape; the entries of     */
/*      ABI 9 compute what they computed.                                        */
/*      Added later under the same number (nothing changed shape or result):    */
/*      ovgpu_state_marginalize_batched.  Callers discover it by symbol (a weak */
/*      reference in C / C++, hasattr in Python), not by the ABI number.        */
/*      Likewise ovgpu_slam_update_chunked (every chunk of a frame's SLAM        */
/*      update in one device pass): a new symbol under the same number.          */
/*      Likewise ovgpu_msckf_update_lm (the MSCKF update of a state whose        */
/*      resident landmarks stay current, on the landmark-free state's kernels). */
/*      Likewise ovgpu_slam_delayed_init_fused (the delayed initialisation with  */
/*      every candidate's step as five launches; ovgpu_slam_delayed_init keeps   */
/*      its kernels and its bits).                                               */
/*      Likewise the debug option "slam_fused" (ovgpu_slam_update's per-feature  */
/*      stage as one fused kernel on the matrix cores; off by default: every     */
/*      entry enqueues what it enqueued and returns its bits).  No new symbol.   */
/*      Likewise the debug option "slam_mode_a" (ovgpu_slam_compress on the      */
/*      pivoted Gram route; off by default: every entry enqueues what it         */
/*      enqueued and returns its bits).  No new symbol.                          */
/* ------------------------------------------------------------------------- */
#define OVGPU_ABI_VERSION 10
int ovgpu_abi_version(void);

/* ------------------------------------------------------------------------- */
/* status codes                                                              */
/* ------------------------------------------------------------------------- */
typedef enum {
  OVGPU_OK = 0,
  OVGPU_ERR_INVALID = 1,           /* bad argument / size                    */
  OVGPU_ERR_NO_DEVICE = 2,         /* no HIP device / extension unusable     */
  OVGPU_ERR_HIP = 3,               /* a HIP runtime call failed              */
  OVGPU_ERR_NEGATIVE_DIAGONAL = 4, /* StateHelper.cpp:172-182                */
  OVGPU_ERR_NOT_SPD = 5,           /* Cholesky of S broke down               */
  OVGPU_ERR_CAPACITY = 6,          /* more clones/cams/measurements than ctx */
  OVGPU_ERR_NO_STATE = 7           /* ovgpu_set_state was never called       */
} ovgpu_status;

/* per-feature outcome (what the reference expresses by erasing the feature
 * from feature_vec and setting to_delete, UpdaterMSCKF.cpp:88-90,136-139,
 * 225-227)                                                                   */
typedef enum {
  OVGPU_FEAT_USED = 0,           /* accepted, stacked into the update        */
  OVGPU_FEAT_TOO_FEW_MEAS = 1,   /* < 2 measurements after cleaning (:87)    */
  OVGPU_FEAT_TRI_FAILED = 2,     /* single_triangulation returned false      */
  OVGPU_FEAT_GN_FAILED = 3,      /* single_gaussnewton returned false        */
  OVGPU_FEAT_CHI2_REJECTED = 4   /* chi2 > chi2_multipler * table (:225)     */
} ovgpu_feat_status;

/* ov_type::LandmarkRepresentation::Representation
 * (ov_core/src/types/LandmarkRepresentation.h:38-46), same numeric values    */
typedef enum {
  OVGPU_REP_GLOBAL_3D = 0,
  OVGPU_REP_GLOBAL_FULL_INVERSE_DEPTH = 1,
  OVGPU_REP_ANCHORED_3D = 2,
  OVGPU_REP_ANCHORED_FULL_INVERSE_DEPTH = 3,
  OVGPU_REP_ANCHORED_MSCKF_INVERSE_DEPTH = 4,
  OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE = 5
} ovgpu_feat_rep;

/* ------------------------------------------------------------------------- */
/* options: UpdaterOptions (ov_msckf/src/update/UpdaterOptions.h:32-48),      */
/* FeatureInitializerOptions (ov_core/src/feat/FeatureInitializerOptions.h:   */
/* 33-69) and the StateOptions subset the path reads                          */
/* (ov_msckf/src/state/StateOptions.h:35-92).  Defaults = the reference's.    */
/* ------------------------------------------------------------------------- */
typedef struct {
  /* UpdaterOptions */
  double chi2_multipler; /* (sic) reference spelling, default 5              */
  double sigma_pix;      /* default 1                                        */
  /* FeatureInitializerOptions */
  int32_t triangulate_1d;  /* default 0 */
  int32_t refine_features; /* default 1 */
  int32_t max_runs;        /* default 5 */
  int32_t _pad0;
  double init_lamda;      /* 1e-3 */
  double max_lamda;       /* 1e10 */
  double min_dx;          /* 1e-6 */
  double min_dcost;       /* 1e-6 */
  double lam_mult;        /* 10   */
  double min_dist;        /* 0.10 */
  double max_dist;        /* 60   */
  double max_baseline;    /* 40   */
  double max_cond_number; /* 10000 */
  /* StateOptions subset */
  int32_t do_fej;                     /* use_fej                            */
  int32_t do_calib_camera_pose;       /* calib_cam_extrinsics               */
  int32_t do_calib_camera_intrinsics; /* calib_cam_intrinsics               */
  int32_t feat_rep_msckf;             /* ovgpu_feat_rep                     */
  /* Library switches.  Everything that can change the arithmetic route of   */
  /* an update is an option of the context, never the environment; 0 is the  */
  /* default of every field (a zero-initialised tail behaves like            */
  /* ovgpu_default_options).                                                  */
  int32_t compress_route;    /* ovgpu_compress_route of the on-device update */
  int32_t gram_no_whiten;    /* 1: Gram matrix of the raw stack, whitened    */
                             /* afterwards (round-1 form; loses accuracy     */
                             /* when the prior is large along the            */
                             /* unobservable directions)*/
  int32_t no_prior_overlap;  /* 1: factor the prior block on the main stream */
  int32_t tsqr_workers;      /* leaf nodes of the Householder TSQR, 0 = one  */
                             /* per compute unit                             */
  int32_t tsqr_no_pipeline;  /* 1: merge tree level by level                 */
  int32_t tsqr_overlap;      /* 0 auto, 1 merge tree next to the leaves,     */
                             /* 2 never                                      */
  int32_t gate_always_factor; /* MSCKF gate (round 4; the slot of round 3's retired tsqr_leaf_blocked).  0 (default): a feature whose  */
                             /* RESIDUAL BOUND |r'|^2 / sigma^2 (r' = the nullspace-projected residual) is under its threshold  */
                             /* is accepted without forming or factoring its gate matrix: S = H P H^T + sigma^2 I >= sigma^2 I,  */
                             /* hence chi2 = r'^T S^-1 r' <= the bound, and the reference's test (UpdaterMSCKF.cpp:216-225)      */
                             /* cannot reject it.  Accept / reject sets, dx and P' are those of the full gate; the chi2 output   */
                             /* of such a feature is the BOUND (>= the reference's statistic, <= chi2_thresh);                   */
                             /* ovgpu_update_stats::n_gate_bound counts them.  1: every gate matrix is formed and factored and   */
                             /* every chi2 output is the reference's statistic.  The bound is used by the fused per-feature    */
                             /* kernels (MSCKF features in a global representation, tracks of up to 232 observations); the      */
                             /* general kernel (anchored representations, SLAM, delayed initialisation) always factors          */
  int32_t no_timing;         /* 1: no HIP events around the stages           */
  int32_t no_fast_feature_kernel; /* 1: always the general per-feature       */
                             /* kernel (k_system) instead of the MSCKF fast  */
                             /* path (k_feat: gate matrix in registers)      */
  int32_t no_single_launch_cholesky; /* 1: the Cholesky-with-carry factorisations run as one launch per 16 rows (0: one launch up to 256 columns, four up to 512) */
                             /* (k_ekf_chol_step) instead of the pipelined single launch (k_chol.h)           */
  double prior_pivot_tol;    /* Gram route: a pivot of the prior block's      */
                             /* Cholesky factorisation below this fraction of */
                             /* its diagonal entry sends the update through   */
                             /* the Householder route instead (0 = 1e-13:     */
                             /* cond(P_DD) beyond ~1e13) */
  int32_t feature_kernel_shape; /* MSCKF fast path: 0 = chosen from the longest */
                             /* track; 1 = 4 wavefronts x 11 gate tiles, 2 = 8 x */
                             /* 17 (tuning / tests; a shape the batch does not   */
                             /* fit falls back to the automatic choice)          */
  int32_t gram_fp32;         /* 1: the Gram matrix of the (prior-whitened)    */
                             /* stack is formed in fp32 — BASELINE configs[4]'s */
                             /* "fp32 compressed-QR"; up to 383 columns, on the */
                             /* update, local-Gram and sharded entries.  Two    */
                             /* device paths.  (a) The fused per-feature        */
                             /* kernels (the MSCKF fast path: one noise level,  */
                             /* no resident landmark off the fast path,         */
                             /* "featy_big" != 2) store the stack as FLOATS and */
                             /* gram32::k_gram_f32 forms G on                   */
                             /* v_mfma_f32_32x32x2_f32 ("stack_is_f32" 1,       */
                             /* "last_gram_kernel" 5).  (b) Where the stack     */
                             /* stays float64 on such a context — the general   */
                             /* per-feature kernel: no_fast_feature_kernel,     */
                             /* tracks beyond the fused kernels, per-feature    */
                             /* noise, resident landmarks off the fast path; or */
                             /* "featy_big" = 2, which has no float twin —      */
                             /* gram::k_gram_blk<true> rounds it to float stage */
                             /* by stage and forms G on v_mfma_f32_16x16x4_f32  */
                             /* ("last_gram_kernel" 2).  Either way a product   */
                             /* is summed in fp32 over one stage of 32 rows at  */
                             /* most and the stages in float64, so with         */
                             /* u = 2^-24 and n_i the 2-norm of column i of the */
                             /* stack  |G_ij - (A^T A)_ij| <= 40 u n_i n_j      */
                             /* (35 u and 34 u by the arithmetic; measured 0.4  */
                             /* to 9 u: tests/test_gpu_fp32_gram.py, DESIGN.md  */
                             /* section 7); the update stays within dx 1e-4 /   */
                             /* P 1e-3 of the f64 result                        */
                             /* (tests/test_gpu_fullsize.py)                    */
} ovgpu_options;

/* Measurement compression (UpdaterHelper.cpp:456-487) of ovgpu_msckf_update / ovgpu_slam_update (mode B) and  */
/* of ovgpu_msckf_compress (mode A: the compressed system leaves the device):                                */
typedef enum {
  OVGPU_COMPRESS_GRAM = 0,   /* default.  Mode B: Gram matrix of the prior-whitened stack on the matrix cores + */
                             /* the update in whitened coordinates (D <= 383 columns; D <= 511 on a float64     */
                             /* context under ovgpu_debug_option "gram_wide" = 1).  Mode A: the DIAGONALLY       */
                             /* PIVOTED Cholesky factor of that Gram matrix, un-whitened — a dense rank x D     */
                             /* system with H^T H, H^T r of the stack (D <= 255; Householder beyond, for SLAM   */
                             /* stacks and when the prior block's factorisation fails)                          */
  OVGPU_COMPRESS_TSQR = 1,   /* Householder TSQR: the reference's upper-triangular factor (mode A) + the        */
                             /* reference-shaped update (mode B); always used by ovgpu_measurement_compress     */
                             /* (2 was OVGPU_COMPRESS_CHOLQR, the UNPIVOTED factor of the Gram matrix: a        */
                             /* measured negative result — closed-loop drift 6e-6 — retired with ABI 8;         */
                             /* ovgpu_create refuses the value)                                                 */
  OVGPU_COMPRESS_PCHOLQR = 3 /* what ovgpu_last_update_route reports after a mode A call that took the pivoted  */
                             /* factor; as an option it is an alias of OVGPU_COMPRESS_GRAM                      */
} ovgpu_compress_route;

/* Fills *o with the reference defaults. */
void ovgpu_default_options(ovgpu_options *o);

/* ------------------------------------------------------------------------- */
/* state snapshot: what UpdaterMSCKF::update reads out of ov_msckf::State     */
/* (ov_msckf/src/state/State.h:137-192).  The clone table is ordered by the   */
/* caller (normally ascending timestamp = iteration order of _clones_IMU).    */
/* ------------------------------------------------------------------------- */
typedef struct {
  int32_t N;               /* dim of the covariance (State::_Cov)           */
  int32_t C;               /* number of IMU clones in the window            */
  int32_t K;               /* number of cameras                             */
  int32_t _pad0;
  const double *P;             /* [N*N] row-major covariance                */
  const double *clone_q_p;     /* [C*7] q_GtoI (JPL xyzw), p_IinG  (value)  */
  const double *clone_q_p_fej; /* [C*7] first-estimate values (PoseJPL fej) */
  const int32_t *clone_cov_id; /* [C]   Type::id() of each clone (6 dof)    */
  const double *calib_q_p;     /* [K*7] q_ItoC, p_IinC                      */
  const double *intrinsics;    /* [K*8] fx fy cx cy d0 d1 d2 d3             */
  const uint8_t *cam_is_fisheye; /* [K] 0 = CamRadtan, 1 = CamEqui          */
  const int32_t *calib_cov_id; /* [K] id of the 6-dof extrinsic, -1 if none */
  const int32_t *intr_cov_id;  /* [K] id of the 8-dof intrinsics, -1 if none*/
} ovgpu_state_view;

/* ------------------------------------------------------------------------- */
/* feature tracks, flattened (ov_core::Feature, Feature.h:39-98).             */
/* Measurements of feature f are meas_offsets[f] .. meas_offsets[f+1]-1.      */
/* Inside a feature they MUST be grouped by camera in the iteration order of  */
/* Feature::timestamps and in time order inside a camera: the anchor rule of  */
/* FeatureInitializer.cpp:36-46 (first camera group with strictly most        */
/* measurements, last measurement of that group) is evaluated on this order.  */
/* clone_idx is the index into the clone table (the result of                 */
/* Feature::clean_old_measurements, Feature.cpp:26-53, done by the caller).   */
/* ------------------------------------------------------------------------- */
typedef struct {
  int32_t F; /* number of features                                        */
  int32_t M; /* total number of measurements = meas_offsets[F]            */
  const int32_t *meas_offsets; /* [F+1]                                   */
  const float *uv;             /* [2*M] raw pixel (Feature::uvs)          */
  const float *uvn;            /* [2*M] normalized (Feature::uvs_norm)    */
  const int32_t *clone_idx;    /* [M]                                     */
  const int32_t *cam_idx;      /* [M]                                     */
} ovgpu_features_view;

/* ------------------------------------------------------------------------- */
/* results of one MSCKF update                                                */
/* ------------------------------------------------------------------------- */
typedef struct {
  int32_t n_used;      /* features stacked into the update                  */
  int32_t n_rows;      /* rows of Hx_big before compression (ct_meas)       */
  int32_t D;           /* columns of the stacked Jacobian (canonical order) */
  int32_t n_rows_comp; /* rows after measurement compression                */
  int32_t status;      /* ovgpu_status of the EKF step                      */
  int32_t n_gate_bound; /* features the gate's residual bound accepted (ovgpu_options::gate_always_factor = 0; was _pad0) */
  /* device-side stage times in ms (same five stages the reference prints,
   * UpdaterMSCKF.cpp:289-294), 0 when timing is disabled                   */
  float ms_triangulate;
  float ms_system;
  float ms_compress;
  float ms_update;
  float ms_total;
  float _pad1;
} ovgpu_update_stats;

typedef struct ovgpu_ctx ovgpu_ctx;

/* ------------------------------------------------------------------------- */
/* life cycle                                                                */
/* ------------------------------------------------------------------------- */

/* Creates a context on HIP device `device`.  Replaces the constructors
 * ov_msckf::UpdaterMSCKF::UpdaterMSCKF (UpdaterMSCKF.cpp:42-56: stores the
 * options, builds the FeatureInitializer and the chi2 table for dof 1..499)
 * and ov_core::FeatureInitializer::FeatureInitializer
 * (FeatureInitializer.h:88).  Fails with OVGPU_ERR_NO_DEVICE when no GPU is
 * present: there is no CPU fallback.                                         */
int ovgpu_create(const ovgpu_options *opts, int device, ovgpu_ctx **out);
void ovgpu_destroy(ovgpu_ctx *ctx);

/* Last HIP / library error text for this thread (never NULL). */
const char *ovgpu_last_error(void);

/* 0.95 chi-square quantile for `dof` degrees of freedom — the table entry the
 * reference gets from boost::math::quantile(chi_squared(dof), 0.95)
 * (UpdaterMSCKF.cpp:52-55, :219-220).  Host-side, no GPU needed.             */
double ovgpu_chi2_quantile_95(int dof);

/* Uploads the state snapshot (covariance, clone / calibration tables) and
 * builds the clone-camera pose table of UpdaterMSCKF.cpp:97-115
 * (R_GtoCi = R_ItoC R_GtoIi, p_CiinG = p_IiinG - R_GtoCi^T p_IinC).
 * The data stay resident in HBM until the next ovgpu_set_state.              */
int ovgpu_set_state(ovgpu_ctx *ctx, const ovgpu_state_view *st);

/* Uploads a batch of feature tracks (host pointers) and keeps it resident.
 * What depends on the batch and on the state's column map alone is derived
 * here, once, behind the copies on the context's stream (the anchor
 * measurement of every track by FeatureInitializer.cpp:36-46's rule, the
 * clone-major order of a track's measurements, the column blocks each tile of
 * 16 Jacobian rows touches): updates on the resident batch do not repeat it.  */
int ovgpu_set_features(ovgpu_ctx *ctx, const ovgpu_features_view *fv);

/* ------------------------------------------------------------------------- */
/* ov_core::FeatureInitializer                                               */
/* ------------------------------------------------------------------------- */

/* Runs single_triangulation / single_triangulation_1d
 * (FeatureInitializer.cpp:30-112 / :114-195) followed, when
 * refine_features is set, by single_gaussnewton (:197-375) on every resident
 * feature, exactly the loop of UpdaterMSCKF.cpp:117-142.
 *   p_FinA, p_FinG   [3*F]  Feature::p_FinA / p_FinG
 *   anchor_meas      [F]    index (into the flat measurement arrays) of the
 *                           anchor measurement: its cam_idx / clone_idx are
 *                           Feature::anchor_cam_id / anchor_clone_timestamp
 *   status           [F]    OVGPU_FEAT_USED (= success so far),
 *                           _TOO_FEW_MEAS, _TRI_FAILED or _GN_FAILED
 * All outputs are host pointers; any may be NULL.
 * The kernel keeps the pose of every (camera, clone) pair in LDS, 96 bytes
 * a pair: a rig with 96 * K * C beyond the workgroup's LDS (160 KB: 1706
 * pairs) is refused with OVGPU_ERR_CAPACITY by this and every other entry
 * that triangulates, before anything is launched.                            */
int ovgpu_triangulate(ovgpu_ctx *ctx, double *p_FinA, double *p_FinG,
                      int32_t *anchor_meas, int32_t *status);

/* The direct input of ov_core::FeatureInitializer: the camera pose of every (camera, clone) pair, i.e. the
 * clonesCAM argument of single_triangulation / single_gaussnewton (FeatureInitializer.h:100-122, ClonePose :51-82)
 * as the caller computed it, instead of a state snapshot.  R_GtoC [K*C*9] row-major, p_CinG [K*C*3], pair (k, c) at
 * index k*C + c.  After this call only ovgpu_set_features and ovgpu_triangulate are usable (no covariance is
 * resident) until the next ovgpu_set_state.                                                                      */
int ovgpu_set_camera_poses(ovgpu_ctx *ctx, int C, int K, const double *R_GtoC, const double *p_CinG);

/* FeatureInitializer::single_gaussnewton ALONE (FeatureInitializer.cpp:197-375): the Levenberg-Marquardt refinement of the
 * resident features started from the caller's estimates p_FinA_in (3 doubles per feature, in the frame of the anchor
 * measurement anchor_meas_in[f]) instead of from the library's own linear triangulation — for callers that seed
 * Feature::p_FinA themselves.  Outputs as ovgpu_triangulate (the anchor is the one passed in).  refine_features of the
 * context must be set; an anchor outside the feature's measurements fails that feature.                              */
int ovgpu_refine(ovgpu_ctx *ctx, const double *p_FinA_in, const int32_t *anchor_meas_in, double *p_FinA,
                 double *p_FinG, int32_t *status);

/* Reads back what the triangulation stage of the LAST pipeline call on the current features left on the device
 * (ovgpu_msckf_compress / _update / ovgpu_slam_delayed_init triangulate internally): p_FinA / p_FinG (3 doubles per
 * feature) and the anchor measurement index, the values the reference stores on the Feature
 * (FeatureInitializer.cpp:45-46, :109-110, :333-335).  Saves the separate ovgpu_triangulate call (and the second
 * triangulation it would cost) when a caller wants both the compressed system and the Feature side effects.
 * Any pointer may be NULL.  Entries of features that failed triangulation are unspecified. */
int ovgpu_get_triangulation(ovgpu_ctx *ctx, double *p_FinA, double *p_FinG, int32_t *anchor_meas);

/* Supplies the feature positions instead of triangulating them: the updates that
 * follow (until the next ovgpu_set_features) skip the triangulation stage and use
 * these values.  This is the situation of UpdaterSLAM::update, where the landmark
 * estimate comes out of the state (UpdaterSLAM.cpp:326-353), and what the stage-wise
 * parity tests use.  p_FinG [3*F] is required; p_FinA [3*F] and anchor_meas [F] are
 * needed for anchored representations; status [F] (NULL = all OVGPU_FEAT_USED).
 * Host pointers.                                                                  */
int ovgpu_set_triangulation(ovgpu_ctx *ctx, const double *p_FinA, const double *p_FinG,
                            const int32_t *anchor_meas, const int32_t *status);

/* ------------------------------------------------------------------------- */
/* ov_msckf::UpdaterMSCKF::update  (UpdaterMSCKF.cpp:58-295)                  */
/* ------------------------------------------------------------------------- */

/* Mode B (whole update on the GPU): triangulate + refine, build and
 * nullspace-project every feature's Jacobian, chi2-gate against the prior,
 * compress the stacked system, and apply StateHelper::EKFUpdate
 * (StateHelper.cpp:116-197).  Operates on the resident state and features.
 *   feat_status [F]     ovgpu_feat_status per feature (NULL ok)
 *   chi2        [F]     gate statistic, NaN when the gate was not reached
 *   chi2_thresh [F]     chi2_multipler * table[rows]
 *   p_FinG      [3*F]   triangulated positions (Feature::p_FinG)
 *   dx          [N]     correction vector K*res (the caller applies
 *                       Type::update to variables the GPU does not hold)
 *   P_out       [N*N]   updated covariance
 * The resident covariance, clone and calibration tables are updated in place
 * (box-plus of JPLQuat.h:114-125 / PoseJPL.h:74-91 / Vec.h:55-58), FEJ values
 * untouched, so a following call sees the posterior, as VioManager's
 * successive updater calls do (VioManager.cpp:525-547).
 * The device does not factor the stack on this call: it accumulates [H | r]^T [H | r] on the matrix cores
 * and applies the update in coordinates whitened by the prior (same dx, P' as compress -> EKFUpdate;
 * DESIGN.md section 4).  ovgpu_options::compress_route = OVGPU_COMPRESS_TSQR keeps the reference's order
 * (nothing in the library reads the environment).                                           */
int ovgpu_msckf_update(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2,
                       double *chi2_thresh, double *p_FinG, double *dx,
                       double *P_out, ovgpu_update_stats *stats);

/* UpdaterMSCKF::update (VioManager.cpp:525) on a state that carries SLAM landmarks, in the resident
 * frame loop: ovgpu_msckf_update with the landmarks kept current on the device.  It replaces, for
 * such a state, the update itself (UpdaterMSCKF.cpp:144-283: an MSCKF feature has no landmark
 * column), StateHelper::EKFUpdate's walk over the state's variables (StateHelper.cpp:188-196) where
 * it reaches the landmarks, and Landmark::update (Landmark.h:55-62, Landmark.cpp:130-140) — which a
 * caller of ovgpu_msckf_update has to do on the host from dx, followed by ovgpu_set_landmarks.
 * ORDER: ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks(ctx, NULL, 0) — no
 * landmark has a Jacobian column —, ovgpu_set_features with the MSCKF batch, this call.
 *   feat_status, chi2, chi2_thresh, p_FinG, dx, P_out, stats   as ovgpu_msckf_update; dx and P_out
 *                       cover all N rows, the landmarks' among them
 *   lm_out      [3*L]   the corrected landmark values (NULL ok); arrives with the same single
 *                       synchronisation as dx and P_out
 * The update is UpdaterMSCKF::update over the calibration and clone columns.  Every resident
 * landmark value is then corrected on the device, in the same stream pass: value += dx[id .. id +
 * dof), a single-depth landmark's LAST stored value takes dx[id].  FEJ values, anchors and
 * representations stay.  Afterwards the landmarks are resident and current: a following SLAM call
 * needs ovgpu_set_active_landmarks and its batch, not ovgpu_set_landmarks.
 * The correction is predicated on the device exactly as the box-plus of the clones is, through the
 * fall-backs of ovgpu_msckf_update (Householder route after a prior block that is not positive
 * definite, step-wise Cholesky after a follower's time-out): an update the device skipped leaves the
 * landmarks untouched, the repeat corrects them once, and on an error return the landmarks are in
 * the state the clones are in.
 * ROUTE: with a global or an anchored MSCKF representation (the anchored ones since
 * k_feat_rows_anchored, unless "anchored_fast" = 0), no per-feature sigma / multiplier and tracks
 * within the fused kernels' limits (per length class under "feat_classes" = 1) the call runs
 * what a landmark-free state of the same N runs — rows laid out once, when the batch is handed
 * over under the empty set; the one-kernel-per-feature path; the
 * Gram-form update; the prior block's factorisation started by ovgpu_set_features on the second
 * stream — and returns that state's bits.  Otherwise it takes the general per-feature kernel as
 * ovgpu_msckf_update does, and corrects the landmarks all the same.  ovgpu_msckf_update on the
 * same context keeps the general kernel.
 * With L == 0 the call IS ovgpu_msckf_update.  Every check runs before anything changes:
 * OVGPU_ERR_NO_STATE (no state, no batch); OVGPU_ERR_INVALID when landmarks are resident and the
 * batch was laid out under a non-empty active set (the message names the calls to make).
 * Not in every libovgpu.so that reports ABI 10: resolve it by symbol.                          */
int ovgpu_msckf_update_lm(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2, double *chi2_thresh,
                          double *p_FinG, double *dx, double *P_out, double *lm_out,
                          ovgpu_update_stats *stats);

/* Mode A (strict drop-in): same pipeline up to and including
 * UpdaterHelper::measurement_compress_inplace (UpdaterHelper.cpp:456-487) and
 * returns the compressed system so that the caller feeds the stock
 * StateHelper::EKFUpdate.
 *   D_out          number of columns
 *   col_cov_id [D] covariance index of every column of H (canonical order)
 *   H   [rows*D]   compressed Jacobian
 *   r   [rows]     compressed residual
 *   rows_out       <= D
 * H, r, col_cov_id must hold Dmax = 6*C + 14*K columns / rows.
 * What EKFUpdate needs from (H, r) is H^T H and H^T r (StateHelper.cpp:131-160 uses H only through H P H^T, P H^T
 * and H^T-weighted residuals), and both forms below carry the stack's:
 *   default (OVGPU_COMPRESS_GRAM)  the diagonally pivoted Cholesky factor of the prior-whitened stack's Gram
 *                                  matrix, un-whitened: DENSE, rows = its numerical rank (the stack of an MSCKF
 *                                  update has a null space: gauge directions) — 1.2 ms host to host at 2000 features
 *   OVGPU_COMPRESS_TSQR            the reference's form, the upper-triangular Householder factor, rows = D
 *                                  (4.0 ms); also taken beyond 383 columns (255 before ABI 5; beyond 511 under
 *                                  ovgpu_debug_option "mode_a_wide" = 1) and when the prior block's factorisation fails.  ovgpu_last_update_route tells which one came back.
 * Which kernels the default form runs, by the column count D (LD = D + 1 with the residual column, NT = ceil(LD / 16)
 * tile columns; ovgpu_debug_option "last_gram_kernel" / "last_factor_kernel" / "last_unwhiten_kernel" report them):
 *   Gram matrix   D <= 255 (NT <= 16): the one-pass kernel with ceil(NT / 2) * 2 tile columns (15 at NT = 15);
 *                 D = 352 .. 367 (NT = 23): k_gram_wide, two passes; D = 256 .. 351 and 368 .. 383: k_gram_blk, 8 x 8-tile blocks
 *   factor        D <= 127 (NT <= 8): k_gram_pchol_blk<4, 9, 2>; D = 128 .. 223 (NT <= 14): k_gram_pchol_blk<7, 15, 4>;
 *                 D = 224 .. 383: the rank-one k_gram_pchol<NB>, NB = ceil(LD / 32) = 8 .. 12 ("pchol_blocked" = 0: for every
 *                 D, NB = 1 .. 12), unless "mode_a_panel" is in force (below)
 *   un-whitening  D <= 256 and the prior block factored in one launch: k_unwhiten_blk<16>; D <= 256 otherwise
 *                 (options.no_single_launch_cholesky, "unwhiten_blocked" = 0): k_unwhiten<16>; D = 257 .. 383: k_unwhiten<24>
 *   D >= 384      none of them: the Householder triangle, rows = D, OVGPU_COMPRESS_TSQR — unless ovgpu_debug_option "mode_a_wide" = 1
 *                 is in force on a float64 context (options.gram_fp32 = 0) with the whitened stack: then, for D = 384 .. 511 (NT = 25 .. 32),
 *                 Gram matrix k_gram_blk over four column windows; factor k_pchol_panel (32 pivots per launch) around k_pchol_schur
 *                 ("last_factor_kernel" 3); un-whitening k_unwhiten_blk<32> on the inverse diagonal tiles of the prior block's two-panel
 *                 factorisation ("last_unwhiten_kernel" 4), or on k_uinv_tiles' when that factorisation ran step-wise
 *                 (options.no_single_launch_cholesky, "chol_wide" = 0) or "unwhiten_blocked" is 0 (5); rows = the numerical rank,
 *                 OVGPU_COMPRESS_PCHOLQR.  ovgpu_slam_compress keeps the Householder triangle at every width, unless ovgpu_debug_option
 *                 "slam_mode_a" is in force: then the table above is its own (D counts the active landmarks' columns), with one difference:
 *   un-whitening  (ovgpu_slam_compress under "slam_mode_a") D = 257 .. 383: k_unwhiten_blk<24>, the blocked form with six accumulator tiles per
 *                 wavefront, on the inverse diagonal tiles of the prior block's two-panel factorisation ("last_unwhiten_kernel" 6), or on
 *                 k_uinv_tiles' when that factorisation ran step-wise (options.no_single_launch_cholesky, "chol_wide" = 0) or
 *                 "unwhiten_blocked" is 0 (7).  ovgpu_msckf_compress keeps k_unwhiten<24> (3) there, unless "mode_a_panel" is in force.
 *   factor        (either entry under ovgpu_debug_option "mode_a_panel" = 1) D = 256 .. 383 (NT = 17 .. 24; the lower edge is one constant
 *                 of the library, MODE_A_PANEL_MIN_NT = 17 tile columns: at 15 and 16 the rank-one k_gram_pchol<8> measured no slower):
 *                 k_pchol_panel (32 pivots per launch) around k_pchol_schur ("last_factor_kernel" 3).  Under the switch
 *                 ovgpu_msckf_compress takes ovgpu_slam_compress's un-whitening at D = 257 .. 383 (6 / 7).  Every other width keeps
 *                 its kernels.
 * A batch whose every feature is rejected returns rows = 0 and OVGPU_OK. */
int ovgpu_msckf_compress(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2,
                         double *chi2_thresh, double *p_FinG, int32_t *D_out,
                         int32_t *rows_out, int32_t *col_cov_id, double *H,
                         double *r, ovgpu_update_stats *stats);

/* Reads back the resident posterior tables after ovgpu_msckf_update.
 * Any pointer may be NULL.  Sizes as in ovgpu_state_view.                    */
int ovgpu_get_state(ovgpu_ctx *ctx, double *P, double *clone_q_p,
                    double *calib_q_p, double *intrinsics);


/* ------------------------------------------------------------------------- */
/* ov_msckf::UpdaterSLAM::update  (UpdaterSLAM.cpp:253-479)                   */
/* ------------------------------------------------------------------------- */

/* SLAM landmarks that live in the state (State::_features_SLAM, ov_type::Landmark,
 * ov_core/src/types/Landmark.h), all in one representation `feat_rep` (StateOptions
 * feat_rep_slam; 0 = GLOBAL_3D, the reference default, StateOptions.h:89) or — feat_rep_each —
 * each in its own (Landmark::_feat_representation: ArUco corners are initialised in
 * StateOptions::feat_rep_aruco, the others in feat_rep_slam, and UpdaterSLAM::update reads the
 * representation from the landmark, UpdaterSLAM.cpp:336-341).
 *   p_value [3*L]  Landmark::value()  — REPRESENTATION coordinates (xyz, (theta, phi, rho) or
 *                  (alpha, beta, rho), Landmark.cpp:66-141); the library applies
 *                  Landmark::get_xyz (Landmark.cpp:25-62) where the reference does
 *                  (UpdaterSLAM.cpp:345-353).  ANCHORED_INVERSE_DEPTH_SINGLE: the 1-dof
 *                  landmark is handed over as (uv_norm_zero.x, uv_norm_zero.y, value()(0)) —
 *                  its constant bearing and its inverse depth (Landmark.cpp:57-60, :124-140);
 *                  only the third entry is a state variable and ever changes
 *   p_fej   [3*L]  Landmark::fej(), same convention
 *   cov_id  [L]    Type::id() of the landmark in the covariance (3 dof; 1 for the single depth)
 *   anchor_cam, anchor_clone [L]  Landmark::_anchor_cam_id and the clone index (into the
 *                  state view's clone arrays) of _anchor_clone_timestamp; read for the anchored
 *                  representations only (may be NULL otherwise)                          */
typedef struct {
  int32_t L;
  int32_t feat_rep; /* ovgpu_feat_rep of every landmark of the view */
  const double *p_value;
  const double *p_fej;
  const int32_t *cov_id;
  const int32_t *anchor_cam;
  const int32_t *anchor_clone;
  const int32_t *feat_rep_each; /* optional [L]: ovgpu_feat_rep per landmark; NULL = feat_rep for all (ABI 7).
                                 * A 3-dof landmark takes 3 covariance ids / columns, a single-depth one 1; the
                                 * anchors of the global ones are not read                                     */
} ovgpu_landmarks_view;

/* Uploads the landmarks the next ovgpu_slam_update works on; their 3 columns each join the
 * canonical column order (sorted by covariance id).  Call after ovgpu_set_state.
 * L is bounded by 4096 and by the memory of the N x N covariance that holds the landmarks;
 * the number of Jacobian COLUMNS is bounded per SLAM call, not here: a call over more than 511
 * (calibration + 6 per clone + the dof of every landmark that has columns) returns
 * OVGPU_ERR_CAPACITY.  With 30 clones, stereo and online calibration that is 101 landmarks
 * with columns at a time: name the ones a call needs with ovgpu_set_active_landmarks.        */
int ovgpu_set_landmarks(ovgpu_ctx *ctx, const ovgpu_landmarks_view *lm);

/* The active landmark set: the resident landmarks that get Jacobian columns in the SLAM calls
 * that follow.  UpdaterSLAM::update builds Hx_order from the variables its batch's features
 * touch (UpdaterSLAM.cpp:300-340), and delayed_init gives resident landmarks no column at all
 * (UpdaterSLAM.cpp:147-239, StateHelper.cpp:393-482): every other landmark is corrected
 * through the covariance alone.  The same here — the column order narrows to the calibrated
 * camera variables, the clones and the n landmarks lm_index names (by covariance id, as
 * before); a landmark outside the set has no column and still receives its share of dx.  In
 * exact arithmetic the results equal those over all landmarks (columns that are zero for the
 * whole stack change nothing); in floating point they differ at rounding level.
 *   n == 0  the empty set: what ovgpu_slam_delayed_init, ovgpu_slam_init_systems(_len) and
 *           ovgpu_slam_change_anchor(s) need;  n < 0  every resident landmark again.
 *   lm_index [n]  indices into the landmark view; one named twice is in the set once.
 * Holds until the next ovgpu_set_landmarks, ovgpu_set_state or call with n < 0.  Landmarks
 * appended by ovgpu_slam_delayed_init are outside it; ovgpu_state_marginalize of a landmark
 * removes it and the set follows the indices of the others.
 * ORDER: ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks,
 * ovgpu_set_features, the SLAM call.  The batch's layout depends on the column count, so a
 * batch uploaded before this call is no longer resident: the SLAM call returns
 * OVGPU_ERR_NO_STATE until ovgpu_set_features is called again (n < 0 without a set in force
 * changes nothing and keeps the batch).  ovgpu_slam_update / _compress return
 * OVGPU_ERR_INVALID for a batch that observes a landmark outside the set, and
 * ovgpu_slam_update / _compress / _delayed_init / _init_systems(_len) return
 * OVGPU_ERR_CAPACITY when the set in force (all landmarks when none was named) has more than
 * 511 columns; until one that fits is named no landmark has a column.
 * ovgpu_slam_change_anchor(s) read no column table and run under any set.
 * The tables are built on the device in one launch on the context's stream; the call does
 * not wait for it.                                                                          */
int ovgpu_set_active_landmarks(ovgpu_ctx *ctx, int32_t n, const int32_t *lm_index);

/* UpdaterSLAM::update on the resident state, landmarks and feature tracks: feature f observes
 * landmark lm_index[f].  Per feature the Jacobian of UpdaterHelper::get_feature_jacobian_full
 * with the landmark's own columns appended (UpdaterSLAM.cpp:369-384, no nullspace projection
 * for a full 3-dof landmark), the chi2 gate on all 2m rows against the prior with the
 * landmark's covariance (:390-420, dof = 2m), stacking (:427-447) and one EKF update (:470).
 * A single-depth landmark contributes its depth column only: the two bearing columns of H_f are
 * projected out of [H_x | h_rho] and the residual (:371-379), 2m - 2 rows and dof = 2m - 2; a
 * track with one measurement leaves no row and is flagged OVGPU_FEAT_TOO_FEW_MEAS.
 * The context's options are the UpdaterSLAM's (sigma_pix, chi2_multipler of `slam`).
 * The reference stacks without compressing; here the stack goes through the same TSQR as the
 * MSCKF update first — the EKF result is the same matrix (QR is an orthogonal transform of
 * the rows).  Features with no measurement are flagged OVGPU_FEAT_TOO_FEW_MEAS (:289-291).
 *   feat_status, chi2, chi2_thresh [F];  dx [N];  P_out [N*N];  lm_out [3*L] updated
 *   landmark values in representation coordinates (Landmark::update, Landmark.h:80-89:
 *   additive).  The landmarks stay resident: a following ovgpu_slam_update /
 *   ovgpu_slam_delayed_init continues from the updated values.
 * With ovgpu_debug_option "slam_fused" = 1 (default 0) a batch whose landmarks are all 3-dof and whose
 * longest track holds at most 62 measurements takes its per-feature stage as ONE fused kernel
 * (S0 = Y Y^T + sigma^2 I from the whitened rows Y = H L the stack holds anyway): the same update to
 * rounding, this entry and ovgpu_slam_update_chunked alike.  At level 2 a batch that observes
 * single-depth landmarks takes it as well (the bearing's projection inside the same kernel); at
 * level 3 so does a batch whose longest track holds 63 to 126 measurements.  */
int ovgpu_slam_update(ovgpu_ctx *ctx, const int32_t *lm_index, int32_t *feat_status,
                      double *chi2, double *chi2_thresh, double *dx, double *P_out,
                      double *lm_out, ovgpu_update_stats *stats);

/* Every chunk of one frame's SLAM update in ONE device pass.  The reference calls
 * UpdaterSLAM::update once per chunk of max_slam_in_update features (VioManager.cpp:529-547),
 * chunk k + 1 linearised at the state chunk k left.  The result is that of this chain, for
 * k = 0 .. n_chunks - 1, on a state carried from chunk to chunk:
 *   1. ovgpu_set_active_landmarks with the distinct landmarks of
 *      lm_index[chunk_first[k] .. chunk_first[k + 1]);
 *   2. ovgpu_set_features with that range of the batch (and that range's per-feature sigma and
 *      multiplier, ovgpu_set_feature_options);
 *   3. ovgpu_slam_update —
 * per-feature status, chi2 and thresholds, dx of every chunk, the final P', clone, calibration
 * and intrinsic values, and every landmark (those no chunk observes are corrected through
 * their rows of P, as in the single call).  The same kernels run on the same inputs as in the
 * chain; what the chain pays per chunk besides — the host walk of the columns, the batch's
 * uploads, the blocking upload of lm_index, a read-back and its synchronisation — is paid once:
 * one upload, one gather, one synchronisation.
 * ORDER: ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_features with the WHOLE frame's SLAM
 * batch (chunks are contiguous feature ranges), optionally ovgpu_set_feature_options, this call.
 *   n_chunks >= 1;  chunk_first [n_chunks + 1]  first feature of every chunk, chunk_first[0] = 0,
 *                   chunk_first[n_chunks] = F, not decreasing; an empty chunk does nothing (its
 *                   dx row is zero, its stats are zero)
 *   lm_index [F];  feat_status, chi2, chi2_thresh [F];  dx_seq [n_chunks][N] or NULL;
 *   P_out [N*N];  lm_out [3*L];  stats [n_chunks] or NULL (ms_* are 0: the pass records no
 *   stage events)
 * n_chunks == 1 is one ovgpu_slam_update under the batch's own active set.  All six landmark
 * representations in any mix and the per-feature options behave as in the single call.
 * Every check runs before anything changes, with the single call's codes: OVGPU_ERR_INVALID
 * (null or decreasing chunk_first, a table that does not span [0, F], an index out of range),
 * OVGPU_ERR_NO_STATE (no state, no landmarks, no batch), OVGPU_ERR_CAPACITY — the message names
 * the chunk — when a chunk's column set exceeds 511 columns.
 * ON RETURN the active set in force is "all", as after ovgpu_set_active_landmarks(n < 0) — so,
 * as there, the batch has to be handed over again before another SLAM call — and
 * ovgpu_get_triangulation answers for the whole batch as uploaded.
 * A chunk whose flag word is set (a prior block that fails its pivot test, a Cholesky follower
 * that timed out, a negative diagonal) is seen at the one synchronisation: the entry state is
 * put back from a device copy and the chunks run one by one with the single call's fall-backs.
 * OVGPU_ERR_NEGATIVE_DIAGONAL in chunk k then leaves the state as the chain would, and the
 * per-feature outputs up to chunk k are written.  ovgpu_debug_option "slam_chunked_fallbacks"
 * counts these passes.
 * Not in every libovgpu.so that reports ABI 10: resolve it by symbol.                          */
int ovgpu_slam_update_chunked(ovgpu_ctx *ctx, int32_t n_chunks, const int32_t *chunk_first,
                              const int32_t *lm_index, int32_t *feat_status, double *chi2,
                              double *chi2_thresh, double *dx_seq, double *P_out, double *lm_out,
                              ovgpu_update_stats *stats);

/* Mode A of the SLAM update (strict drop-in): everything of ovgpu_slam_update up to the
 * compressed stack, returned for the stock StateHelper::EKFUpdate exactly as
 * ovgpu_msckf_compress does.  The landmark columns appear in col_cov_id with the landmarks'
 * covariance ids.  H, r, col_cov_id must hold 6*C + 14*K + 3*L columns / rows.
 * By default the Householder triangle at every width: rows = D (0 when nothing was used),
 * OVGPU_COMPRESS_TSQR.  With ovgpu_debug_option "slam_mode_a" = 1, set after ovgpu_create, the
 * entry takes the pivoted Gram route on the terms ovgpu_msckf_compress does (the rule there): a
 * float64 context on OVGPU_COMPRESS_GRAM with the whitened stack, D <= 383 (D <= 511 when
 * "mode_a_wide" = 1 is in force as well) and a prior block that factors ("mode_a_panel" picks
 * the factor kernel at D = 256 .. 383 for this entry as well).  rows = the numerical
 * rank, at most the rows of the stack plus noise rows; ovgpu_last_update_route reports
 * OVGPU_COMPRESS_PCHOLQR.  The per-feature stage is then the one ovgpu_slam_update runs:
 * k_slam_y for a batch laid out under "slam_fused" ("last_feature_kernel" 4 / 5 / 6 / 7), the
 * general kernel writing whitened rows otherwise.  Rows are scaled to the context's sigma_pix
 * whatever ovgpu_set_feature_options gave (R = sigma_pix^2 I holds on both routes).  The resident
 * state is untouched.  A batch whose every feature is rejected returns rows = 0 and OVGPU_OK.     */
int ovgpu_slam_compress(ovgpu_ctx *ctx, const int32_t *lm_index, int32_t *feat_status,
                        double *chi2, double *chi2_thresh, int32_t *D_out, int32_t *rows_out,
                        int32_t *col_cov_id, double *H, double *r, ovgpu_update_stats *stats);

/* UpdaterSLAM::delayed_init (UpdaterSLAM.cpp:61-251) with StateHelper::initialize /
 * initialize_invertible (StateHelper.cpp:393-577) on the resident state and the uploaded feature
 * tracks: every feature is triangulated against the clone poses at entry (:121-144), then ONE
 * AFTER THE OTHER (each accepted feature changes the state the next one is linearised at):
 * Jacobians (:165), separation of the 2m rows into the 3 rows that determine the landmark and
 * the 2m-3 rows that do not (StateHelper.cpp:429-455; any orthonormal basis gives the same
 * result, here 3 Householder reflectors instead of the Givens sweep), chi2 gate of the latter
 * against chi2_multipler * chi2_0.95(2m) (:459-470), and for an accepted feature the covariance
 * augmentation (:541-565), the landmark's first correction (:569) and StateHelper::EKFUpdate
 * with the 2m-3 rows (:476-478).  The context's options are the UpdaterSLAM's (sigma_pix,
 * chi2_multipler of `slam`).  `feat_rep` = the representation the NEW landmarks get
 * (StateOptions::feat_rep_slam, or feat_rep_aruco for a batch of ArUco corners, UpdaterSLAM.cpp:
 * 206-213); the resident landmarks keep theirs (ABI 7; one representation for all before).
 * ANCHORED_INVERSE_DEPTH_SINGLE:
 * the bearing is projected out first (UpdaterSLAM.cpp:181-196), the third of the three rows
 * initialises the 1-dof landmark and the gate uses the quantile of 2m-2 dof.
 *
 * The covariance grows by s = 3 (1 for the single depth) per accepted feature, in feature order
 * (new ids N, N+s, ...); below, "3*F" in the sizes of dx_seq and P_out reads s*F.
 * Outputs (any may be NULL):
 *   feat_status, chi2, chi2_thresh [F]   as ovgpu_msckf_update (chi2 rejected ->
 *                                        OVGPU_FEAT_CHI2_REJECTED)
 *   lm_cov_id [F]     covariance id given to the feature's landmark, -1 if not initialised
 *   lm_value, lm_fej [3*F]  Landmark::value() / fej() in representation coordinates AFTER the
 *                     whole call (later features' updates included)
 *   anchor_cam, anchor_clone [F]   anchor of the triangulation (Feature::anchor_cam_id and the
 *                     clone index of anchor_clone_timestamp)
 *   dx_seq [F * (N + 3*F)]  row f = the state correction of feature f's EKFUpdate (zero when it
 *                     was rejected), for the variables the library does not hold (IMU, time
 *                     offset ...): apply the rows in order
 *   N_out             new covariance dimension N + 3 * n_accepted
 *   P_out [(N + 3*F)^2 capacity]   the N_out x N_out covariance, row-major with stride N_out
 * Afterwards the resident state has dimension N_out and the accepted landmarks are resident
 * (appended to those of ovgpu_set_landmarks); upload the next feature batch with
 * ovgpu_set_features before another feature update.                                       */
int ovgpu_slam_delayed_init(ovgpu_ctx *ctx, int32_t feat_rep, int32_t *feat_status, double *chi2,
                            double *chi2_thresh, int32_t *lm_cov_id, double *lm_value,
                            double *lm_fej, int32_t *anchor_cam, int32_t *anchor_clone,
                            double *dx_seq, int32_t *N_out, double *P_out,
                            ovgpu_update_stats *stats);

/* ovgpu_slam_delayed_init with every candidate's step fused: same inputs, outputs, ordering rules (triangulation once at entry,
 * candidate f linearised at the state candidates 0 .. f-1 left, StateHelper::initialize's gate, growth by 3 or 1 per accepted
 * candidate, a rejected candidate leaves the state bit for bit untouched), checks (all before anything changes) and error codes.
 * Per candidate the chain of about eleven launches and two clears becomes five launches and no clear (csrc/k_init_fused.h): the
 * system and its gate; ONE product [G ; A2_x] P(cols, :) on the matrix cores that serves initialize_invertible and EKFUpdate
 * both; the innovation covariance next to the appended columns; its Cholesky factorisation with the carried columns; one tail
 * (covariance with its new rows / columns, dx, box-plus, landmarks, the new landmark, counters, pose tables).  No host
 * synchronisation inside the chain.  The results agree with ovgpu_slam_delayed_init's to rounding (the products are summed in
 * another order), not bit for bit.
 * Bound of the fused step: tracks of m <= 64 measurements (2m - 3 <= 125 projected rows).  A longer candidate takes
 * ovgpu_slam_delayed_init's step where it stands in the chain and the chain goes on; so does every candidate when
 * ovgpu_options::no_single_launch_cholesky is set or ovgpu_debug_option "delayed_init_fused" is 0 (then the outputs are
 * ovgpu_slam_delayed_init's bit for bit).  "delayed_init_fused_steps" / "delayed_init_chain_steps" count the candidates of this
 * entry by the step they took.  A time-out of the factorisation's bounded waits is reported as OVGPU_ERR_HIP, as there.
 * At level 2 of "delayed_init_fused" (default 1) chi2 is the statistic of the projected system's own factorisation,
 * |U^-T res2|^2 with S = A2 P A2^T + sigma^2 I = U^T U: the same number to rounding, the verdicts identical for a candidate
 * that does not sit on its threshold.  A rejected candidate then costs the step's first four launches (the system's rows, the
 * two products, the factorisation) where level 1 pays the per-feature kernel alone; a candidate whose triangulation failed
 * costs neither.  "delayed_init_rows_steps" counts the candidates that took the step at level 2.
 * With ovgpu_debug_option "delayed_init_fused_long" = 1 (default 0) the bound of the fused step is m <= 232 measurements, at either
 * level: up to 129 measurements (2m - 3 <= 256) the step is the same five launches, from 130 on its factorisation is two panels
 * around a Schur step (eight launches and the clears of the step words; where "chol_wide" is 0 such a candidate takes
 * ovgpu_slam_delayed_init's step).  Candidates of m <= 64 run what they run without the switch, bit for bit; m >= 233 takes
 * ovgpu_slam_delayed_init's step in place.  "delayed_init_long_steps" counts the fused candidates of more than 64 measurements.
 * Callers find the entry by symbol (ABI 10).                                                                      */
int ovgpu_slam_delayed_init_fused(ovgpu_ctx *ctx, int32_t feat_rep, int32_t *feat_status, double *chi2,
                                  double *chi2_thresh, int32_t *lm_cov_id, double *lm_value,
                                  double *lm_fej, int32_t *anchor_cam, int32_t *anchor_clone,
                                  double *dx_seq, int32_t *N_out, double *P_out,
                                  ovgpu_update_stats *stats);

/* Mode A of UpdaterSLAM::delayed_init (UpdaterSLAM.cpp:61-251): the chain of ovgpu_slam_delayed_init run
 * SPECULATIVELY, every feature's system exported in the form the stock StateHelper::initialize
 * (StateHelper.cpp:393-481) takes, so that an unpatched reference applies them itself.  Inputs as
 * ovgpu_slam_delayed_init (resident state and landmarks, the uploaded batch, feat_rep,
 * ovgpu_set_feature_reps / _options, ovgpu_set_triangulation).  The triangulation runs once at entry
 * (:121-144); feature f is linearised at the state the chain reached when it got there (:147-239:
 * UpdaterHelper::get_feature_jacobian_full after the previous features' initialize), as the reference
 * linearises it — provided the host's gate decisions agree with the device's (`status`).
 *
 * first_feature = k restarts the chain at feature k from the state resident NOW: features before k
 * produce nothing (status -1).  After the host decided feature f differently, it uploads its own state
 * (ovgpu_set_state / _landmarks / _features, the options, and ovgpu_set_triangulation with the entry
 * triangulation and its anchors) and calls with first_feature = f + 1.
 *
 * No side effect on the resident state: P, clones, calibration, intrinsics, landmarks and the feature
 * batch are what they were before the call (the chain works on copies); the triangulation of the call
 * stays readable through ovgpu_get_triangulation.
 *
 * Per feature f, sys[f] (all F entries are written):
 *   status        the device's decision: OVGPU_FEAT_USED (passed the gate, initialised in the chain),
 *                 OVGPU_FEAT_CHI2_REJECTED, or the triangulation's failure; -1 for f < first_feature
 *   feat_rep      the representation the feature is initialised in
 *   rows, cols_f  rows of H_x / H_f / res and columns of H_f: 2m x 3, or (2m - 2) x 1 for
 *                 ANCHORED_INVERSE_DEPTH_SINGLE after the bearing projection (:181-196); rows = 0: no
 *                 system (status neither USED nor CHI2_REJECTED)
 *   n_vars, h     Hx_order = var_id / var_size [var_off .. var_off + n_vars): (covariance id, size) of
 *                 the clones, extrinsics and intrinsics the Jacobian touches, by covariance id; h = the
 *                 sum of the sizes
 *   H_x [hx_off .. + rows * h], H_f [hf_off .. + rows * cols_f], res [res_off .. + rows]: row-major.  An
 *                 orthogonal transform of the reference's rows: [R1; 0] as H_f with Q^T [H_x | res]
 *                 (initialize is invariant under it up to rounding); R = sigma_pix_f^2 I
 *   chi2, chi2_thresh   the device's gate (NaN without a system)
 *   anchor_cam, anchor_clone   the triangulation's anchor (Feature::anchor_cam_id, the clone of
 *                 anchor_clone_timestamp)
 *   p_seed[3]     what Landmark::set_from_xyz receives (:213-221): p_FinA for an anchored
 *                 representation, p_FinG otherwise
 * The ragged arrays are sized by ovgpu_slam_init_systems_len (same batch, feat_rep, first_feature);
 * OVGPU_ERR_CAPACITY when `cap` is smaller.  stats->n_used = features the device accepted.          */
typedef struct {
  int64_t n_vars; /* entries of var_id / var_size */
  int64_t n_hx;   /* doubles of H_x                */
  int64_t n_hf;   /* doubles of H_f                */
  int64_t n_res;  /* doubles of res                */
} ovgpu_init_sizes;

typedef struct {
  int32_t status, feat_rep, rows, cols_f, n_vars, h, anchor_cam, anchor_clone;
  int64_t var_off, hx_off, hf_off, res_off;
  double chi2, chi2_thresh;
  double p_seed[3];
} ovgpu_init_system;

int ovgpu_slam_init_systems_len(ovgpu_ctx *ctx, int32_t feat_rep, int32_t first_feature,
                                ovgpu_init_sizes *sizes);
int ovgpu_slam_init_systems(ovgpu_ctx *ctx, int32_t feat_rep, int32_t first_feature,
                            const ovgpu_init_sizes *cap, ovgpu_init_system *sys, int32_t *var_id,
                            int32_t *var_size, double *H_x, double *H_f, double *res,
                            ovgpu_update_stats *stats);

/* Landmarks resident after ovgpu_slam_update / ovgpu_slam_delayed_init: L_out = count,
 * value / fej [3*L] (representation coordinates), cov_id / anchor_cam / anchor_clone [L]. */
int ovgpu_get_landmarks(ovgpu_ctx *ctx, int32_t *L_out, double *value, double *fej,
                        int32_t *cov_id, int32_t *anchor_cam, int32_t *anchor_clone);

/* ... and their representations, feat_rep [L] (ovgpu_feat_rep; ABI 7).                      */
int ovgpu_get_landmark_reps(ovgpu_ctx *ctx, int32_t *L_out, int32_t *feat_rep);

/* UpdaterSLAM::perform_anchor_change (UpdaterSLAM.cpp:506-647) for the resident anchored landmark
 * lm_index: its position is re-expressed in the camera `new_anchor_cam` of clone `new_anchor_clone`
 * (value and first estimate, :536-571), and the covariance is propagated with
 * Phi = H_f_new^-1 [H_x_old | H_f_old | -H_x_new] through StateHelper::EKFPropagation (:612-640;
 * the single depth uses the pseudo-inverse of its 3 x 1 Jacobian, :619).
 * OVGPU_ERR_INVALID for a global representation.                                            */
int ovgpu_slam_change_anchor(ovgpu_ctx *ctx, int32_t lm_index, int32_t new_anchor_cam,
                             int32_t new_anchor_clone);

/* UpdaterSLAM::change_anchors (UpdaterSLAM.cpp:481-504): every resident landmark anchored in clone
 * `marg_clone` (the one about to be marginalised) moves to clone `new_clone` (the newest, the
 * reference passes state->_timestamp), same camera.  n_changed (optional) = how many moved.  */
int ovgpu_slam_change_anchors(ovgpu_ctx *ctx, int32_t marg_clone, int32_t new_clone,
                              int32_t *n_changed);

/* The same call in a fixed number of launches (ABI 10): one kernel forms the transition matrix Phi_l,
 * the new value / first estimate and the new anchor of EVERY moving landmark at the entry state
 * (perform_anchor_change builds Phi from state values alone, and no anchor change moves a clone or a
 * calibration), three more apply the joint StateHelper::EKFPropagation whose transition matrix has
 * the block rows Phi_l.  Contract, checks and error codes are ovgpu_slam_change_anchors'; the
 * covariance differs from its result by the rounding of another order of summation and is exactly
 * symmetric.  ovgpu_slam_change_anchors itself launches per landmark, as before.                  */
int ovgpu_slam_change_anchors_batched(ovgpu_ctx *ctx, int32_t marg_clone, int32_t new_clone,
                                      int32_t *n_changed);

/* Mode A of UpdaterSLAM::change_anchors (ABI 10), shaped like ovgpu_slam_init_systems: what
 * perform_anchor_change hands to StateHelper::EKFPropagation (:612-640) and writes into the landmark
 * (:642-646), for every resident landmark anchored in `marg_clone`, in landmark order.  The resident
 * state (P, landmarks, anchors, column map, a pending prior factorisation) is left exactly as it was:
 * the host replays the systems through the stock EKFPropagation(state, {landmark}, phi_order_OLD,
 * Phi, Q = 0), one landmark after the other.  Each Phi depends on state values only, so the replay
 * in order reproduces the reference's sequence.  Per landmark (ovgpu_anchor_system):
 *   lm_index, cov_id   the landmark (index into the landmark view, covariance id); lsz = 3, or 1 for the single depth
 *   n_vars, n_old      phi_order_OLD = var_id / var_size [var_off .. var_off + n_vars) in the REFERENCE's order (:592-610): old
 *                      anchor clone, old extrinsics (if estimated), new anchor clone, new extrinsics (if estimated and
 *                      another camera), the landmark; n_old = the sum of the sizes
 *   Phi [phi_off .. + lsz * n_old]   row-major
 *   value / fej [3 * k .. 3 * k + 3) of system k   the landmark in its new anchor, representation coordinates as
 *                      ovgpu_get_landmarks gives them (single depth: bearing x, bearing y, rho)
 *   anchor_cam, anchor_clone   the new anchor
 * The arrays are sized by ovgpu_slam_anchor_systems_len (same state, marg_clone, new_clone): sys / value / fej by
 * n_sys, var_id / var_size by n_vars, Phi by n_phi; OVGPU_ERR_CAPACITY when `cap` is smaller.  Without an anchored
 * landmark both return OVGPU_OK with all sizes 0.  A resident state and landmarks are all they need.             */
typedef struct {
  int64_t n_sys;  /* moving landmarks               */
  int64_t n_vars; /* entries of var_id / var_size   */
  int64_t n_phi;  /* doubles of Phi                 */
} ovgpu_anchor_sizes;

typedef struct {
  int32_t lm_index, cov_id, lsz, feat_rep, n_vars, n_old, anchor_cam, anchor_clone;
  int64_t var_off, phi_off;
} ovgpu_anchor_system;

int ovgpu_slam_anchor_systems_len(ovgpu_ctx *ctx, int32_t marg_clone, int32_t new_clone,
                                  ovgpu_anchor_sizes *sizes);
int ovgpu_slam_anchor_systems(ovgpu_ctx *ctx, int32_t marg_clone, int32_t new_clone,
                              const ovgpu_anchor_sizes *cap, ovgpu_anchor_system *sys, int32_t *var_id,
                              int32_t *var_size, double *Phi, double *value, double *fej);

/* Per-feature landmark representation for ovgpu_slam_delayed_init on the uploaded batch: UpdaterSLAM::delayed_init
 * initialises an ArUco corner in StateOptions::feat_rep_aruco and every other feature in feat_rep_slam
 * (UpdaterSLAM.cpp:160-166).  feat_rep [F] (ovgpu_feat_rep); NULL = the call's feat_rep argument for every feature.
 * The covariance then grows by 3 or 1 per accepted feature as each one's representation says.  Until the next batch is
 * uploaded (ABI 7).                                                                                         */
int ovgpu_set_feature_reps(ovgpu_ctx *ctx, const int32_t *feat_rep);

/* Per-feature measurement noise and gate multiplier for the uploaded batch — UpdaterSLAM keeps two
 * UpdaterOptions, `slam` and `aruco`, and picks per feature by its id (UpdaterSLAM.cpp:227-232,
 * :392-409).  sigma_pix / chi2_multipler [F] (either may be NULL = the context's value for every
 * feature).  Applies to the SLAM update, the delayed initialisation and the MSCKF update alike,
 * until the next batch is uploaded.  The rows of a feature enter the stacked system scaled by
 * sigma_ctx / sigma_f, i.e. the returned compressed system (mode A) has the context's sigma.  */
int ovgpu_set_feature_options(ovgpu_ctx *ctx, const double *sigma_pix, const double *chi2_multipler);

/* ------------------------------------------------------------------------- */
/* Window bookkeeping on the RESIDENT covariance: the steps either   */
/* side of the update, so that P does not cross PCIe between frames.  The means of the    */
/* variables the library does not hold (IMU, time offset ...) stay with the caller.       */
/* After each call the feature batch has to be uploaded again (ovgpu_set_features): clone  */
/* indices and covariance ids changed.                                                     */
/* ------------------------------------------------------------------------- */

/* StateHelper::marginalize (StateHelper.cpp:271-339): removes rows / columns
 * [cov_id, cov_id + size) of the covariance; every resident variable behind it moves forward by
 * `size` (:320-323).  When a resident clone or landmark starts at cov_id it is dropped — the
 * clones / landmarks behind it move down by one INDEX as well (StateHelper::marginalize_old_clone,
 * marginalize_slam, :618-651); a calibration variable at cov_id stops being estimated.      */
int ovgpu_state_marginalize(ovgpu_ctx *ctx, int32_t cov_id, int32_t size);

/* The same for n blocks in ONE device pass (StateHelper::marginalize_slam drops every lost
 * landmark of a frame, :618-651): three launches and one ovgpu_state_marginalize's worth of
 * table rebuilding whatever n is, where the chain pays a covariance copy, up to six record
 * shifts and a host wait per block.
 *   cov_id, size [n]  blocks of the covariance AS IT IS AT ENTRY (not the ids a chain of single
 *                     calls would see after its earlier removals), in any order
 * Per block the rules of ovgpu_state_marginalize hold; in addition the blocks must not overlap or
 * repeat (OVGPU_ERR_INVALID), and a landmark anchored in a clone that leaves is legal only if
 * that landmark leaves in the same call.  At least one clone must remain.  Every check runs
 * before anything is modified: a refused call leaves the context as it was.  n == 0 is a no-op.
 * Afterwards the context is in the state the chain would have left (ids shifted, anchors
 * renumbered to the new clone indices, the active landmark set following the landmarks' indices).
 * The covariance is SELECTED, P'[i][j] = P[keep[i]][keep[j]]: no value is touched.  (A chain of
 * single calls takes the lower-left block of every step from the upper-right one, :303-304; the
 * two agree bit for bit on a covariance that is symmetric bit for bit.)
 * Not in every libovgpu.so that reports ABI 10: resolve it by symbol.                          */
int ovgpu_state_marginalize_batched(ovgpu_ctx *ctx, int32_t n, const int32_t *cov_id,
                                    const int32_t *size);

/* StateHelper::clone of a 6-dof pose at the end of the covariance (StateHelper.cpp:341-391) plus
 * the time-offset part of StateHelper::augment_clone (:601-615).
 *   src_cov_id   id of the pose being cloned (State::_imu->pose(), or any 6-dof pose)
 *   q_p, q_p_fej [7]  value and first estimate of the new clone (PoseJPL::clone copies both)
 *   dt_cov_id    id of the camera time offset, -1 when it is not calibrated (:601)
 *   dnc_dt [6]   [last_w ; v_I] (:603-605), read when dt_cov_id >= 0
 *   new_cov_id   out: id of the new clone (the old covariance dimension); its clone index is the
 *                old clone count                                                           */
int ovgpu_state_augment_clone(ovgpu_ctx *ctx, int32_t src_cov_id, const double *q_p,
                              const double *q_p_fej, int32_t dt_cov_id, const double *dnc_dt,
                              int32_t *new_cov_id);

/* StateHelper::EKFPropagation (StateHelper.cpp:36-114): P(new, :) = Phi P(old, :), P(new, new) =
 * Phi P(old, old) Phi^T + Q for the contiguous block [new_cov_id, new_cov_id + n_new).
 *   old_cov_ids [n_old]  covariance index of every COLUMN of Phi (the flattened order_OLD)
 *   Phi [n_new * n_old] row-major, Q [n_new * n_new] (its upper triangle is used, :87)
 * OVGPU_ERR_NEGATIVE_DIAGONAL mirrors the reference's exit on a negative diagonal (:101-113): the
 * WHOLE diagonal of the covariance is scanned, not only the propagated block's — a negative
 * entry that ovgpu_set_state accepted outside the block is reported here.  The covariance has
 * been written by then, as in the reference.                                                  */
int ovgpu_state_propagate(ovgpu_ctx *ctx, int32_t new_cov_id, int32_t n_new, int32_t n_old,
                          const int32_t *old_cov_ids, const double *Phi, const double *Q);

/* StateHelper::get_marginal_covariance (StateHelper.cpp:226-258) on the RESIDENT covariance:
 * out [n x n, row-major] = P restricted to the covariance indices cov_idx [n] (any order, e.g. the dofs of
 * the variables of an H_order).  UpdaterZeroVelocity's chi2 test (UpdaterZeroVelocity.cpp:193-203) reads the
 * IMU orientation / bias block this way.                                                                   */
int ovgpu_state_marginal_covariance(ovgpu_ctx *ctx, int32_t n, const int32_t *cov_idx, double *out);

/* Current dimension of the resident covariance and number of resident clones. */
int ovgpu_state_dims(ovgpu_ctx *ctx, int32_t *N_out, int32_t *C_out);

/* ------------------------------------------------------------------------- */
/* A FeatureDatabase on the device: observations are appended once    */
/* per frame, the batch of an update is assembled on the device — the host never walks the   */
/* per-feature maps of ov_core::Feature (Feature.h:49-55) and never re-sends an observation. */
/* The host keeps the id -> slot table and the last observation time of every track.        */
/* ------------------------------------------------------------------------- */

/* Allocates the store: up to max_tracks live tracks of up to max_obs observations each (all
 * cameras together).  Replaces FeatureDatabase's constructor; call again to resize (drops all). */
int ovgpu_tracks_create(ovgpu_ctx *ctx, int32_t max_tracks, int32_t max_obs);

/* FeatureDatabase::update_feature (FeatureDatabase.cpp:59-85) for the n observations of one camera
 * frame: feature featid[i] was seen by camera cam_id[i] at `timestamp` at raw pixel uv[2i..] /
 * normalised uvn[2i..].  Unknown ids open a new track.  OVGPU_ERR_CAPACITY when the store or a
 * track is full (nothing is appended then).                                                  */
int ovgpu_tracks_append(ovgpu_ctx *ctx, double timestamp, int32_t n, const int64_t *featid,
                        const int32_t *cam_id, const float *uv, const float *uvn);

/* Drops tracks (Feature::to_delete + FeatureDatabase::cleanup, FeatureDatabase.cpp:211-224);
 * unknown ids are ignored.                                                                    */
int ovgpu_tracks_erase(ovgpu_ctx *ctx, int32_t n, const int64_t *featid);

/* FeatureDatabase::features_not_containing_newer(timestamp) (FeatureDatabase.cpp:87-126): ids of the
 * tracks whose last observation is older than `timestamp` (the lost tracks VioManager turns into
 * MSCKF features, VioManager.cpp:366-378).  ids [capacity], n_out = how many there are.       */
int ovgpu_tracks_not_containing_newer(ovgpu_ctx *ctx, double timestamp, int32_t capacity,
                                      int64_t *ids, int32_t *n_out);

/* FeatureDatabase::features_containing_older(timestamp) (FeatureDatabase.cpp:128-167): tracks with a camera
 * whose FIRST stored observation is older than `timestamp`; FeatureDatabase::features_containing(timestamp)
 * (FeatureDatabase.cpp:169-209): tracks with an observation AT `timestamp` (exact ==) — with the oldest clone's
 * time, the tracks VioManager marginalises into MSCKF features (VioManager.cpp:376-378).  Same conventions as
 * ovgpu_tracks_not_containing_newer: ids [capacity] ascending, n_out = how many there are (call with
 * capacity 0 to size the array); nothing is removed (the reference's `remove` = false; ovgpu_tracks_erase does
 * that) and there is no to_delete flag on the device (`skip_deleted`: erase what was used).                  */
int ovgpu_tracks_containing_older(ovgpu_ctx *ctx, double timestamp, int32_t capacity,
                                  int64_t *ids, int32_t *n_out);
int ovgpu_tracks_containing(ovgpu_ctx *ctx, double timestamp, int32_t capacity, int64_t *ids,
                            int32_t *n_out);

/* FeatureDatabase::get_oldest_timestamp (FeatureDatabase.cpp:265-276): the smallest FIRST observation time
 * over all tracks and cameras, -1 when the store holds no observation.                                       */
int ovgpu_tracks_oldest_timestamp(ovgpu_ctx *ctx, double *t_out);

/* FeatureDatabase::cleanup_measurements(timestamp) (FeatureDatabase.cpp:226-243, Feature.cpp:84-110): every
 * observation with time <= timestamp leaves (VioManager.cpp:589-591 calls it once per frame with the time of
 * the clone about to be marginalised: this is what keeps a long-lived track inside max_obs); _exact
 * (FeatureDatabase.cpp:245-263, Feature.cpp:55-82; UpdaterZeroVelocity.cpp:257): every observation with time ==
 * timestamp leaves.  A track left without observations is dropped (:236-238).  n_erased (may be NULL): how
 * many tracks were dropped.  The survivors keep their order.                                                  */
int ovgpu_tracks_cleanup_measurements(ovgpu_ctx *ctx, double timestamp, int32_t *n_erased);
int ovgpu_tracks_cleanup_measurements_exact(ovgpu_ctx *ctx, double timestamp, int32_t *n_erased);

/* FeatureDatabase::get_feature_clone (FeatureDatabase.cpp:41-57): the stored observations of one track in the
 * order they were appended (per camera = the order of Feature::timestamps[cam]).  n_out = their number (0 for
 * an unknown id); the first min(n_out, capacity) are written to timestamps [capacity], cam_id [capacity],
 * uv / uvn [2 * capacity] (any of them may be NULL).                                                          */
int ovgpu_tracks_get_feature(ovgpu_ctx *ctx, int64_t featid, int32_t capacity, int32_t *n_out,
                             double *timestamps, int32_t *cam_id, float *uv, float *uvn);

/* ---- VioManager::retriangulate_active_tracks (VioManagerHelper.cpp:190-387), SURVEY.md row N4 -------------
 * The running linear triangulation of the tracks alive in the newest frame.  Per call = per camera frame:
 * the n newest observations (TrackBase::get_last_obs / get_last_ids), grouped by camera in the order of
 * CameraData::sensor_ids, WITHOUT the features that are SLAM landmarks (:248-250: the state estimate takes
 * priority; the caller appends those from the state, :311-327).  cam_id = camera INDEX of the state view,
 * uv = distorted pixel, uvn = CamBase::undistort_cv of it, clone_index = the clone of the frame (:199).
 * The library keeps A, b and the observation count of every track on the device between calls
 * (active_feat_linsys_*, VioManager.h); tracks that are not in this call are dropped (:305-309).
 * Outputs, one entry per distinct track in order of first appearance: out_featid, out_p_FinG (3 doubles, NaN
 * until the track has more than three observations and passes the condition-number / depth checks, :275-299)
 * and out_uvd (pixel in cam0 and depth in the current cam0 frame, NaN unless the track is triangulated, seen
 * by camera index cam0 in this frame, has depth >= 0.1 and lies inside img_w x img_h, :345-379; cam0 = -1:
 * never).  Arrays of capacity n.  max_cond_number / min_dist / max_dist come from the context's options. */
int ovgpu_retriangulate(ovgpu_ctx *ctx, int32_t clone_index, int32_t n, const int64_t *featid,
                        const int32_t *cam_id, const float *uv, const float *uvn, int32_t cam0,
                        int32_t img_w, int32_t img_h, int32_t *n_tracks, int64_t *out_featid,
                        double *out_p_FinG, double *out_uvd);
/* Forgets every running system (a reset of the front end). */
int ovgpu_retriangulate_reset(ovgpu_ctx *ctx);

/* Number of live tracks. */
int ovgpu_tracks_count(ovgpu_ctx *ctx, int32_t *n_tracks);

/* Order of the camera groups inside a track of the assembled batch.  It decides the anchor of a feature:
 * FeatureInitializer.cpp:36-46 iterates Feature::timestamps (a std::unordered_map<size_t, ...>) and keeps the
 * FIRST camera with strictly the most measurements, and for full stereo tracks the counts tie.  libstdc++
 * iterates such a map in REVERSE order of first insertion of its keys.
 *   OVGPU_GROUPS_REFERENCE   (default) exactly that: the store remembers, per track, the order in which cameras
 *                            first observed it (the order of the entries of ovgpu_tracks_append calls) and walks it
 *                            backwards.  The front ends insert camera 0 first (TrackKLT.cpp feed_stereo,
 *                            TrackSIM.cpp:37-63), so this is normally descending camera id and a tie is anchored in
 *                            the highest id; a track first seen by camera 1 alone and later by camera 0 iterates 0, 1.
 *   OVGPU_GROUPS_DESCENDING / _ASCENDING   by camera id, whatever the history.
 * The host-flattened path (shim/ovgpu_flatten.h) walks the map itself and needs no such rule.
 * ASSUMPTION of OVGPU_GROUPS_REFERENCE: the reference is built against libstdc++ and a track's map never
 * rehashes (at most 13 distinct camera keys: the first bucket count).  libc++ / MSVC iterate differently,
 * and a rehash reverses the list again; a host in that situation flattens on its side (it iterates its
 * own map) or passes OVGPU_GROUPS_DESCENDING / _ASCENDING explicitly.                                         */
enum { OVGPU_GROUPS_REFERENCE = 0, OVGPU_GROUPS_DESCENDING = 1, OVGPU_GROUPS_ASCENDING = 2 };
int ovgpu_tracks_group_order(ovgpu_ctx *ctx, int32_t order);

/* Builds the resident feature batch from F stored tracks — what ovgpu_set_features would receive
 * after Feature::clean_old_measurements(clone_times) (Feature.cpp:26-53) and the shim's
 * flattening: observations whose time is (exactly) one of clone_times [C] (index = clone index
 * of the resident state), camera groups in the order of ovgpu_tracks_group_order (default: the
 * reference's iteration order of Feature::timestamps), time order inside a group.
 * An unknown id gives an empty track.  The state must be resident (C clones).
 * The track lengths come back to the host before the batch is laid out, so a batch assembled here
 * follows ovgpu_debug_option "feat_classes" exactly as one handed to ovgpu_set_features does.   */
int ovgpu_tracks_to_features(ovgpu_ctx *ctx, int32_t F, const int64_t *featid,
                             const double *clone_times);

/* Reads the resident feature batch back (any pointer may be NULL): F, M, meas_offsets [F+1],
 * uv / uvn [2M], clone_idx / cam_idx [M].                                                    */
int ovgpu_get_features(ovgpu_ctx *ctx, int32_t *F_out, int32_t *M_out, int32_t *meas_offsets,
                       float *uv, float *uvn, int32_t *clone_idx, int32_t *cam_idx);

/* ------------------------------------------------------------------------- */
/* the two helpers of the path as standalone calls (UpdaterZeroVelocity.cpp:183-321 */
/* and any other updater stack a dense system and call them this way)         */
/* ------------------------------------------------------------------------- */

/* UpdaterHelper::measurement_compress_inplace (UpdaterHelper.cpp:456-487): (rows x cols) H and
 * res (host, row-major) -> the upper-triangular (cols x cols) system with the same H^T H and
 * H^T res; rows <= cols is returned unchanged (:459-460).  H_out holds min(rows, cols) x cols.     */
int ovgpu_measurement_compress(ovgpu_ctx *ctx, int rows, int cols, const double *H,
                               const double *res, double *H_out, double *res_out,
                               int32_t *rows_out);

/* StateHelper::EKFUpdate (StateHelper.cpp:116-197) with R = sigma2 * I on the RESIDENT
 * covariance and pose tables: column j of H (rows x cols, host) is the covariance index
 * col_cov_id[j].  dx [N] and P_out [N*N] as in ovgpu_msckf_update.  Re-upload the feature batch
 * (ovgpu_set_features) before the next feature update: the compression buffers are shared.   */
int ovgpu_ekf_update(ovgpu_ctx *ctx, int rows, int cols, const int32_t *col_cov_id,
                     const double *H, const double *res, double sigma2, double *dx,
                     double *P_out);

/* ------------------------------------------------------------------------- */
/* feature-sharded multi-GPU update                           */
/* ------------------------------------------------------------------------- */

/* Number of doubles of one rank's compressed triangle [R | Q^T r]:
 * Dmax * (Dmax + 1) with Dmax = 6*C + 14*K of the resident state.            */
int ovgpu_triangle_len(ovgpu_ctx *ctx, int64_t *n_doubles);

/* Stage 1 on every rank: everything of ovgpu_msckf_update up to the local
 * compression of this rank's feature shard; the local triangle stays in HBM.
 * `tri_dev` (DEVICE pointer, ovgpu_triangle_len doubles, may be NULL)
 * receives a copy so that the caller can hand it to RCCL
 * (torch.distributed.all_gather_into_tensor).                                */
int ovgpu_msckf_local(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2,
                      double *chi2_thresh, double *p_FinG, void *tri_dev,
                      ovgpu_update_stats *stats);

/* Stage 2: `tris_dev` (DEVICE pointer) holds G gathered triangles; they are
 * re-compressed by one more QR (QR of stacked R factors = R of the full
 * stack) and the EKF update is applied to the resident state.  Every rank
 * calls it with identical data and obtains identical dx / P_out.             */
int ovgpu_msckf_merge_update(ovgpu_ctx *ctx, const void *tris_dev, int G,
                             double *dx, double *P_out,
                             ovgpu_update_stats *stats);

/* The same exchange in Gram form (k_gram.h): every GPU accumulates G_g = [H_g | r_g]^T [H_g | r_g] of its
 * shard, the shards' sum is ONE all-reduce of ovgpu_gram_len() doubles (a 16 ceil((D+1)/16) square, row
 * major, + 1 trailing double = the accepted-row count), and every rank factors the sum and applies
 * the identical update.  Needs D <= 383 (OVGPU_ERR_CAPACITY beyond, from all three calls, the state untouched); a rank
 * whose shard is empty hands out zeros and takes the summed matrix as the other ranks' whitened one.  A follower time-out of the
 * single-launch Cholesky (ovgpu_msckf_update_sharded below) makes ovgpu_msckf_gram_update and ovgpu_msckf_merge_update return OVGPU_ERR_HIP:
 * no update was applied.  ovgpu_msckf_gram_update leaves the state untouched and may be called again with the same buffer; after
 * ovgpu_msckf_merge_update's, upload the state again (ovgpu_set_state / ovgpu_reset_state) before the call is repeated.  The caller falls back to the triangle exchange above when
 * the summed row count is below 4 (D + 1) (short stacks: see DESIGN.md section 4).  Replaces the
 * same stretch of UpdaterMSCKF::update as ovgpu_msckf_local / ovgpu_msckf_merge_update.            */
int ovgpu_gram_len(ovgpu_ctx *ctx, int64_t *n_doubles);
int ovgpu_msckf_local_gram(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2, double *chi2_thresh,
                           double *p_FinG, void *gram_dev, ovgpu_update_stats *stats);
int ovgpu_msckf_gram_update(ovgpu_ctx *ctx, const void *gram_dev, double *dx, double *P_out,
                            ovgpu_update_stats *stats);

/* ------------------------------------------------------------------------- */
/* camera models                                                              */
/* ------------------------------------------------------------------------- */

/* Evaluates the device camera model on n normalized points (host arrays):
 * CamBase::distort_d (CamBase.h:130-135 -> CamRadtan::distort_f, CamRadtan.h:127-146,
 * or CamEqui::distort_f, CamEqui.h:136-158, including the float round trip) and
 * compute_distort_jacobian (CamRadtan.h:154-198 / CamEqui.h:166-230).
 *   cam8 [8] fx fy cx cy d0..d3 ; uv_norm [2n] ; uv_dist [2n] ; dz_dzn [4n] ; dz_dzeta [16n]
 * Used by the parity tests of the camera row; outputs may be NULL. */
int ovgpu_cam_distort(ovgpu_ctx *ctx, int is_fisheye, const double *cam8, int n,
                      const double *uv_norm, double *uv_dist, double *dz_dzn,
                      double *dz_dzeta);

/* ------------------------------------------------------------------------- */
/* benchmarking hooks                                                         */
/* ------------------------------------------------------------------------- */

/* Re-uploads the prior (covariance + pose tables) saved by the last
 * ovgpu_set_state from a device-side copy, so that repeated timed updates all
 * start from the same prior with inputs already resident in HBM.             */
int ovgpu_reset_state(ovgpu_ctx *ctx);

/* Enqueues one complete update (as ovgpu_msckf_update) on the context's
 * stream without any host read-back or synchronisation.  Its status
 * (OVGPU_ERR_NOT_SPD, OVGPU_ERR_NEGATIVE_DIAGONAL) is returned by the next
 * ovgpu_synchronize.  Unlike ovgpu_msckf_update it cannot repeat the update through
 * the Householder route when the prior block of the involved variables is
 * numerically singular: the state is then left untouched and NOT_SPD reported.  */
int ovgpu_msckf_update_async(ovgpu_ctx *ctx);

/* Blocks until the context's stream is idle; returns the status of a preceding
 * ovgpu_msckf_update_async. */
int ovgpu_synchronize(ovgpu_ctx *ctx);

/* hipStream_t of the context, as an integer (for hipEvent timing). */
uint64_t ovgpu_stream(ovgpu_ctx *ctx);

/* ------------------------------------------------------------------------- */
/* Multi-GPU.  Features shard across GPUs, one exchange: the   */
/* Gram matrices of the (identically whitened) shards add, so the exchange is */
/* ONE all-reduce of (16 ceil((D+1)/16))^2 doubles over RCCL / xGMI on the    */
/* context's stream; every GPU then applies the identical update.  With the   */
/* Householder route (or more than 383 columns: 24 tile columns of [H | r],  */
/* whatever "gram_wide" says) the D x (D+1) triangles are all-gathered and    */
/* merged instead.  RCCL is loaded at run time.                               */
/* ------------------------------------------------------------------------- */
typedef struct { char internal[128]; } ovgpu_comm_id; /* = ncclUniqueId */

/* One process per GPU (torchrun / MPI): rank 0 draws an id, the host program distributes the 128 bytes by its own means, every
 * rank joins.  world == 1 is valid (no collective is issued). */
int ovgpu_comm_unique_id(ovgpu_comm_id *id);
int ovgpu_comm_init_rank(ovgpu_ctx *ctx, const ovgpu_comm_id *id, int rank, int world);
int ovgpu_comm_destroy(ovgpu_ctx *ctx);
/* rank / world as ovgpu_comm_init_rank was told, and as the RCCL communicator itself reports them (ncclCommUserRank / ncclCommCount;
 * -1 without a communicator): evidence for a multi-GPU run's log that the collective spans the ranks it is believed to span. */
int ovgpu_comm_info(ovgpu_ctx *ctx, int32_t *rank_told, int32_t *world_told, int32_t *rccl_rank, int32_t *rccl_ranks);

/* UpdaterMSCKF::update of THIS rank's shard (uploaded with ovgpu_set_features on the replicated state): local stage, exchange and
 * update are enqueued back to back on the context's stream, no host synchronisation in between.  Per-feature outputs are the
 * shard's; dx / P_out are identical on every rank.  _async returns after enqueueing (status through ovgpu_synchronize).
 * Errors: OVGPU_ERR_NOT_SPD conditions of the (replicated) prior are repeated through the Householder route on every rank alike.
 * A follower time-out of the single-launch Cholesky (a scheduling event of ONE rank; since round 5 the carried columns' workgroups are
 * blocks of the factor workgroup's own launch, placed behind it, so it takes a wedged device or the test knob to see one) is NOT
 * repeated in a world of more than one rank -- a local repeat would issue a collective the peers never match: OVGPU_ERR_HIP is
 * returned, this rank's state is untouched while the peers have applied the update, and the caller uploads the state again on every
 * rank (ovgpu_multi_msckf_update: the same, detected for the whole set).  options.no_single_launch_cholesky = 1 rules it out.
 * ovgpu_last_update_route reports the exchange the call took: OVGPU_COMPRESS_GRAM, or OVGPU_COMPRESS_TSQR for the triangles. */
int ovgpu_msckf_update_sharded(ovgpu_ctx *ctx, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out,
                               ovgpu_update_stats *stats);
int ovgpu_msckf_update_sharded_async(ovgpu_ctx *ctx);

/* One host process driving several GPUs (the reference's host is ONE C++ process: VioManager.cpp:155-156, :518-526).
 * devices == NULL: 0 .. n-1.  set_features deals the tracks round-robin by length (stable sort by descending length, rank g holds
 * every n-th from the g-th on, in ascending order of the caller's indices); the update returns every output in the caller's feature
 * order.  A device may be named more than once, up to 8 times (OVGPU_ERR_CAPACITY beyond, nothing is left allocated): those ranks
 * share the device and exchange through the library's loop-back collective, and are driven through ovgpu_multi_msckf_update alone
 * (ovgpu_msckf_update_sharded[_async] on one of them returns OVGPU_ERR_INVALID).
 * ovgpu_multi_msckf_update does NOT repeat an update: a prior block that does not factor on the Gram exchange returns
 * OVGPU_ERR_NOT_SPD for the set, and every rank's state is left as it was uploaded, bit for bit (the prior is replicated: every rank
 * skipped the same kernels).  Such a filter selects compress_route = OVGPU_COMPRESS_TSQR, whose exchange needs no factor of the prior.
 * ovgpu_last_update_route of a rank (ovgpu_multi_ctx) reports the exchange the set took. */
typedef struct ovgpu_multi ovgpu_multi;
int ovgpu_multi_create(const ovgpu_options *opts, int n, const int *devices, ovgpu_multi **out);
void ovgpu_multi_destroy(ovgpu_multi *m);
int ovgpu_multi_size(ovgpu_multi *m);
ovgpu_ctx *ovgpu_multi_ctx(ovgpu_multi *m, int i);
int ovgpu_multi_set_state(ovgpu_multi *m, const ovgpu_state_view *st);
int ovgpu_multi_set_features(ovgpu_multi *m, const ovgpu_features_view *fv);
int ovgpu_multi_msckf_update(ovgpu_multi *m, int32_t *feat_status, double *chi2, double *chi2_thresh, double *p_FinG, double *dx, double *P_out,
                             ovgpu_update_stats *stats);

/* Which route the last ovgpu_msckf_update / ovgpu_slam_update took: OVGPU_COMPRESS_GRAM, or OVGPU_COMPRESS_TSQR when it was
 * selected or when the prior block failed the pivot test of the Gram route (ovgpu_options::prior_pivot_tol). */
int ovgpu_last_update_route(ovgpu_ctx *ctx);

/* Developer / test aid (no reference counterpart): reads (old_value, may be NULL) and, with value >= 0, sets a named internal.
 *   "chol_follow_spin_limit"  wait bound of the single-launch Cholesky's follower workgroups (k_chol.h); 0 makes every follower
 *                             give up at once, which the tests use to exercise the recovery: the kernels behind the factorisation
 *                             are switched off on the device, the state stays untouched and the synchronous update calls repeat
 *                             the update with the step-wise kernels
 *   "chol_timeouts"           (read only) number of updates repeated that way
 *   "chol_wide"               (default 1) a Cholesky-with-carry factorisation of 257 .. 512 columns runs as two panels of the single-launch
 *                             kernel around a Schur step, four launches (k_chol_wide.h), in every update entry point, with no lower bound on
 *                             the second panel's width (measured faster from 257 columns on); 0: one launch per 16 rows up
 *                             there (the same result to rounding).  ovgpu_options::no_single_launch_cholesky = 1 and the repeat after a
 *                             follower's time-out select the step-wise kernels at every column count
 *   "chol_wide_factorisations" number of factorisations ENQUEUED on the two-panel path, counted on the host: one that a predicate switches off on the
 *                             device counts too (a value >= 0 sets the counter)
 *   "gram_wide"               (default 0) a level; the read-back returns it (values above 1 are taken as 1).
 *                             1: a float64 context (options.gram_fp32 = 0) on compress_route = OVGPU_COMPRESS_GRAM takes the whitened Gram route of
 *                             mode B at 384 .. 511 Jacobian columns as well: ovgpu_msckf_update, ovgpu_msckf_update_lm, ovgpu_slam_update and
 *                             ovgpu_slam_update_chunked stack Y = H L, k_gram_blk forms Y^T Y over four column windows of 128 (ten block pairs;
 *                             "last_gram_kernel" 2), both factorisations are two-panel ones ("chol_wide"), and the fused per-feature kernels are
 *                             taken on the terms they have below 384 columns ("last_feature_kernel", "slam_fused").  0: such updates take the
 *                             Householder route, as without the switch.  Whatever the level: mode A (ovgpu_msckf_compress, ovgpu_slam_compress;
 *                             ovgpu_msckf_compress has a switch of its own, "mode_a_wide"), a gram_fp32 context, the local-Gram, sharded and multi-GPU entries and the speculative prior keep 383 columns, the
 *                             stack beyond 383 columns is the projected one, and more than 511 columns are refused.  The fall-backs are the
 *                             route's own: a failed prior pivot repeats through the Householder route, options.no_single_launch_cholesky,
 *                             "chol_wide" = 0 and the repeat after a follower's time-out factor step-wise on the Gram route.  Takes effect with
 *                             the next ovgpu_set_state / ovgpu_set_features (ovgpu_tracks_to_features hands a batch over as well) and at no
 *                             other call: a batch that is resident keeps the level it was handed over under
 *   "gram_wide_updates"       (read only) number of updates that took the Gram route beyond 383 columns and stand, once per update (per chunk of
 *                             ovgpu_slam_update_chunked): an attempt the library repeats — through the Householder route after a failed prior
 *                             pivot, with the step-wise Cholesky after a time-out, a chunked pass that is put back — is not counted, nor is an
 *                             update that returns an error (ovgpu_msckf_update_async alone counts when it enqueues)
 *   "mode_a_wide"             (default 0) a level; the read-back returns it (values above 1 are taken as 1).  Independent of "gram_wide".
 *                             1: ovgpu_msckf_compress on a float64 context (options.gram_fp32 = 0) whose compress_route is not OVGPU_COMPRESS_TSQR
 *                             takes the pivoted Gram route at 384 .. 511 Jacobian columns as well (the rule at ovgpu_msckf_compress):
 *                             ovgpu_last_update_route reports OVGPU_COMPRESS_PCHOLQR and rows = the numerical rank.  0: such compressions return
 *                             the Householder triangle, as without the switch.  Whatever the level: ovgpu_slam_compress (it has a switch of
 *                             its own, "slam_mode_a"; with both in force it takes the route at 384 .. 511 columns too), compress_route =
 *                             OVGPU_COMPRESS_TSQR, a gram_fp32 context and an un-whitened stack keep the Householder triangle, every update entry
 *                             keeps its route, and more than 511 columns are refused.  A prior block that does not factor (or a follower's
 *                             time-out) repeats the call through the Householder route.  Takes effect where "gram_wide" does: with the next
 *                             ovgpu_set_state / ovgpu_set_features, and at no other call
 *   "mode_a_wide_compressions" (read only) number of compressions that took the pivoted route beyond 383 columns and stand: an attempt the
 *                             library repeats through the Householder route is not counted
 *   "slam_mode_a"             (default 0) a level; the read-back returns it (values above 1 are taken as 1).
 *                             1: ovgpu_slam_compress on a float64 context (options.gram_fp32 = 0) whose compress_route is not OVGPU_COMPRESS_TSQR
 *                             takes the pivoted Gram route up to 383 Jacobian columns (511 when "mode_a_wide" = 1 is in force as well), by the
 *                             rule at ovgpu_msckf_compress: ovgpu_last_update_route reports OVGPU_COMPRESS_PCHOLQR and rows = the numerical rank.
 *                             Its per-feature stage is ovgpu_slam_update's ("slam_fused", "last_feature_kernel"), its un-whitening at D = 257 ..
 *                             383 k_unwhiten_blk<24> ("last_unwhiten_kernel" 6 / 7).  0: the Householder triangle, as without the switch.
 *                             Whatever the level: compress_route = OVGPU_COMPRESS_TSQR, a gram_fp32 context and an un-whitened stack keep the
 *                             Householder triangle, so do more than 383 columns without "mode_a_wide"; every other entry keeps its route and its
 *                             bits; more than 511 columns are refused.  A prior block that does not factor (or a follower's time-out) repeats
 *                             the call through the Householder route with the bits of a context that never named the switch.  Takes effect
 *                             where "mode_a_wide" does: with the next ovgpu_set_state / ovgpu_set_features, and at no other call: a batch that
 *                             is resident keeps the level it was handed over under
 *   "slam_mode_a_compressions" (read only) number of SLAM compressions that took the pivoted route and stand: an attempt the library repeats
 *                             through the Householder route is not counted
 *   "mode_a_panel"            (default 0) a level; the read-back returns it (values above 1 are taken as 1).  Independent of "mode_a_wide" and
 *                             "slam_mode_a".  Where a compression takes the pivoted Gram route anyway (ovgpu_msckf_compress on a float64 context
 *                             with the whitened stack whose compress_route is not OVGPU_COMPRESS_TSQR and whose prior block factors;
 *                             ovgpu_slam_compress on the same terms with "slam_mode_a" in force) and D = 256 .. 383 (17 .. 24 tile columns of
 *                             [H | r]), 1: the factor is k_pchol_panel / k_pchol_schur instead of the rank-one k_gram_pchol<9 .. 12>, and
 *                             ovgpu_msckf_compress un-whitens D = 257 .. 383 with k_unwhiten_blk<24>.  0, or
 *                             never named: every entry enqueues what it did before and returns those bits.  Whatever the level: every other
 *                             width, route and entry keeps its kernels and its bits.  A prior block that does not factor repeats the call
 *                             through the Householder route with the bits of a context that never named the switch.  Takes effect where
 *                             "mode_a_wide" does: with the next ovgpu_set_state / ovgpu_set_features, and at no other call
 *   "mode_a_panel_compressions" (read only) number of compressions that took the panelled factor at 256 .. 383 columns and stand: an attempt
 *                             the library repeats through the Householder route is not counted
 *   "tsqr_leaves" / "tsqr_rows_per_node" / "tsqr_last_leaf_kernel" / "tsqr_last_tree" / "tsqr_last_qh"  (read only) what the last Householder
 *                             compression launched, stand-alone (ovgpu_measurement_compress, ovgpu_ekf_update) or on the update route: the number
 *                             of leaves W; the rows per leaf; the leaf kernel (0 the panel-wave kernel of k_tsqr_pw.h, 1 k_qr_node of k_tsqr.h,
 *                             2 k_qr_append; -1 before the first compression); the merge (0 none: one leaf, 1 the single-launch tree next to the
 *                             leaves, 2 the single-launch tree behind them, 3 one launch per level); the merge kernels' quads per register array
 *                             (16, 28 or 32; 0 for k_qr_append and where nothing was merged).  A merge without leaves (ovgpu_msckf_merge_update)
 *                             sets the last two only
 *   "slam_chunked_fallbacks"  number of ovgpu_slam_update_chunked passes that put the entry state back and ran the chunks one by one
 *                             (a value >= 0 sets the counter)
 *   "delayed_init_fused"      (default 1) a level; the read-back returns it (values above 2 are taken as 2).
 *                             0: ovgpu_slam_delayed_init_fused runs ovgpu_slam_delayed_init's step for every candidate
 *                             1: the fused step of five launches; its first, the general per-feature kernel, decides the gate ahead of the step
 *                             2: the fused step with the gate-free k_init_rows as its first launch; the step's tail decides the gate from the
 *                                residual the factorisation of the projected system carries (chi2 = |U^-T res2|^2)
 *   "delayed_init_rows_steps" number of candidates of ovgpu_slam_delayed_init_fused that took the fused step at level 2 (a value >= 0 sets the
 *                             counter); "delayed_init_fused_steps" counts the fused steps of either level
 *   "delayed_init_fused_steps" / "delayed_init_chain_steps"  number of candidates of ovgpu_slam_delayed_init_fused that took the fused step /
 *                             the chain's step (a track beyond the fused step's bound, or the switch above; a value >= 0 sets the counter)
 *   "delayed_init_fused_long" (default 0) 0 / 1; the read-back returns it.  1: under "delayed_init_fused" = 1 or 2 a candidate of
 *                             ovgpu_slam_delayed_init_fused with 65 .. 232 measurements takes the fused step as well: k_init_rows' LDS carve
 *                             grows to 152 704 bytes at 232 measurements, and from 130 measurements on (2m - 3 > 256 projected rows) the
 *                             factorisation runs as two panels around a Schur step (four launches, "chol_wide").  Candidates of 64
 *                             measurements at most keep their launches and their bits; 233 and more take the chain's step in place, and so
 *                             does a candidate of 130 .. 232 where "chol_wide" is 0
 *   "delayed_init_long_steps" number of candidates of ovgpu_slam_delayed_init_fused with more than 64 measurements that took the fused step
 *                             (a value >= 0 sets the counter); "delayed_init_fused_steps" counts them as well
 *   "slam_chunked_fail_chunk" k >= 0: the next ovgpu_slam_update_chunked treats chunk k's flag word as failed after its pass and takes
 *                             that path (one-shot; tests)
 *   "layout_every_update"     1: the integer tables ovgpu_set_features derives once per batch (anchor measurements, clone-major
 *                             positions, column-block lists) are built again at the head of every update — what a timing loop over
 *                             a resident batch has to add to stand for a filter that hands over a new batch per frame
 *   "tri_waves"               features per workgroup of the triangulation kernel, 1 .. 16; 0 (default) = chosen by the batch so that,
 *                             where possible, a few compute units stay free for the prior block's factorisation launched beside it
 *   "stage_timing_period"     n >= 1: the six stage events (ovgpu_update_stats::ms_*, ovgpu_kernel_times) go into every n-th update
 *                             only (each is a marker packet the next kernel waits for, ~5 us); updates without events report 0
 *   "stack_is_f32"            (read only) the last pipeline stored the stack as floats and ran k_gram_f32 (options.gram_fp32)
 *   "raw_stack"               (round 6, default 1) the Gram route of ovgpu_msckf_update stacks the UNPROJECTED whitened rows in regions by column reach and
 *                             subtracts the Gram matrix of the rows the nullspace projection drops (k_gram.h: k_gram_regions) — same H^T H, H^T r to rounding;
 *                             0: the projected rows of rounds 2-5; takes effect with the next ovgpu_set_state / ovgpu_set_features.  Mode A
 *                             (ovgpu_msckf_compress), the fp32 variant, the Householder route and batches assembled by ovgpu_tracks_to_features
 *                             always stack projected rows.  ("raw_work_const": the region work model's constant; 2: one region, developer experiments)
 *   "last_stack_raw"          (read only) the last pipeline's Gram matrix came from the unprojected stack
 *   "last_feature_kernel"     (read only) per-feature kernel of the last batch pipeline (enum FeatKernel, csrc/api_context.inc): 0 the general one, 1 / 2 the one-pass fused shapes, 3 the block-row one,
 *                             4 the fused kernel of the SLAM update (k_slam_y.h, under "slam_fused")
 *                             (k_slam_y<false>: no single-depth landmark observed), 5 k_slam_y<true>, the same kernel with the projection of
 *                             single-depth landmarks ("slam_fused" = 2), 6 / 7 the long shapes of k_slam_y<false> / k_slam_y<true>: a batch whose
 *                             longest track holds 63 to 126 measurements ("slam_fused" = 3), 8 / 9 the block-row shapes k_slam_y_big<false> /
 *                             k_slam_y_big<true>: 127 to 232 measurements ("slam_fused_big" = 1 under "slam_fused" = 3)
 *                             Under "feat_classes" = 1 it keeps its meaning: the kernel of the batch's LONGEST track, the first class launched
 *   "feat_classes"            a level, default 0.  0: one per-feature kernel per batch, picked from its longest track — up to 62 observations
 *                             k_feat_y<4, 9, 2>, 63 to 126 k_feat_y<8, 17, 1>, 127 to 232 k_feat_y_big, beyond that the general kernel — so that one
 *                             long track decides for every other.  1: an MSCKF batch laid out for the fast path is partitioned into up to four
 *                             LENGTH CLASSES by the same rule applied per track (csrc/feat_classes.h), each a contiguous range of the slots sorted by
 *                             descending length, and the update launches one kernel per class, longest class first, on the context's stream: each
 *                             track on the smallest shape that holds it.  Tracks of 0 or 1 observations go with the shortest class present (the
 *                             kernels skip them by status).  Every other term of the fast path's eligibility is evaluated once per batch as at
 *                             level 0; the block of the reflector kernel in front is sized by the longest FUSED track, so a track beyond 232
 *                             observations no longer keeps the others off the fused kernels: it alone takes the general kernel.  The stack: a
 *                             batch whose classes are all one-pass kernels keeps the unprojected stack on the terms of "raw_stack"; a batch with
 *                             a block-row or a general class stacks projected rows for all of its classes, as such batches do at level 0.
 *                             The switch acts only with options.feature_kernel_shape = 0, "featy_big" = 0, no_fast_feature_kernel = 0 and on a
 *                             batch whose track lengths the host has: one of ovgpu_set_features or of ovgpu_tracks_to_features.  A batch of one
 *                             class, per-feature sigma / multiplier, the routes without the prior's factor (Householder), options.gram_fp32 next to
 *                             a general class (the general kernel writes no float stack), SLAM batches and the delayed initialisation keep the
 *                             single-kernel rule, launch for launch as at level 0.  What follows the switch without code of its own:
 *                             ovgpu_msckf_update / _async, ovgpu_msckf_update_lm (its eligibility per batch, as before), ovgpu_msckf_compress, the
 *                             local-Gram, sharded and multi entries (every rank partitions its own share).  Outputs: the reference's update to
 *                             rounding; a feature's chi2 is the one its kernel gives at level 0 in a batch that kernel takes, bit for bit.
 *                             Consecutive launches on one stream do not overlap: a class of a few features pays a serial tail (DESIGN.md section 7
 *                             has the measurements; no class is merged into its neighbour).  Takes effect with the next ovgpu_set_features; a
 *                             resident batch keeps the level it was laid out under, as with "slam_fused"
 *   "last_feature_classes"    (read only) bit mask over the FeatKernel codes 0 .. 3 of the kernels the last batch pipeline launched; a single bit
 *                             (the code "last_feature_kernel" reports) whenever one MSCKF kernel took the whole batch; 0 after a fused SLAM batch
 *   "last_class_features_0" .. "last_class_features_3"  (read only) features of the last batch pipeline in the class of that code
 *   "feat_class_batches"      counter: batch pipelines that launched more than one class, once per update that stands — the pipelines of an attempt
 *                             the library repeats (Householder route, step-wise Cholesky) are not counted, the rule of "slam_fused_batches"; a
 *                             value >= 0 sets it
 *   "sys_lds_limit" / "sys_m_lds_max" / "sys_rows_global" / "sys_row_stride" / "sys_lds_bytes"  (read only) the general per-feature kernel's
 *                             LDS carve for the batch in force, as sized with the last ovgpu_set_features (or the entry point that laid the batch out):
 *                             the byte limit of a workgroup's LDS; the largest track length whose gate matrix is LDS-resident (longer tracks of
 *                             the batch keep theirs in a per-workgroup global workspace); 1 when the Jacobian records of a feature live in a global
 *                             workspace too (k_system_t<true>: the longest track's records do not fit LDS next to the T chunk), else 0; the doubles
 *                             per Jacobian record (48; 72 once an anchored representation is in force); the launch's dynamic LDS size in bytes
 *   "last_gram_kernel" / "last_factor_kernel" / "last_unwhiten_kernel"  (read only) what the last batch pipeline launched: the Gram kernel (0 none,
 *                             1 the one-pass kernel, 2 k_gram_blk, 3 k_gram_wide, 4 k_gram_regions, 5 k_gram_f32); mode A's pivoted factor (0 none: the
 *                             Householder triangle, 1 k_gram_pchol_blk<4, 9, 2>, 2 k_gram_pchol_blk<7, 15, 4>, 3 k_pchol_panel + k_pchol_schur, 32 + NB the rank-one
 *                             k_gram_pchol<NB>); mode A's un-whitening (0 none, 1 k_unwhiten_blk<16>, 2 k_unwhiten<16>, 3 k_unwhiten<24>, 4 k_unwhiten_blk<32> on
 *                             the two-panel factorisation's inverse tiles, 5 k_unwhiten_blk<32> on k_uinv_tiles', 6 k_unwhiten_blk<24> on the
 *                             two-panel factorisation's inverse tiles, 7 k_unwhiten_blk<24> on k_uinv_tiles' — ovgpu_slam_compress under
 *                             "slam_mode_a", ovgpu_msckf_compress under "mode_a_panel"): the rule at ovgpu_msckf_compress
 *   "last_gram_workgroups"    (read only) the row shares of that Gram kernel where it is one of the two that options.gram_fp32 reaches: gridDim.x of the
 *                             last pipeline's k_gram_f32 launch (workgroups per part of the macro-tile triangle: max(1, ceil(rows / 1536),
 *                             min(ceil(2 CUs / parts), ceil(rows / 128)))) or k_gram_blk launch (min(CUs, ceil(rows / 32)); a tenth of the CUs at
 *                             25 .. 32 tile columns); 0 for every other Gram kernel, for a pipeline without one and before the first
 *   "slam_fused"              (default 0) a level; the read-back returns it (values above 3 are taken as 3).
 *                             1: ovgpu_slam_update / ovgpu_slam_update_chunked run the per-feature stage of a batch as the fused kernel
 *                             k_slam_y — one sweep Y = H L on the matrix cores feeds the stack and the gate's S0 = Y Y^T + sigma_f^2 I — when every
 *                             landmark the batch observes is 3-dof, its longest track holds at most 62 measurements, 16 <= D, K C <= 8192,
 *                             options.no_fast_feature_kernel is 0 and the update takes the whitened (Gram) route; per-feature sigma_pix /
 *                             chi2_multipler do not disqualify.  Everything else keeps the general kernel: a batch with a single-depth landmark,
 *                             the Householder route (compress_route = OVGPU_COMPRESS_TSQR, more than 383 columns — 511 under "gram_wide" —, the repeat after a failed prior
 *                             pivot), ovgpu_slam_compress (unless "slam_mode_a" puts it on the whitened route: then the terms above hold for it
 *                             as well, at every level), the delayed initialisation.
 *                             2: level 1, and a batch that observes a single-depth landmark (OVGPU_REP_ANCHORED_INVERSE_DEPTH_SINGLE) takes
 *                             k_slam_y<true> when the remaining terms hold (longest track <= 62, 16 <= D, K C <= 8192, no_fast_feature_kernel 0, the
 *                             whitened route): per feature of such a landmark the two reflectors of its bearing columns are applied to the rows
 *                             of [Y | r] on their way to the stack (2m - 2 rows) and the gate is r^T S0^-1 r - g^T G^-1 g at dof 2m - 2, from the
 *                             same sweep; a batch that observes none takes k_slam_y<false> as at level 1, with the same bits.  The fall-backs
 *                             of level 1 stay.
 *                             3: level 2, and a batch whose longest track holds 63 to 126 measurements takes the long shape of the kernel — the
 *                             same algebra on 16 tile rows of the gate matrix (2 m + 4 <= 256 rows) and column blocks of 32 — when the remaining
 *                             terms hold (16 <= D, K C <= 8192, no_fast_feature_kernel 0, the whitened route, its LDS carve within the workgroup's
 *                             limit): "last_feature_kernel" 6 without, 7 with a single-depth landmark observed.  A batch of at most 62 takes the
 *                             shapes of level 2 with their bits (4 / 5); 127 measurements and beyond, and every fall-back of levels 1 and 2, keep
 *                             the general kernel.  Takes effect with the next ovgpu_set_features (a batch over landmarks of both sizes is laid out
 *                             again when a SLAM call names its landmarks: the level in force at that call decides)
 *   "slam_fused_big"          (default 0) a level; the read-back returns it (1 and every value above is taken as 1).  It acts only when
 *                             "slam_fused" is at 3.  1: a batch whose longest track holds 127 to 232 measurements (SLY_MMAX_B, csrc/k_slam_y_big.h)
 *                             takes the block-row shape of the fused kernel, k_slam_y_big — k_slam_y's algebra, the gate matrix factored block
 *                             row by block row in passes of up to 136 tiles as k_feat_y_big does, the records written by a small kernel in front
 *                             of it on the same stream — on the long shape's terms: 16 <= D, K C <= 8192, no_fast_feature_kernel 0, the whitened
 *                             route, its LDS carve within the workgroup's limit.  "last_feature_kernel" 8 without, 9 with a single-depth landmark
 *                             observed; "slam_fused_batches" counts them.  A batch of at most 126 does what level 3 does, with its bits; 233
 *                             measurements and beyond, and every fall-back of level 3, keep the general kernel; wherever level 3 hands the batch's
 *                             fused kernel to another entry (ovgpu_slam_update_chunked, ovgpu_slam_compress under "slam_mode_a", the 384 .. 511
 *                             column routes under "gram_wide" / "mode_a_wide") the block-row shape goes the same way.  A short track of such a
 *                             batch goes through the block-row kernel's single pass: the same update to rounding, not the short shapes' bits.
 *                             Takes effect with the next ovgpu_set_features, as "slam_fused" does
 *   "slam_fused_batches"      counter: batch pipelines that took k_slam_y (either instantiation), once per update — the pipelines of an attempt the library repeats (through the
 *                             Householder route after a failed prior pivot, with the step-wise Cholesky after a time-out) are not counted; a value >= 0 sets it
 *   "anchored_fast"           (default 1) batches of an anchored feat_rep_msckf take the fused per-feature kernels: 48-double records with
 *                             H_f = A dl at the p_FinG the anchor gives and no anchor blocks, which the nullspace projection annihilates
 *                             (k_featy.h: k_feat_rows_anchored) — the same update to rounding; 0: the general kernel with its 72-double
 *                             records, as before; takes effect with the next ovgpu_set_features
 *   "live_allocations" / "live_allocation_bytes"  (read only) the allocations of this library still alive in the PROCESS, device and page-locked
 *                             memory together, and their bytes as requested (a buffer of n elements counts max(n, 1) elements).  The same values
 *                             from any context: a context that was destroyed has given back everything it held, so both return to what they
 *                             were before it was created (tests/test_gpu_context_frees.py)
 *   "upload_arena_bytes"      reads the capacity of the page-locked upload arena of ovgpu_set_state / ovgpu_set_features (8 MB once the first
 *                             of them has run).  A value >= 64 is the size asked for the next time one of them starts; the arena only ever
 *                             grows, so a small arena is had by setting this before the context's first upload.  An array that does not fit
 *                             what is left of the arena bypasses it: it is copied from the caller's memory and the stream is synchronised
 *                             before the call goes on, and the arena is twice what would have fitted (1 GiB at most) from the next call on
 *   "upload_bypasses"         counter: the arrays that bypassed the arena; a value >= 0 sets it
 *   "raw_gram_tile_rows"      (read only) rows x tiles summed over the regions of the resident batch: the 16 x 16 products per row k_gram_regions executes
 *   "speculative_prior"       (round 6, default 1) ovgpu_set_features starts the prior block's factorisation on the second stream, next to its own
 *                             uploads; the update joins it.  0: the factorisation starts with the update (round 5)
 *   "pchol_blocked"           (round 6, default 1) mode A's pivoted Gram factor by the blocked kernel (k_pchol.h, up to 223 Jacobian columns); 0: the
 *                             rank-one kernel of rounds 3-5 everywhere.  Same pivots, same factor at rounding
 *   "unwhiten_blocked"        (round 6, default 1) mode A's X = R L^-1 right-looking with the diagonal tiles' inverses of the prior's factorisation
 *                             (k_unwhiten.h); 0: one wavefront per 16 rows, substitution inside the tiles (rounds 3-5)
 *   "layout_fpw"              (round 6, default 8) features per workgroup of the batch-layout kernel at most (1 .. 8): the launch is kept at 250
 *                             workgroups or fewer where that allows, so that the prior's factorisation finds free compute units
 *   "featy_big"               1 / 2: the block-row form of the per-feature kernel (k_featy_big.h) on batches the one-pass kernel holds
 *   "gram_interleaved"        0: k_gram instead of k_gram_il (staging not interleaved with the matrix instructions)
 *   "gram_read_ahead"         (default 1) k_gram_regions reads the operands of a 4-row step during the products of the step before; 0: every step
 *                             opens with its own reads (as k_gram_il).  The same products in the same order: the same Gram matrix bit for bit
 *   "gram_waves"              (default 8) wavefronts per workgroup of k_gram_regions: 8 puts two on every SIMD, so that one's products fill the matrix
 *                             pipe while the other issues its staging; 4: one per SIMD.  Anything else is refused.  Every tile is summed by one
 *                             wavefront over the same rows in the same order: the same Gram matrix bit for bit.  With "gram_read_ahead" = 0 always 4
 *   "featy_chains"            (default 1) k_feat_y takes the run list of the unprojected stack from k_batch_layout's table and requests the next
 *                             slot's record and status a feature ahead; 0: the kernel without either (the run list derived per feature). The same
 *                             loads, products and stores: the results are equal bit for bit.
 *   "gram_blocks_only"        1: always the 8 x 8-tile block form of the Gram kernel (k_gram_blk)
 *   "fuse_chol_inputs"        0: round 2's k_tf_gather / k_tf_abh assemble the factorisations' inputs
 *   "featy_skip"              DEVELOPER BUILD ONLY (-DOVG_FEAT_ABLATE; the shipped library answers OVGPU_ERR_INVALID): bit mask
 *                             (1 sweep, 2 projection + stores, 4 SYRK, 8 Cholesky) of phases of the fused kernel skipped for
 *                             timing (tools/dev_featy_ablate.py); the results of such an update are GARBAGE.                    */
int ovgpu_debug_option(ovgpu_ctx *ctx, const char *name, int64_t value, int64_t *old_value);

/* Developer aid (no reference counterpart): per-phase cycle counters of workgroup 0 of the per-feature kernel.
 * enable != 0 allocates / clears 512 counters, out512 != NULL reads them back first. */
int ovgpu_debug_cycles(ovgpu_ctx *ctx, int enable, long long *out512);

/* Measurement aid (no reference counterpart): what kind of box this is, from six short probes (out3 holds SIX doubles).
 *   out3[0]  shader clock in MHz: shader cycles (s_memtime) over the constant 100 MHz reference (s_memrealtime) across a
 *            dependent-arithmetic loop
 *   out3[1]  latency of a dependent load that hits L2, in ns (pointer chase over 1 MB)
 *   out3[2]  latency of a dependent load beyond L2, in ns (pointer chase over 256 MB, one load per 4 KB page)
 *   out3[3]  shader clock in MHz with every SIMD busy on the FP64 matrix pipe for ~1 ms (what the power limit leaves under load)
 *   out3[4]  microseconds per launch of 200 dependent empty kernels on one stream (command processor + host)
 *   out3[5]  nanoseconds per workgroup of one launch of 65 536 empty workgroups (dispatch rate)
 * The boxes of a pool run the same binary 20 % apart (0.85 and 1.02 ms per update measured within minutes of each other);
 * bench.py reports these numbers next to its line.  (On the one slow box probed they equalled the fast boxes': whatever
 * separates the boxes, it is none of the six.)                                                                        */
int ovgpu_debug_box_probe(ovgpu_ctx *ctx, double *out3);

/* Time in ms of the measurement compression (all its launches) and of the
 * whole update, averaged over the launches since the last call with
 * reset != 0; measured with HIP events on the context's stream.              */
int ovgpu_kernel_times(ovgpu_ctx *ctx, int reset, double *ms_compress_avg,
                       double *ms_update_avg, int64_t *n_launches);

/* Average time in ms of the per-feature kernel (Jacobians, nullspace projection, chi2 gate:
 * k_system) over the same launches; call BEFORE ovgpu_kernel_times(reset = 1).              */
int ovgpu_system_time(ovgpu_ctx *ctx, double *ms_system_avg, int64_t *n_launches);

#ifdef __cplusplus
}
#endif
#endif /* OVGPU_H */
