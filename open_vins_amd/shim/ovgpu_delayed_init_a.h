// Mode-A body of ov_msckf::UpdaterSLAM::delayed_init (ov_msckf/src/update/UpdaterSLAM.cpp:61-251, rpng/open_vins v2.7), for an UNPATCHED
// reference: public API of State / StateHelper only.  Included by UpdaterSLAM_delayed_init.cpp when OVGPU_SHIM_DELAYED_INIT_A is defined.
//
// One device call (ovgpu_slam_init_systems) triangulates the batch and runs the chain of StateHelper::initialize calls speculatively on
// copies of the state, exporting every feature's system as linearised where the reference linearises it.  The host then hands the
// systems, in order, to the stock StateHelper::initialize, which gates, initialises and updates the state itself.  Where the host decides
// a gate differently from the device (a chi2 within rounding of its threshold), the chain is restarted from the host's state at the next
// feature, so the host's filter stays the reference's.  UpdaterSLAM::change_anchors stays the reference's in mode A.
#pragma once

#include <unordered_map>

#include "ovgpu_shim_common.h"

void ov_msckf::UpdaterSLAM::delayed_init(std::shared_ptr<State> state, std::vector<std::shared_ptr<ov_core::Feature>> &feature_vec) {
  using namespace ov_type;
  if (feature_vec.empty()) return; // :64-65
  const auto rep = state->_options.feat_rep_slam;
  auto is_single = [](LandmarkRepresentation::Representation r) { return r == LandmarkRepresentation::Representation::ANCHORED_INVERSE_DEPTH_SINGLE; };
  auto snap = std::make_unique<ovgpu_shim::StateSnapshot>(state);
  const ovgpu_shim::CloneIndex clones(snap->fs.clone_times);

  // ---- 1. clean the tracks (:75-96) and flatten them; ArUco corners use _options_aruco (:226-232) and feat_rep_aruco (:160-166)
  static thread_local ovgpu_shim::FlatFeatures ff;
  ff.clear();
  std::vector<double> f_sigma, f_mult;
  std::vector<int32_t> f_rep;
  bool any_aruco = false;
  for (auto it = feature_vec.begin(); it != feature_vec.end();) {
    if (ovgpu_shim::flatten_track(**it, *snap, clones, ff) < 2) { // :91-93
      (*it)->to_delete = true;
      it = feature_vec.erase(it);
      continue;
    }
    ovgpu_shim::append_track(**it, *snap, clones, ff);
    const bool is_aruco = (int)(*it)->featid < state->_options.max_aruco_features;
    any_aruco |= is_aruco;
    f_sigma.push_back(is_aruco ? _options_aruco.sigma_pix : _options_slam.sigma_pix);
    f_mult.push_back(is_aruco ? _options_aruco.chi2_multipler : _options_slam.chi2_multipler);
    f_rep.push_back((int32_t)(is_aruco ? state->_options.feat_rep_aruco : rep));
    ++it;
  }
  if (feature_vec.empty()) return;
  const int F = (int)feature_vec.size();

  // ---- 2. one device call (and one more after every gate the host decides differently)
  ovgpu_shim::Context &cx = ovgpu_shim::context_for(ovgpu_shim::make_options(_options_slam, initializer_feat->config(), state->_options, (int)rep));
  ovgpu_ctx *ctx = cx.get();
  std::vector<int32_t> tri_anchor(F, -1), tri_status(F, OVGPU_FEAT_USED), var_id, var_size;
  std::vector<double> pA(3 * (size_t)F), pG(3 * (size_t)F), H_x, H_f, res;
  std::vector<ovgpu_init_system> sys(F);
  auto run = [&](int first) {
    ovgpu_shim::FlatLandmarks old;
    for (const auto &kv : state->_features_SLAM) old.add(kv.second, *snap, clones);
    const ovgpu_state_view sv = snap->fs.view();
    const ovgpu_features_view fv = ff.view();
    const ovgpu_landmarks_view lv = old.view();
    cx.check(ovgpu_set_state(ctx, &sv), "ovgpu_set_state");
    cx.check(ovgpu_set_landmarks(ctx, &lv), "ovgpu_set_landmarks");
    cx.check(ovgpu_shim::set_active_landmarks(ctx, 0, nullptr), "ovgpu_set_active_landmarks"); // no resident landmark has a column in StateHelper::initialize
    cx.check(ovgpu_set_features(ctx, &fv), "ovgpu_set_features");
    if (any_aruco) cx.check(ovgpu_set_feature_options(ctx, f_sigma.data(), f_mult.data()), "ovgpu_set_feature_options");
    if (any_aruco && state->_options.feat_rep_aruco != rep) cx.check(ovgpu_set_feature_reps(ctx, f_rep.data()), "ovgpu_set_feature_reps");
    if (first > 0) // a restart: the triangulation of the first call (the reference does not triangulate again inside the loop)
      cx.check(ovgpu_set_triangulation(ctx, pA.data(), pG.data(), tri_anchor.data(), tri_status.data()), "ovgpu_set_triangulation");
    ovgpu_init_sizes sz;
    cx.check(ovgpu_slam_init_systems_len(ctx, (int32_t)rep, first, &sz), "ovgpu_slam_init_systems_len");
    var_id.resize(std::max<int64_t>(sz.n_vars, 1)), var_size.resize(std::max<int64_t>(sz.n_vars, 1));
    H_x.resize(std::max<int64_t>(sz.n_hx, 1)), H_f.resize(std::max<int64_t>(sz.n_hf, 1)), res.resize(std::max<int64_t>(sz.n_res, 1));
    cx.check(ovgpu_slam_init_systems(ctx, (int32_t)rep, first, &sz, sys.data(), var_id.data(), var_size.data(), H_x.data(), H_f.data(), res.data(), nullptr),
             "ovgpu_slam_init_systems");
    if (first == 0) {
      cx.check(ovgpu_get_triangulation(ctx, pA.data(), pG.data(), tri_anchor.data()), "ovgpu_get_triangulation");
      for (int f = 0; f < F; f++) tri_status[f] = sys[f].status == OVGPU_FEAT_CHI2_REJECTED ? OVGPU_FEAT_USED : sys[f].status;
    }
  };
  run(0);
  std::unordered_map<int, std::shared_ptr<Type>> var_at; // covariance id -> clone / extrinsics / intrinsics (new landmarks go behind them)
  for (const auto &v : snap->var_of_cov) var_at[v->id()] = v;

  // ---- 3. the systems in order through the stock StateHelper::initialize (:203-239)
  int f = 0;
  for (auto it = feature_vec.begin(); it != feature_vec.end(); f++) {
    // the triangulation's side effects on the Feature, for every representation (FeatureInitializer.cpp:45-46, :109-110, :333-335)
    ovgpu_shim::write_triangulation(**it, *snap, ff, tri_anchor[f], &pA[3 * f], &pG[3 * f]);
    (*it)->to_delete = true;
    const ovgpu_init_system &s = sys[f];
    if (s.rows == 0) { // no system: the triangulation failed (:127-143)
      it = feature_vec.erase(it);
      continue;
    }
    const auto frep = (LandmarkRepresentation::Representation)s.feat_rep;
    std::vector<std::shared_ptr<Type>> Hx_order;
    for (int i = 0; i < s.n_vars; i++) Hx_order.push_back(var_at.at(var_id[s.var_off + i]));
    using RowMajor = Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>;
    Eigen::MatrixXd Hx = Eigen::Map<const RowMajor>(H_x.data() + s.hx_off, s.rows, s.h);
    Eigen::MatrixXd Hf = Eigen::Map<const RowMajor>(H_f.data() + s.hf_off, s.rows, s.cols_f);
    Eigen::VectorXd r = Eigen::Map<const Eigen::VectorXd>(res.data() + s.res_off, s.rows);
    auto landmark = std::make_shared<Landmark>(is_single(frep) ? 1 : 3);
    landmark->_featid = (*it)->featid;
    landmark->_feat_representation = frep;
    landmark->_unique_camera_id = (*it)->anchor_cam_id; // :214
    const Eigen::Vector3d seed = Eigen::Map<const Eigen::Vector3d>(s.p_seed);
    if (LandmarkRepresentation::is_relative_representation(frep)) {
      landmark->_anchor_cam_id = (int)snap->cam_ids[s.anchor_cam];
      landmark->_anchor_clone_timestamp = snap->fs.clone_times[s.anchor_clone];
    }
    landmark->set_from_xyz(seed, false);
    landmark->set_from_xyz(seed, true);
    const double sigma = f_sigma[f];
    Eigen::MatrixXd R = sigma * sigma * Eigen::MatrixXd::Identity(s.rows, s.rows);
    const bool ok = StateHelper::initialize(state, landmark, Hx_order, Hx, Hf, R, r, f_mult[f]);
    const bool device_ok = s.status == OVGPU_FEAT_USED;
    if (ok) {
      state->_features_SLAM.insert({(*it)->featid, landmark});
      ++it;
    } else {
      it = feature_vec.erase(it);
    }
    // ---- 4. a gate decided differently: the chain again, from the host's state, at the next feature
    if (ok != device_ok && f + 1 < F) {
      snap = std::make_unique<ovgpu_shim::StateSnapshot>(state);
      run(f + 1);
    }
  }
}
