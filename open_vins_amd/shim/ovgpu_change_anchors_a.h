// Mode-A body of ov_msckf::UpdaterSLAM::change_anchors (ov_msckf/src/update/UpdaterSLAM.cpp:481-504 and perform_anchor_change, :506-647,
// rpng/open_vins v2.7), for an UNPATCHED reference: public API of State / StateHelper only.  Included by UpdaterSLAM_change_anchors.cpp when
// OVGPU_SHIM_CHANGE_ANCHORS_A is defined.
//
// One device call (ovgpu_slam_anchor_systems) forms, for every landmark anchored in the clone that leaves, what perform_anchor_change hands
// to StateHelper::EKFPropagation — phi_order_OLD and Phi (:583-634) — and what it writes into the landmark (:640-646), and leaves the
// library's own state alone.  The host then calls the stock StateHelper::EKFPropagation (public static, StateHelper.h:76-78) landmark after
// landmark in the reference's iteration order.  The reference computes each Phi after the previous landmark's propagation, but from state
// VALUES only (clone poses, extrinsics, the landmark itself), none of which a propagation moves: replaying the exported Phi's in order
// reproduces its sequence.
#pragma once

#include <unordered_map>

#include "ovgpu_shim_common.h"

void ov_msckf::UpdaterSLAM::change_anchors(std::shared_ptr<State> state) {
  using namespace ov_type;
  if ((int)state->_clones_IMU.size() <= state->_options.max_clone_size) return; // :484-486
  const double marg_timestep = state->margtimestep();
  // every landmark of the state in ONE view, in the iteration order of _features_SLAM: the library walks them in that order (:492)
  const ovgpu_shim::StateSnapshot snap(state);
  const ovgpu_shim::CloneIndex clones(snap.fs.clone_times);
  ovgpu_shim::FlatLandmarks fl;
  bool any = false;
  for (const auto &kv : state->_features_SLAM) {
    any |= LandmarkRepresentation::is_relative_representation(kv.second->_feat_representation) && kv.second->_anchor_clone_timestamp == marg_timestep; // :498-500
    fl.add(kv.second, snap, clones);
  }
  if (!any) return;
  ov_core::FeatureInitializerOptions fo;
  ovgpu_shim::Context &cx = ovgpu_shim::context_for(ovgpu_shim::make_options(_options_slam, fo, state->_options, OVGPU_REP_GLOBAL_3D));
  ovgpu_ctx *ctx = cx.get();
  const ovgpu_state_view sv = snap.fs.view(); // (uploaded as the mode-B body uploads it; the export itself reads values, not the covariance)
  const ovgpu_landmarks_view lv = fl.view();
  cx.check(ovgpu_set_state(ctx, &sv), "ovgpu_set_state");
  cx.check(ovgpu_set_landmarks(ctx, &lv), "ovgpu_set_landmarks");
  cx.check(ovgpu_shim::set_active_landmarks(ctx, 0, nullptr), "ovgpu_set_active_landmarks"); // perform_anchor_change reads no column table
  const int32_t marg = clones.find(marg_timestep), newest = clones.find(state->_timestamp);
  ovgpu_anchor_sizes sz;
  cx.check(ovgpu_slam_anchor_systems_len(ctx, marg, newest, &sz), "ovgpu_slam_anchor_systems_len");
  if (sz.n_sys == 0) return;
  std::vector<ovgpu_anchor_system> sys((size_t)sz.n_sys);
  std::vector<int32_t> var_id((size_t)sz.n_vars), var_size((size_t)sz.n_vars);
  std::vector<double> Phi((size_t)sz.n_phi), val(3 * (size_t)sz.n_sys), fej(3 * (size_t)sz.n_sys);
  cx.check(ovgpu_slam_anchor_systems(ctx, marg, newest, &sz, sys.data(), var_id.data(), var_size.data(), Phi.data(), val.data(), fej.data()),
           "ovgpu_slam_anchor_systems");
  std::unordered_map<int, std::shared_ptr<Type>> var_at; // covariance id -> clone / extrinsics / landmark
  for (const auto &v : snap.var_of_cov) var_at[v->id()] = v;
  for (const auto &l : fl.lm) var_at[l->id()] = l;

  // ---- the systems in order through the stock StateHelper::EKFPropagation (:583-637), then the landmark (:640-646)
  using RowMajor = Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>;
  for (size_t k = 0; k < sys.size(); k++) {
    const ovgpu_anchor_system &s = sys[k];
    const std::shared_ptr<Landmark> &landmark = fl.lm[(size_t)s.lm_index];
    std::vector<std::shared_ptr<Type>> phi_order_NEW{landmark}, phi_order_OLD;
    for (int i = 0; i < s.n_vars; i++) phi_order_OLD.push_back(var_at.at(var_id[s.var_off + i]));
    const Eigen::MatrixXd Phi_l = Eigen::Map<const RowMajor>(Phi.data() + s.phi_off, s.lsz, s.n_old);
    const Eigen::MatrixXd Q = 0.0 * Eigen::MatrixXd::Identity(s.lsz, s.lsz); // :612, Q = 0
    StateHelper::EKFPropagation(state, phi_order_NEW, phi_order_OLD, Phi_l, Q);
    landmark->_anchor_cam_id = (int)snap.cam_ids[s.anchor_cam]; // :642-643
    landmark->_anchor_clone_timestamp = snap.fs.clone_times[s.anchor_clone];
    const double *v = val.data() + 3 * k, *vf = fej.data() + 3 * k;
    if (landmark->_feat_representation == LandmarkRepresentation::Representation::ANCHORED_INVERSE_DEPTH_SINGLE) { // Landmark::set_from_xyz, Landmark.cpp:124-140
      landmark->uv_norm_zero << v[0], v[1], 1.0;
      landmark->uv_norm_zero_fej << vf[0], vf[1], 1.0;
      landmark->set_value(Eigen::Matrix<double, 1, 1>(v[2]));
      landmark->set_fej(Eigen::Matrix<double, 1, 1>(vf[2]));
    } else {
      landmark->set_value(Eigen::Map<const Eigen::Vector3d>(v)); // :644-645
      landmark->set_fej(Eigen::Map<const Eigen::Vector3d>(vf));
    }
    landmark->has_had_anchor_change = true; // :646
  }
}
