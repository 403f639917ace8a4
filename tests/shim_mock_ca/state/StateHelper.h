// stand-in for ov_msckf/src/state/StateHelper.h:45-240 (TEST INFRASTRUCTURE): the entry points of tests/shim_mock/state/StateHelper.h
// plus StateHelper::EKFPropagation (StateHelper.h:76-78), which the mode-A anchor change (open_vins_amd/shim/ovgpu_change_anchors_a.h)
// calls.  Placed in front of tests/shim_mock on the include path.
#pragma once
#include <Eigen/Eigen>
#include <memory>
#include <vector>
#include "state/State.h"
namespace ov_msckf {
class StateHelper {
public:
  static void EKFPropagation(std::shared_ptr<State> state, const std::vector<std::shared_ptr<ov_type::Type>> &order_NEW,
                             const std::vector<std::shared_ptr<ov_type::Type>> &order_OLD, const Eigen::MatrixXd &Phi, const Eigen::MatrixXd &Q);
  static void EKFUpdate(std::shared_ptr<State> state, const std::vector<std::shared_ptr<ov_type::Type>> &H_order, const Eigen::MatrixXd &H,
                        const Eigen::VectorXd &res, const Eigen::MatrixXd &R);
  static Eigen::MatrixXd get_full_covariance(std::shared_ptr<State> state);
  static void marginalize(std::shared_ptr<State> state, std::shared_ptr<ov_type::Type> marg);
};
} // namespace ov_msckf
