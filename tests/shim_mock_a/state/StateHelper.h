// stand-in for ov_msckf/src/state/StateHelper.h:45-240 (TEST INFRASTRUCTURE): the entry points of tests/shim_mock/state/StateHelper.h
// plus StateHelper::initialize (StateHelper.h:148-162), which the mode-A delayed initialisation (open_vins_amd/shim/ovgpu_delayed_init_a.h)
// calls.  Placed in front of tests/shim_mock on the include path.
#pragma once
#include <Eigen/Eigen>
#include <memory>
#include <vector>
#include "state/State.h"
namespace ov_msckf {
class StateHelper {
public:
  static void EKFUpdate(std::shared_ptr<State> state, const std::vector<std::shared_ptr<ov_type::Type>> &H_order, const Eigen::MatrixXd &H,
                        const Eigen::VectorXd &res, const Eigen::MatrixXd &R);
  static Eigen::MatrixXd get_full_covariance(std::shared_ptr<State> state);
  static void marginalize(std::shared_ptr<State> state, std::shared_ptr<ov_type::Type> marg);
  static bool initialize(std::shared_ptr<State> state, std::shared_ptr<ov_type::Type> new_variable, const std::vector<std::shared_ptr<ov_type::Type>> &H_order,
                         Eigen::MatrixXd &H_R, Eigen::MatrixXd &H_L, Eigen::MatrixXd &R, Eigen::VectorXd &res, double chi_2_mult);
};
} // namespace ov_msckf
