// proxsuite/proxqp/dense/helpers.hpp -- estimate_minimal_eigen_value_of_symmetric_matrix of the dense ProxQP API,
// MI355X build (reference include/proxsuite/proxqp/dense/helpers.hpp:115-166).  The value goes to
// QP::init(..., manual_minimal_H_eigenvalue) / QP::update for non-convex QPs.  It is computed on the device by
// pqp_estimate_min_eigenvalues (include/proxqp_hip.h) with count = 1; batches of matrices call that entry directly.
#ifndef PROXSUITE_AMD_PROXQP_DENSE_HELPERS_HPP
#define PROXSUITE_AMD_PROXQP_DENSE_HELPERS_HPP

#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "proxqp_hip.h"
#include "proxsuite/proxqp/dense/wrapper.hpp"

namespace proxsuite {
namespace proxqp {
namespace dense {

/*!
 * Estimate minimal eigenvalue of a symmetric Matrix
 * @param H symmetric matrix.
 * @param EigenValueEstimateMethodOption
 * @param power_iteration_accuracy power iteration algorithm accuracy tracked
 * @param nb_power_iteration maximal number of power iteration executed
 *
 * Throws std::invalid_argument when H is not square or not symmetric (!H.isApprox(H^T, eps)).
 */
template<typename T>
T
estimate_minimal_eigen_value_of_symmetric_matrix(
  MatRef<T> H,
  EigenValueEstimateMethodOption estimate_method_option = EigenValueEstimateMethodOption::ExactMethod,
  T power_iteration_accuracy = T(1.e-3),
  isize nb_power_iteration = 1000,
  int device = 0)
{
  static_assert(std::is_same<T, double>::value, "the device path computes in fp64");
  if (H.rows() != H.cols())
    detail::bad_size("H has a number of rows different of the number of columns.", H.cols(), H.rows());
  if (H.rows() == 0)
    return T(0); // (the reference's res(0.): nothing to estimate)
  const isize n = H.rows();
  std::vector<T> packed;
  const T* data = H.ptr;
  if (!H.is_packed_row_major()) {
    packed.resize(usize(n * n));
    for (isize i = 0; i < n; ++i)
      for (isize j = 0; j < n; ++j)
        packed[usize(i * n + j)] = H(i, j);
    data = packed.data();
  }
  T res(0.);
  const int rc = pqp_estimate_min_eigenvalues(
    device, 1, n, data, int(estimate_method_option), power_iteration_accuracy, nb_power_iteration, &res, nullptr);
  if (rc == PQP_ERR_INVALID_ARGUMENT && std::string(pqp_last_error()).rfind("H is not symmetric.", 0) == 0)
    throw std::invalid_argument("H is not symmetric.");
  detail::check(rc);
  return res;
}

template<typename T>
T
estimate_minimal_eigen_value_of_symmetric_matrix(
  const Mat<T>& H,
  EigenValueEstimateMethodOption estimate_method_option = EigenValueEstimateMethodOption::ExactMethod,
  T power_iteration_accuracy = T(1.e-3),
  isize nb_power_iteration = 1000,
  int device = 0)
{
  return estimate_minimal_eigen_value_of_symmetric_matrix(
    MatRef<T>(H), estimate_method_option, power_iteration_accuracy, nb_power_iteration, device);
}

} // namespace dense
} // namespace proxqp
} // namespace proxsuite

#endif
