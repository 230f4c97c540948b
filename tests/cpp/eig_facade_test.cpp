// dense::estimate_minimal_eigen_value_of_symmetric_matrix of the C++ facade (include/proxsuite/proxqp/dense/helpers.hpp)
// on a 6 x 6 matrix of prescribed spectrum: H = Q diag(lambda) Q^T with Q a Householder reflector, so lambda_min is known.
// Linked against the emulator build of the device code or against libproxqp_hip.so by tests/test_cpp_eig_facade.py.
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "proxsuite/proxqp/dense/dense.hpp"

using namespace proxsuite::proxqp;
using T = double;

static int failures = 0;
#define EXPECT(cond)                                                                                                     \
  do {                                                                                                                   \
    if (!(cond)) {                                                                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                    \
      ++failures;                                                                                                        \
    }                                                                                                                    \
  } while (0)

int
main()
{
  const isize n = 6;
  const T lambda[n] = { -2.5, -1.0, 0.5, 1.0, 2.0, 4.0 };
  // Q = I - 2 w w^T / (w^T w): orthogonal and symmetric
  T w[n], ww = 0;
  for (isize i = 0; i < n; ++i) {
    w[i] = T(1 + i) / T(n) - 0.3;
    ww += w[i] * w[i];
  }
  dense::Mat<T> Q(n, n), H(n, n);
  for (isize i = 0; i < n; ++i)
    for (isize j = 0; j < n; ++j)
      Q(i, j) = (i == j ? 1.0 : 0.0) - 2 * w[i] * w[j] / ww;
  for (isize i = 0; i < n; ++i)
    for (isize j = 0; j <= i; ++j) {
      T s = 0;
      for (isize k = 0; k < n; ++k)
        s += Q(i, k) * lambda[k] * Q(j, k);
      H(i, j) = s;
      H(j, i) = s;
    }
  const T u = std::ldexp(1.0, -53), norm2 = 4.0; // ||H||_2 = max |lambda|
  // ExactMethod: |value - lambda_min| <= 8 n u ||H||_2
  const T exact = dense::estimate_minimal_eigen_value_of_symmetric_matrix(H);
  std::printf("exact %.17g (error %.3g, gate %.3g)\n", exact, std::fabs(exact - lambda[0]), 8 * n * u * norm2);
  EXPECT(std::fabs(exact - lambda[0]) <= 8 * n * u * norm2);
  // PowerIteration: |value - lambda_min| <= 2 sqrt(n) accuracy
  for (T accuracy : { 1e-3, 1e-8 }) {
    const T power = dense::estimate_minimal_eigen_value_of_symmetric_matrix(
      H, EigenValueEstimateMethodOption::PowerIteration, accuracy, 1000);
    std::printf("power(%g) %.17g (error %.3g, gate %.3g)\n", accuracy, power, std::fabs(power - lambda[0]),
                2 * std::sqrt(T(n)) * accuracy);
    EXPECT(std::fabs(power - lambda[0]) <= 2 * std::sqrt(T(n)) * accuracy);
  }
  // a view with strides (the transpose of a row-major block) goes through the packed copy
  const T viewed = dense::estimate_minimal_eigen_value_of_symmetric_matrix(dense::MatRef<T>(H.data(), n, n, 1, n));
  EXPECT(viewed == exact);
  bool thrown = false;
  try {
    dense::Mat<T> A = H;
    A(1, 4) += 1.0;
    (void)dense::estimate_minimal_eigen_value_of_symmetric_matrix(A);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "H is not symmetric.";
  }
  EXPECT(thrown);
  thrown = false;
  try {
    dense::Mat<T> R(3, 4);
    (void)dense::estimate_minimal_eigen_value_of_symmetric_matrix(R);
  } catch (const std::invalid_argument&) {
    thrown = true;
  }
  EXPECT(thrown);
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
