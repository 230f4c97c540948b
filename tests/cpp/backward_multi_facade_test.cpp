// dense::compute_backward_multi / dense::solution_jacobians of the C++ facade
// (include/proxsuite/proxqp/dense/compute_ECJ.hpp): K loss derivatives of one solved QP in one call against
// dense::compute_backward row by row on a second QP object of the same model (re-solved before every single call).
// Linked against the emulator build of the device code or against libproxqp_hip.so by tests/test_cpp_backward_multi.py.
#include <cmath>
#include <cstdio>

#include <proxsuite/proxqp/dense/dense.hpp>
#include <proxsuite/proxqp/utils/random_qp_problems.hpp>

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
  const isize n = 10, ne = 4, ni = 7, ntot = n + ne + ni, K = 4;
  utils::rand::set_seed(0);
  dense::Model<T> m = utils::dense_strongly_convex_qp(n, ne, ni, 0.85, 1e-1);
  dense::QP<T> qp{ n, ne, ni }, ref{ n, ne, ni };
  for (auto* q : { &qp, &ref }) {
    q->settings.eps_abs = 1e-9;
    q->settings.eps_rel = 0;
    q->init(m.H, m.g, m.A, m.b, m.C, m.l, m.u);
    q->solve();
  }
  dense::Mat<T> ld(K, ntot);
  for (isize k = 0; k < K; ++k)
    for (isize i = 0; i < (k < 2 ? n : ntot); ++i)
      ld(k, i) = std::sin(T(1 + 3 * k + 7 * i));
  const dense::Mat<T> V = dense::compute_backward_multi<T>(qp, dense::MatRef<T>(ld), 1e-5, 1e-7, 1e-7);
  EXPECT(V.rows() == K && V.cols() == ntot);
  // the project's gate for two kernels of one algorithm: 1e-10 (1 + max |ref|)
  T worst = 0, scale = 1;
  for (isize k = 0; k < K; ++k) {
    dense::Vec<T> row(ntot);
    for (isize i = 0; i < ntot; ++i)
      row[i] = ld(k, i);
    ref.solve();
    dense::compute_backward<T>(ref, row, 1e-5, 1e-7, 1e-7);
    const auto& bd = ref.model.backward_data;
    for (isize i = 0; i < n; ++i) {
      worst = std::fmax(worst, std::fabs(V(k, i) - bd.dL_dg[i]));
      scale = std::fmax(scale, 1 + std::fabs(bd.dL_dg[i]));
    }
    for (isize i = 0; i < ne; ++i) {
      worst = std::fmax(worst, std::fabs(-V(k, n + i) - bd.dL_db[i]));
      scale = std::fmax(scale, 1 + std::fabs(bd.dL_db[i]));
    }
  }
  std::printf("rows vs compute_backward: max |difference| %.3g (gate %.3g)\n", worst, 1e-10 * scale);
  EXPECT(worst <= 1e-10 * scale);
  EXPECT(qp.results.info.rho == 1e-7 && qp.results.info.mu_eq == 1e-7 && qp.results.info.mu_in == 1e-7);

  qp.solve();
  const dense::SolutionJacobians<T> J = dense::solution_jacobians<T>(qp, 1e-5, 1e-7, 1e-7);
  EXPECT(J.dx_dg.rows() == n && J.dx_dg.cols() == n);
  EXPECT(J.dx_db.rows() == n && J.dx_db.cols() == ne);
  EXPECT(J.dx_du.rows() == n && J.dx_du.cols() == ni);
  EXPECT(J.dx_dl.rows() == n && J.dx_dl.cols() == ni);
  // dx/dg of a strictly convex QP is symmetric negative semi-definite on the active constraints' null space: the diagonal is <= 0
  for (isize i = 0; i < n; ++i)
    EXPECT(J.dx_dg(i, i) <= 1e-6);

  bool thrown = false;
  try {
    dense::Mat<T> bad(2, ntot + 1);
    (void)dense::compute_backward_multi<T>(qp, dense::MatRef<T>(bad));
  } catch (const std::invalid_argument&) {
    thrown = true;
  }
  EXPECT(thrown);
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
