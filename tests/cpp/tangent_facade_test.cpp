// dense::compute_forward_sensitivity of the C++ facade (include/proxsuite/proxqp/dense/compute_ECJ.hpp): K tangents of
// one solved QP in one call.  Vector tangents (dg, db: a right-hand side without z part) against
// dense::compute_backward_multi on a second QP object of the same model fed (dg | -db | 0); the full set against the
// adjoint identity <e_i, T> = sum over the parameters of <dL/dtheta, dtheta> with dense::compute_backward for ld = e_i.
// Linked against the emulator build of the device code or against libproxqp_hip.so by tests/test_cpp_tangent.py.
#include <cmath>
#include <cstdio>
#include <vector>

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

static std::vector<T>
wave(isize len, int phase)
{
  std::vector<T> v(static_cast<std::size_t>(len));
  for (isize i = 0; i < len; ++i)
    v[static_cast<std::size_t>(i)] = std::sin(T(phase + 3 * i)) + 0.25 * std::cos(T(7 * phase + i));
  return v;
}

int
main()
{
  const isize n = 10, ne = 4, ni = 7, ntot = n + ne + ni, K = 3;
  utils::rand::set_seed(0);
  dense::Model<T> m = utils::dense_strongly_convex_qp(n, ne, ni, 0.85, 1e-1);
  dense::QP<T> qp{ n, ne, ni }, ref{ n, ne, ni };
  for (auto* q : { &qp, &ref }) {
    q->settings.eps_abs = 1e-9;
    q->settings.eps_rel = 0;
    q->init(m.H, m.g, m.A, m.b, m.C, m.l, m.u);
    q->solve();
  }
  const std::vector<T> dH = wave(K * n * n, 1), dg = wave(K * n, 2), dA = wave(K * ne * n, 3), db = wave(K * ne, 4),
                       dC = wave(K * ni * n, 5), dl = wave(K * ni, 6), du = wave(K * ni, 7);

  // 1. vector tangents against compute_backward_multi: the project's gate for two kernels of one algorithm
  dense::Tangents<T> vec;
  vec.dg = dg.data();
  vec.db = db.data();
  vec.n_dir = K;
  const dense::ForwardSensitivity<T> S = dense::compute_forward_sensitivity<T>(qp, vec, 1e-5, 1e-7, 1e-7);
  EXPECT(S.dx.rows() == K && S.dx.cols() == n && S.dy.rows() == K && S.dy.cols() == ne && S.dz.rows() == K && S.dz.cols() == ni);
  EXPECT(isize(S.active.size()) == ni);
  EXPECT(qp.results.info.rho == 1e-7 && qp.results.info.mu_eq == 1e-7 && qp.results.info.mu_in == 1e-7);
  dense::Mat<T> ld(K, ntot);
  for (isize k = 0; k < K; ++k) {
    for (isize i = 0; i < n; ++i)
      ld(k, i) = dg[std::size_t(k * n + i)];
    for (isize i = 0; i < ne; ++i)
      ld(k, n + i) = -db[std::size_t(k * ne + i)];
  }
  std::vector<std::int32_t> flags;
  const dense::Mat<T> V = dense::compute_backward_multi<T>(ref, dense::MatRef<T>(ld), 1e-5, 1e-7, 1e-7, &flags);
  T worst = 0, scale = 1;
  isize n_active = 0;
  for (isize i = 0; i < ni; ++i) {
    EXPECT(flags[std::size_t(i)] == S.active[std::size_t(i)]);
    n_active += S.active[std::size_t(i)] ? 1 : 0;
  }
  EXPECT(n_active >= 1 && n_active < ni);
  for (isize k = 0; k < K; ++k) {
    for (isize i = 0; i < ntot; ++i) {
      const T got = i < n ? S.dx(k, i) : (i < n + ne ? S.dy(k, i - n) : S.dz(k, i - n - ne));
      if (i >= n + ne && !S.active[std::size_t(i - n - ne)]) {
        EXPECT(got == 0.0); // inactive rows of dz are exactly 0
        continue;
      }
      worst = std::fmax(worst, std::fabs(got - V(k, i)));
      scale = std::fmax(scale, 1 + std::fabs(V(k, i)));
    }
  }
  std::printf("vector tangents vs compute_backward_multi: max |difference| %.3g (gate %.3g)\n", worst, 1e-10 * scale);
  EXPECT(worst <= 1e-10 * scale);

  // 2. all seven tangents: dx against the adjoint identity, the project's gate between restatements 1e-6 (1 + max |ref|)
  dense::Tangents<T> all;
  all.dH = dH.data();
  all.dg = dg.data();
  all.dA = dA.data();
  all.db = db.data();
  all.dC = dC.data();
  all.dl = dl.data();
  all.du = du.data();
  all.n_dir = K;
  qp.solve();
  const dense::ForwardSensitivity<T> F = dense::compute_forward_sensitivity<T>(qp, all, 1e-5, 1e-7, 1e-7);
  worst = 0;
  scale = 1;
  for (isize i = 0; i < n; ++i) {
    dense::Vec<T> e(ntot);
    for (isize j = 0; j < ntot; ++j)
      e[j] = j == i ? 1.0 : 0.0;
    ref.solve();
    dense::compute_backward<T>(ref, e, 1e-5, 1e-7, 1e-7);
    const auto& bd = ref.model.backward_data;
    for (isize k = 0; k < K; ++k) {
      T want = 0;
      for (isize a = 0; a < n; ++a) {
        want += bd.dL_dg[a] * dg[std::size_t(k * n + a)];
        for (isize b = 0; b < n; ++b)
          want += bd.dL_dH(a, b) * dH[std::size_t((k * n + a) * n + b)];
      }
      for (isize a = 0; a < ne; ++a) {
        want += bd.dL_db[a] * db[std::size_t(k * ne + a)];
        for (isize b = 0; b < n; ++b)
          want += bd.dL_dA(a, b) * dA[std::size_t((k * ne + a) * n + b)];
      }
      for (isize a = 0; a < ni; ++a) {
        want += bd.dL_dl[a] * dl[std::size_t(k * ni + a)] + bd.dL_du[a] * du[std::size_t(k * ni + a)];
        for (isize b = 0; b < n; ++b)
          want += bd.dL_dC(a, b) * dC[std::size_t((k * ni + a) * n + b)];
      }
      worst = std::fmax(worst, std::fabs(F.dx(k, i) - want));
      scale = std::fmax(scale, 1 + std::fabs(want));
    }
  }
  std::printf("all seven tangents, dx vs adjoint identity: max |difference| %.3g (gate %.3g)\n", worst, 1e-6 * scale);
  EXPECT(worst <= 1e-6 * scale);

  // 3. no tangent at all: zeros; no direction: empty
  qp.solve();
  dense::Tangents<T> none;
  const dense::ForwardSensitivity<T> Z = dense::compute_forward_sensitivity<T>(qp, none);
  EXPECT(Z.dx.rows() == 1);
  for (isize i = 0; i < n; ++i)
    EXPECT(Z.dx(0, i) == 0.0);
  none.n_dir = 0;
  EXPECT(dense::compute_forward_sensitivity<T>(qp, none).dx.rows() == 0);
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
