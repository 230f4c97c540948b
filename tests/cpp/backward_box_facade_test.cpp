// dense::compute_backward and dense::qp_solve_backward_in_parallel of the C++ facade on QPs with box constraints
// (include/proxsuite/proxqp/dense/compute_ECJ.hpp, parallel/qp_solve.hpp) against numbers the Python test computed with
// the oracle on the same QPs stated with the bounds as rows of C (tests/test_cpp_backward_box.py writes them into the
// file named on the command line).  Linked against the emulator build of the device code or against libproxqp_hip.so.
#include <cmath>
#include <cstdio>
#include <vector>

#include <proxsuite/proxqp/dense/dense.hpp>
#include <proxsuite/proxqp/parallel/qp_solve.hpp>

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
read(std::FILE* f, isize count)
{
  std::vector<T> v(static_cast<usize>(count));
  for (auto& e : v)
    if (std::fscanf(f, "%lf", &e) != 1)
      std::printf("FAILED: short input file\n"), ++failures;
  return v;
}

static dense::Mat<T>
mat(const std::vector<T>& v, isize r, isize c)
{
  dense::Mat<T> m(r, c);
  for (isize i = 0; i < r * c; ++i)
    m.data()[i] = v[usize(i)];
  return m;
}

static dense::Vec<T>
vec(const std::vector<T>& v)
{
  dense::Vec<T> o(isize(v.size()));
  for (usize i = 0; i < v.size(); ++i)
    o[isize(i)] = v[i];
  return o;
}

// the project's device-versus-oracle gate of this pass: max |got - ref| <= 1e-6 (1 + max |ref|)
static void
gate(const T* got, const std::vector<T>& ref, const char* what, isize qp)
{
  T worst = 0, top = 0;
  for (usize i = 0; i < ref.size(); ++i) {
    worst = std::fmax(worst, std::fabs(got[i] - ref[i]));
    top = std::fmax(top, std::fabs(ref[i]));
  }
  std::printf("QP %ld %s: max |difference| %.3g (gate %.3g)\n", long(qp), what, worst, 1e-6 * (1 + top));
  EXPECT(worst <= 1e-6 * (1 + top));
}

struct Instance
{
  dense::Mat<T> H, A, C;
  dense::Vec<T> g, b, l, u, lb, ub, ld;
  std::vector<T> dH, dg, dA, db, dC, du, dl, dlb, dub;
};

static void
gate_all(const dense::BackwardData<T>& bd, const Instance& e, isize i)
{
  gate(bd.dL_dH.data(), e.dH, "dL_dH", i);
  gate(bd.dL_dg.data(), e.dg, "dL_dg", i);
  gate(bd.dL_dA.data(), e.dA, "dL_dA", i);
  gate(bd.dL_db.data(), e.db, "dL_db", i);
  gate(bd.dL_dC.data(), e.dC, "dL_dC", i);
  gate(bd.dL_du.data(), e.du, "dL_du", i);
  gate(bd.dL_dl.data(), e.dl, "dL_dl", i);
  gate(bd.dL_dl_box.data(), e.dlb, "dL_dl_box", i);
  gate(bd.dL_du_box.data(), e.dub, "dL_du_box", i);
}

int
main(int argc, char** argv)
{
  if (argc < 2) {
    std::printf("usage: %s <values file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f)
    return 2;
  long B = 0, n = 0, ne = 0, ni = 0;
  if (std::fscanf(f, "%ld %ld %ld %ld", &B, &n, &ne, &ni) != 4)
    return 2;
  const isize ntot = n + ne + ni + n;
  std::vector<Instance> inst;
  for (long i = 0; i < B; ++i) {
    Instance e;
    e.H = mat(read(f, n * n), n, n);
    e.g = vec(read(f, n));
    e.A = mat(read(f, ne * n), ne, n);
    e.b = vec(read(f, ne));
    e.C = mat(read(f, ni * n), ni, n);
    e.l = vec(read(f, ni));
    e.u = vec(read(f, ni));
    e.lb = vec(read(f, n));
    e.ub = vec(read(f, n));
    e.ld = vec(read(f, ntot));
    e.dH = read(f, n * n);
    e.dg = read(f, n);
    e.dA = read(f, ne * n);
    e.db = read(f, ne);
    e.dC = read(f, ni * n);
    e.du = read(f, ni);
    e.dl = read(f, ni);
    e.dlb = read(f, n);
    e.dub = read(f, n);
    inst.push_back(std::move(e));
  }
  std::fclose(f);

  // compute_backward on a dense::QP with box constraints
  {
    const Instance& e = inst[0];
    dense::QP<T> qp{ n, ne, ni, true };
    EXPECT(qp.is_box_constrained());
    qp.settings.eps_abs = 1e-9;
    qp.settings.eps_rel = 0;
    qp.init(e.H, e.g, e.A, e.b, e.C, e.l, e.u, e.lb, e.ub, false);
    qp.solve();
    EXPECT(qp.results.info.status == QPSolverOutput::PROXQP_SOLVED);
    dense::compute_backward<T>(qp, e.ld, 1e-5, 1e-7, 1e-7);
    gate_all(qp.model.backward_data, e, 0);
    EXPECT(qp.results.info.rho == 1e-7 && qp.results.info.mu_eq == 1e-7 && qp.results.info.mu_in == 1e-7);
    // K rows in one call and the jacobians of x
    qp.solve();
    dense::Mat<T> rows(2, ntot);
    for (isize k = 0; k < ntot; ++k)
      rows(1, k) = e.ld[k];
    rows(0, 0) = 1;
    std::vector<std::int32_t> active;
    const dense::Mat<T> V = dense::compute_backward_multi<T>(qp, dense::MatRef<T>(rows), 1e-5, 1e-7, 1e-7, &active);
    EXPECT(V.rows() == 2 && V.cols() == ntot && isize(active.size()) == ni + n);
    gate(&V(1, 0), e.dg, "row of compute_backward_multi, V_x", 0);
    qp.solve();
    const dense::SolutionJacobians<T> J = dense::solution_jacobians<T>(qp, 1e-5, 1e-7, 1e-7);
    EXPECT(J.dx_dl_box.rows() == n && J.dx_dl_box.cols() == n && J.dx_du_box.rows() == n && J.dx_du.cols() == ni);
    bool thrown = false;
    try {
      dense::Vec<T> bad(n + ne + ni); // (the length of a QP without box constraints)
      dense::compute_backward<T>(qp, bad);
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
    EXPECT(thrown);
  }
  // qp_solve_backward_in_parallel over a BatchQP of box QPs, and over a vector of them
  {
    dense::BatchQP<T> bq{ usize(B) };
    std::vector<dense::QP<T>> vq;
    std::vector<dense::Vec<T>> lds;
    for (long i = 0; i < B; ++i) {
      const Instance& e = inst[usize(i)];
      auto& q = bq.init_qp_in_place(n, ne, ni, true);
      vq.emplace_back(n, ne, ni, true);
      for (dense::QP<T>* p : { &q, &vq.back() }) {
        p->settings.eps_abs = 1e-9;
        p->settings.eps_rel = 0;
        p->init(e.H, e.g, e.A, e.b, e.C, e.l, e.u, e.lb, e.ub, false);
      }
      lds.push_back(e.ld);
    }
    dense::solve_in_parallel(bq);
    dense::qp_solve_backward_in_parallel<T>(nullopt, bq, lds, 1e-5, 1e-7, 1e-7);
    for (long i = 0; i < B; ++i)
      gate_all(bq[isize(i)].model.backward_data, inst[usize(i)], i);
    dense::solve_in_parallel(vq);
    dense::qp_solve_backward_in_parallel<T>(nullopt, vq, lds, 1e-5, 1e-7, 1e-7);
    for (long i = 0; i < B; ++i)
      gate_all(vq[usize(i)].model.backward_data, inst[usize(i)], i);
  }
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
