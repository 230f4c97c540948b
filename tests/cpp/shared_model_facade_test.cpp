// dense::BatchQP<T>::init_shared / update_shared of the C++ facade (include/proxsuite/proxqp/dense/wrapper.hpp) against
// the same QPs initialised one by one: H, A, C shared, g, b, l, u per QP, on a single-device batch and on a batch spread
// over two (logical) shards.  The results must agree bit for bit: after init_shared the handle holds what the per-QP
// init calls leave.  The QPs come from the file named on the command line (tests/test_cpp_shared_model.py writes it).
// Linked against the emulator build of the device code or against libproxqp_hip.so.
#include <cstdio>
#include <cstring>
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

template<typename V>
static bool
same_bits(const V& a, const V& b)
{
  return a.size() == b.size() && (a.size() == 0 || std::memcmp(a.data(), b.data(), usize(a.size()) * sizeof(T)) == 0);
}

static void
same_results(dense::BatchQP<T>& a, dense::BatchQP<T>& r, const char* what)
{
  EXPECT(a.size() == r.size());
  for (isize i = 0; i < a.size(); ++i) {
    const bool ok = same_bits(a[i].results.x, r[i].results.x) && same_bits(a[i].results.y, r[i].results.y) &&
                    same_bits(a[i].results.z, r[i].results.z) && a[i].results.info.iter == r[i].results.info.iter &&
                    a[i].results.info.status == r[i].results.info.status;
    if (!ok)
      std::printf("%s: QP %ld differs\n", what, long(i));
    EXPECT(ok);
  }
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
  const dense::Mat<T> H = mat(read(f, n * n), n, n), A = mat(read(f, ne * n), ne, n), C = mat(read(f, ni * n), ni, n);
  const dense::Mat<T> H2 = mat(read(f, n * n), n, n);
  std::vector<dense::Vec<T>> g, b, l, u;
  for (long i = 0; i < B; ++i) {
    g.push_back(vec(read(f, n)));
    b.push_back(vec(read(f, ne)));
    l.push_back(vec(read(f, ni)));
    u.push_back(vec(read(f, ni)));
  }
  std::fclose(f);

  for (int shards = 1; shards <= 2; ++shards) {
    const std::vector<int> devices(usize(shards), 0);
    dense::BatchQP<T> a(usize(B), devices), r(usize(B), devices);
    const isize first = a.init_shared(B, H, g, A, b, C, l, u);
    EXPECT(first == 0 && a.size() == B);
    for (long i = 0; i < B; ++i) {
      auto& q = r.init_qp_in_place(n, ne, ni);
      q.init(H, g[usize(i)], A, b[usize(i)], C, l[usize(i)], u[usize(i)]);
    }
    for (dense::BatchQP<T>* p : { &a, &r })
      for (isize i = 0; i < p->size(); ++i) {
        (*p)[i].settings.eps_abs = 1e-9;
        (*p)[i].settings.eps_rel = 0;
      }
    dense::solve_in_parallel(a);
    dense::solve_in_parallel(r);
    same_results(a, r, shards == 1 ? "init_shared" : "init_shared over two shards");
    for (isize i = 0; i < a.size(); ++i) {
      EXPECT(a[i].results.info.status == QPSolverOutput::PROXQP_SOLVED);
      EXPECT(same_bits(a[i].model.H, r[i].model.H) && same_bits(a[i].model.g, r[i].model.g) &&
             same_bits(a[i].model.C, r[i].model.C) && same_bits(a[i].model.u, r[i].model.u));
    }
    // a new shared H and per-QP g for all of them; then one QP on its own
    a.update_shared(H2, g, nullopt, nullopt, nullopt, nullopt, nullopt);
    for (isize i = 0; i < r.size(); ++i)
      r[i].update(H2, g[usize(i)], nullopt, nullopt, nullopt, nullopt, nullopt);
    a[1].update(nullopt, g[0], nullopt, nullopt, nullopt, nullopt, nullopt);
    r[1].update(nullopt, g[0], nullopt, nullopt, nullopt, nullopt, nullopt);
    dense::solve_in_parallel(a);
    dense::solve_in_parallel(r);
    same_results(a, r, "update_shared");
    EXPECT(same_bits(a[1].model.g, g[0]) && same_bits(a[2].model.H, H2));
    // a per-QP argument of the wrong length
    bool thrown = false;
    try {
      std::vector<dense::Vec<T>> few(g.begin(), g.begin() + 2);
      a.update_shared(nullopt, few, nullopt, nullopt, nullopt, nullopt, nullopt);
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
    EXPECT(thrown);
  }
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
