// proxsuite/proxqp/dense/compute_ECJ.hpp -- dense::compute_backward on MI355X: derivatives of a
// loss wrt (H, g, A, b, C, u, l) of a SOLVED QP given dL/d(x, y, z), written to
// qp.model.backward_data.  Same signature and defaults as the reference
// (include/proxsuite/proxqp/dense/compute_ECJ.hpp:29-132); the work is one launch of
// pqp_backward_kernel through pqp_batch_backward_range (include/proxqp_hip.h).  compute_backward_multi /
// solution_jacobians: K loss derivatives of one QP in one launch (pqp_batch_backward_multi).  compute_forward_sensitivity:
// the opposite direction, tangents of (x, y, z) for K tangents of the parameters (pqp_batch_tangent_multi).
// A QP with box constraints (is_box_constrained()) goes through pqp_batch_backward_box: its constraint list is [C; I], a
// loss derivative has dim + n_eq + n_in + dim entries (dL/dx | dL/dy | dL/dz_in | dL/dz_box), and backward_data also
// receives dL_dl_box / dL_du_box.
#ifndef PROXSUITE_AMD_PROXQP_DENSE_COMPUTE_ECJ_HPP
#define PROXSUITE_AMD_PROXQP_DENSE_COMPUTE_ECJ_HPP

#include <cstdint>
#include <vector>

#include "proxsuite/proxqp/dense/wrapper.hpp"

namespace proxsuite {
namespace proxqp {
namespace dense {

namespace detail {
template<typename T>
inline void
pull_backward(QP<T>& qp)
{
  BackwardData<T>& bd = qp.model.backward_data;
  bd.initialize(qp.model.dim, qp.model.n_eq, qp.model.n_in);
  check(pqp_batch_get_backward(qp.pool()->h, qp.slot(), bd.dL_dH.data(), bd.dL_dg.data(), bd.dL_dA.data(),
                               bd.dL_db.data(), bd.dL_dC.data(), bd.dL_du.data(), bd.dL_dl.data()));
  if (qp.is_box_constrained())
    check(pqp_batch_get_backward_box(qp.pool()->h, qp.slot(), bd.dL_dl_box.data(), bd.dL_du_box.data()));
}

// entries of a loss derivative / of a row (V_x, V_y, V_z): the inequality part covers [C; I] for a QP with box constraints
template<typename T>
inline isize
backward_width(const QP<T>& qp)
{
  return qp.model.dim + qp.model.n_eq + qp.model.n_in + (qp.is_box_constrained() ? qp.model.dim : 0);
}
} // namespace detail

template<typename T>
void
compute_backward(QP<T>& solved_qp, VecRef<T> loss_derivative, T eps = 1.E-4, T rho_new = 1.E-6, T mu_new = 1.E-6)
{
  const isize ntot = detail::backward_width(solved_qp);
  if (loss_derivative.size() != ntot)
    detail::bad_size(solved_qp.is_box_constrained() ? "the loss derivative has dim + n_eq + n_in + dim entries."
                                                    : "the loss derivative has dim + n_eq + n_in entries.",
                     loss_derivative.size(), ntot);
  std::vector<T> tmp;
  const T* p = loss_derivative.ptr;
  if (loss_derivative.stride != 1) {
    tmp.resize(usize(ntot));
    for (isize i = 0; i < ntot; ++i)
      tmp[usize(i)] = loss_derivative[i];
    p = tmp.data();
  }
  detail::PoolLock lock(solved_qp.pool()->mtx); // (the pool's handle is shared with the other QPs of the pool)
  solved_qp.push_settings();
  if (solved_qp.is_box_constrained())
    detail::check(pqp_batch_backward_box(solved_qp.pool()->h, solved_qp.slot(), 1, 1, p, eps, rho_new, mu_new, nullptr, nullptr));
  else
    detail::check(pqp_batch_backward_range(solved_qp.pool()->h, solved_qp.slot(), 1, p, eps, rho_new, mu_new));
  detail::pull_backward(solved_qp);
  solved_qp.pull(); // results.info carries the backward proximal parameters, as in the reference
}

// compute_backward for K loss derivatives (the rows of `loss_derivatives`, K x (dim + n_eq + n_in)) of one solved QP in
// ONE launch (pqp_batch_backward_multi): the factorisation at (rho_new, mu_new) is done once, the refined KKT solve per
// row.  Returns the K x (dim + n_eq + n_in) matrix of rows (V_x, V_y, V_z): dL_dg = V_x, dL_db = -V_y, dL_du / dL_dl =
// -V_z where the constraint is active from above / below (`active`, optional: n_in flags, bit 0 above, bit 1 below).
// qp.model.backward_data is left alone.  With box constraints: rows of dim + n_eq + n_in + dim entries
// (V_x, V_y, V_zin, V_zbox) and n_in + dim flags.
template<typename T>
Mat<T>
compute_backward_multi(QP<T>& solved_qp,
                       MatRef<T> loss_derivatives,
                       T eps = 1.E-4,
                       T rho_new = 1.E-6,
                       T mu_new = 1.E-6,
                       std::vector<std::int32_t>* active = nullptr)
{
  const bool box = solved_qp.is_box_constrained();
  const isize ntot = detail::backward_width(solved_qp);
  if (loss_derivatives.cols() != ntot)
    detail::bad_size(box ? "a loss derivative has dim + n_eq + n_in + dim entries." : "a loss derivative has dim + n_eq + n_in entries.",
                     loss_derivatives.cols(), ntot);
  const isize K = loss_derivatives.rows();
  Mat<T> ld(K, ntot), out(K, ntot);
  for (isize k = 0; k < K; ++k)
    for (isize i = 0; i < ntot; ++i)
      ld(k, i) = loss_derivatives(k, i);
  std::vector<std::int32_t> flags(usize(solved_qp.model.n_in + (box ? solved_qp.model.dim : 0)), 0);
  detail::PoolLock lock(solved_qp.pool()->mtx);
  solved_qp.push_settings();
  detail::check((box ? pqp_batch_backward_box : pqp_batch_backward_multi)(solved_qp.pool()->h, solved_qp.slot(), 1, K, ld.data(), eps,
                                                                          rho_new, mu_new, out.data(), flags.data()));
  solved_qp.pull(); // results.info carries the backward proximal parameters, as after compute_backward
  if (active)
    *active = flags;
  return out;
}

// The jacobians of the solution x of a solved QP wrt its vectors, from ONE call with the K = dim loss derivatives
// [I | 0]: row i holds compute_backward's dL_dg, dL_db, dL_du, dL_dl for the loss x_i.
template<typename T>
struct SolutionJacobians
{
  Mat<T> dx_dg, dx_db, dx_du, dx_dl; // dim x dim, dim x n_eq, dim x n_in, dim x n_in
  Mat<T> dx_dl_box, dx_du_box;       // dim x dim for a QP with box constraints, empty otherwise
};

template<typename T>
SolutionJacobians<T>
solution_jacobians(QP<T>& solved_qp, T eps = 1.E-4, T rho_new = 1.E-6, T mu_new = 1.E-6)
{
  const isize n = solved_qp.model.dim, ne = solved_qp.model.n_eq, ni = solved_qp.model.n_in;
  const bool box = solved_qp.is_box_constrained();
  Mat<T> ld(n, detail::backward_width(solved_qp));
  for (isize i = 0; i < n; ++i)
    ld(i, i) = T(1);
  std::vector<std::int32_t> active;
  const Mat<T> V = compute_backward_multi(solved_qp, MatRef<T>(ld), eps, rho_new, mu_new, &active);
  SolutionJacobians<T> J{ Mat<T>(n, n), Mat<T>(n, ne), Mat<T>(n, ni), Mat<T>(n, ni), Mat<T>(), Mat<T>() };
  if (box) {
    J.dx_dl_box.resize(n, n);
    J.dx_du_box.resize(n, n);
  }
  for (isize i = 0; i < n; ++i) {
    for (isize k = 0; box && k < n; ++k) {
      J.dx_du_box(i, k) = (active[usize(ni + k)] & 1) ? -V(i, n + ne + ni + k) : T(0);
      J.dx_dl_box(i, k) = (active[usize(ni + k)] & 2) ? -V(i, n + ne + ni + k) : T(0);
    }
    for (isize k = 0; k < n; ++k)
      J.dx_dg(i, k) = V(i, k);
    for (isize k = 0; k < ne; ++k)
      J.dx_db(i, k) = -V(i, n + k);
    for (isize k = 0; k < ni; ++k) {
      J.dx_du(i, k) = (active[usize(k)] & 1) ? -V(i, n + ne + k) : T(0);
      J.dx_dl(i, k) = (active[usize(k)] & 2) ? -V(i, n + ne + k) : T(0);
    }
  }
  return J;
}

// Tangents of the parameters of one QP, K = n_dir directions: every array is optional (null: a zero tangent), row-major,
// direction-major -- dH [K][dim][dim] (need not be symmetric: its symmetric part acts), dg [K][dim], dA [K][n_eq][dim],
// db [K][n_eq], dC [K][n_in][dim], dl / du [K][n_in].
template<typename T>
struct Tangents
{
  const T *dH = nullptr, *dg = nullptr, *dA = nullptr, *db = nullptr, *dC = nullptr, *dl = nullptr, *du = nullptr;
  isize n_dir = 1;
};

// K x dim, K x n_eq, K x n_in (inactive rows of dz are 0) and the n_in flags (bit 0: active from above, bit 1: from below)
template<typename T>
struct ForwardSensitivity
{
  Mat<T> dx, dy, dz;
  std::vector<std::int32_t> active;
};

// Forward-mode sensitivities of a solved QP (pqp_batch_tangent_multi, the adjoint of compute_backward): by how much
// (x, y, z) move when the parameters move by `tangents`, one refined KKT solve per direction on one factorisation at
// (rho_new, mu_new).  qp.model.backward_data is left alone.  A QP with box constraints throws (no box tangents).
template<typename T>
ForwardSensitivity<T>
compute_forward_sensitivity(QP<T>& solved_qp, const Tangents<T>& tangents, T eps = 1.E-4, T rho_new = 1.E-6, T mu_new = 1.E-6)
{
  const isize n = solved_qp.model.dim, ne = solved_qp.model.n_eq, ni = solved_qp.model.n_in, ntot = n + ne + ni;
  const isize K = tangents.n_dir;
  if (K < 0)
    detail::bad_size("the number of directions is not negative.", K, 0);
  Mat<T> out(K, ntot);
  ForwardSensitivity<T> r{ Mat<T>(K, n), Mat<T>(K, ne), Mat<T>(K, ni), std::vector<std::int32_t>(usize(ni), 0) };
  if (K == 0)
    return r;
  detail::PoolLock lock(solved_qp.pool()->mtx);
  solved_qp.push_settings();
  detail::check(pqp_batch_tangent_multi(solved_qp.pool()->h, solved_qp.slot(), 1, K, tangents.dH, tangents.dg, tangents.dA,
                                        tangents.db, tangents.dC, tangents.dl, tangents.du, 0, eps, rho_new, mu_new, out.data(),
                                        r.active.data(), nullptr));
  solved_qp.pull(); // results.info carries the backward proximal parameters, as after compute_backward
  for (isize k = 0; k < K; ++k) {
    for (isize i = 0; i < n; ++i)
      r.dx(k, i) = out(k, i);
    for (isize i = 0; i < ne; ++i)
      r.dy(k, i) = out(k, n + i);
    for (isize i = 0; i < ni; ++i)
      r.dz(k, i) = out(k, n + ne + i);
  }
  return r;
}

} // namespace dense
} // namespace proxqp
} // namespace proxsuite

#endif
