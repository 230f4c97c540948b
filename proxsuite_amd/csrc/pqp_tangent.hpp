// Forward-mode sensitivities of a solved QP (tangents, JVP): by how much (x, y, z) move when the parameters move by
// (dH, dg, dA, db, dC, dl, du).  The adjoint of the backward pass of pqp_solver.hpp (Solver::backward / backward_multi).
//
// Conventions.  (x, y, z) is the solution the last solve left; the active flags are those backward() computes from it on
// the unscaled model: bit 0 (up) C x + z - u >= 0, bit 1 (low) C x + z - l <= 0.  For one direction
//     r_x    = 1/2 (dH + dH^T) x + dg + dA^T y + dC^T z
//     r_y    = dA x - db
//     r_z[i] = (dC x)[i] - [up_i] du[i] - [low_i] dl[i]          (active rows i only)
// and the tangent T = (T_x, T_y, T_z) solves the system backward() factorises -- regularised with (rho, mu, mu), restricted
// to the active rows, stated in the equilibrated space -- with right-hand side -r; inactive rows of T_z are 0.  In the
// kernel's variables (c = ruiz_c, dX / dE / dI the scaling vectors, a the slot of active row i):
//     rx = -r_x dX c,   rd_eq = -r_y dE,   rd_in[a] = -r_z[i] dI[i]
//     T_x = dx dX,      T_y = sd dE / c,   T_z[i] = sd[ne + a] dI[i] / c
// With these, <ld, T> = sum over the parameters of <dL/dtheta, dtheta> for the dL/dtheta pqp_batch_backward returns for the
// loss derivative ld: its symmetrised dL_dH is matched by 1/2 (dH + dH^T), its dL_du / dL_dl by the flags.  A row with
// BOTH flags set takes du and dl; such a row needs C x + z = l = u exactly.
//
// Why backward_multi is not reused: it restates two quirks of the reference's compute_backward -- the inequality part of
// its right-hand side is scaled by delta_in[slot] once per remaining loop iteration, and an inactive row of its output is
// the loss derivative at a permuted position.  A loss derivative almost never has a z part; a tangent's right-hand side
// always has one.  So the solve below scales once, by the row's own factor, and writes zeros on inactive rows.
//
//   pqp_tangent_rhs_kernel<256>      R[slot][k][:] = (r_x | r_y | dC x) from the result arrays and the tangent arrays: one
//                                    workgroup per (QP, direction), every tangent matrix read exactly once
//   pqp_tangent_multi_kernel<.>      backward_multi's prologue (flags, factorisation, active set) once per QP, then per
//                                    direction the right-hand side from R, du, dl and the kernel's own flags, the refined KKT
//                                    solve and the unscaling; _hbm_kernel<1024>: the same on an HBM slice per workgroup
#ifndef PQP_TANGENT_HPP
#define PQP_TANGENT_HPP

struct pqp_batch;

namespace pqp {

// Tangent arrays are [count][n_dir][...] row-major (slot-major, as BackwardMultiArgs::ld); a bit PQP_SHARED_* of
// `shared_mask` says ONE [n_dir][...] block serves every QP of the launch (stride 0).  A null array is a zero tangent and
// is never read.
struct TangentRhsArgs
{
  const double *dH, *dg, *dA, *db, *dC;
  int shared_mask;
  double* R; // [count][n_dir][n + n_eq + n_in]
  long n_dir;
  long first;
  const int* order; // optional: workgroups slot * n_dir + k work on QP order[slot]
};

struct TangentArgs
{
  const double* R;       // what pqp_tangent_rhs_kernel wrote
  const double *dl, *du; // [count][n_dir][n_in] or null
  long dl_stride, du_stride; // doubles between the blocks of two slots: n_dir * n_in, or 0 for a shared block
  double eps, rho_new, mu_new;
  double* out; // [count][n_dir][n + n_eq + n_in]: (T_x, T_y, T_z)
  int* active; // optional, [count][n_in]: flags & 3
  long n_dir;
  long first;
  const int* order;
};

// dynamic LDS of the assembly kernel: the row sums of the three matrices and three column partials per wavefront
inline size_t
tangent_rhs_lds_bytes(long n, long ne, long ni, int nt)
{
  return size_t(n + ne + ni + 3L * nt) * sizeof(double);
}

#ifdef PQP_TANGENT_DEVICE

// sum over the 64 lanes of a wavefront, the same butterfly on every call: every lane returns the same bits
__device__ __forceinline__ double
tangent_wave_sum(double v)
{
  for (int m = 32; m >= 1; m >>= 1)
    v += __shfl_xor(v, m);
  return v;
}

// One pass over M ([m][n] row-major) for the columns c0 + lane: returns this thread's share of column c0 + lane of M^T v
// (rows w, w + NW, ... in that order) and adds the share of (M xs)[i] of this column chunk to rows[i] -- row i belongs to
// wavefront i % NW alone, so rows[i] sees the chunks in their order.  A wavefront reads 64 consecutive doubles of a row.
template<int NW>
__device__ __forceinline__ double
tangent_pass(const double* __restrict__ M, long m, long n, long j, bool in, double xj, const double* __restrict__ v,
             double* rows, int w, int lane)
{
  double col = 0.0;
  for (long i = w; i < m; i += NW) {
    const double a = in ? M[i * n + j] : 0.0;
    col += a * v[i];
    const double s = tangent_wave_sum(a * xj);
    if (lane == 0)
      rows[i] += s;
  }
  return col;
}

// Workgroup slot * n_dir + k: row k of QP `slot` of the launch.  Column chunks of 64 are walked one after the other; within
// a chunk dH, dA and dC are each read once (element (i, j) of dH goes to row i and to column j of the symmetrised product).
// Column sums: per thread over its rows, then over the wavefronts in index order; no atomics anywhere.
template<int NT>
__device__ __forceinline__ void
tangent_rhs_body(const Batch& batch, const TangentRhsArgs& a, double* lds)
{
  constexpr int NW = NT / 64;
  const long n = batch.d.n, ne = batch.d.n_eq, ni = batch.d.n_in, ntot = n + ne + ni;
  const long slot = (long)blockIdx.x / a.n_dir, k = (long)blockIdx.x - slot * a.n_dir;
  const long q = a.order ? (long)a.order[slot] : a.first + slot;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const double *x = batch.x + q * n, *y = batch.y + q * ne, *z = batch.z + q * batch.d.nc;
  const long blk = slot * a.n_dir;
  const double* dH = a.dH ? a.dH + (((a.shared_mask & PQP_SHARED_H) ? 0 : blk) + k) * n * n : nullptr;
  const double* dg = a.dg ? a.dg + (((a.shared_mask & PQP_SHARED_G) ? 0 : blk) + k) * n : nullptr;
  const double* dA = a.dA ? a.dA + (((a.shared_mask & PQP_SHARED_A) ? 0 : blk) + k) * ne * n : nullptr;
  const double* db = a.db ? a.db + (((a.shared_mask & PQP_SHARED_B) ? 0 : blk) + k) * ne : nullptr;
  const double* dC = a.dC ? a.dC + (((a.shared_mask & PQP_SHARED_C) ? 0 : blk) + k) * ni * n : nullptr;
  double* R = a.R + (blk + k) * ntot;
  double *rows = lds, *colp = lds + ntot; // colp: [3][NW][64]
  for (long e = tid; e < ntot; e += NT)
    rows[e] = 0.0;
  __syncthreads();
  for (long c0 = 0; c0 < n; c0 += 64) {
    const long j = c0 + lane;
    const bool in = j < n;
    const double xj = in ? x[j] : 0.0;
    if (dH)
      colp[(0 * NW + w) * 64 + lane] = tangent_pass<NW>(dH, n, n, j, in, xj, x, rows, w, lane);
    if (dA)
      colp[(1 * NW + w) * 64 + lane] = tangent_pass<NW>(dA, ne, n, j, in, xj, y, rows + n, w, lane);
    if (dC)
      colp[(2 * NW + w) * 64 + lane] = tangent_pass<NW>(dC, ni, n, j, in, xj, z, rows + n + ne, w, lane);
    __syncthreads();
    if (w == 0 && in) {
      double acc = dg ? dg[j] : 0.0;
      if (dH) {
        double s = colp[lane];
        for (int u = 1; u < NW; ++u)
          s += colp[(0 * NW + u) * 64 + lane];
        acc += 0.5 * s;
      }
      if (dA) {
        double s = colp[(1 * NW) * 64 + lane];
        for (int u = 1; u < NW; ++u)
          s += colp[(1 * NW + u) * 64 + lane];
        acc += s;
      }
      if (dC) {
        double s = colp[(2 * NW) * 64 + lane];
        for (int u = 1; u < NW; ++u)
          s += colp[(2 * NW + u) * 64 + lane];
        acc += s;
      }
      R[j] = acc;
    }
    __syncthreads(); // (the next chunk rewrites colp; R[j] is read below by another thread)
  }
  if (dH)
    for (long e = tid; e < n; e += NT)
      R[e] = R[e] + 0.5 * rows[e];
  for (long e = tid; e < ne; e += NT)
    R[n + e] = dA ? (db ? rows[n + e] - db[e] : rows[n + e]) : (db ? -db[e] : 0.0);
  for (long e = tid; e < ni; e += NT)
    R[n + ne + e] = dC ? rows[n + ne + e] : 0.0;
}

// ---- the K-tangent solve: Solver::backward_multi's prologue up to apply_active_set(), statement for statement (Solver is
// an aggregate of public members, so this lives here and pqp_solver.hpp does not change); then per direction the right-hand
// side of the header comment from R, du, dl and the flags computed HERE, the refined KKT solve, and the unscaling with
// zeros on inactive rows.  The state epilogue is backward_multi's, once per QP.
template<int NT>
__device__ __forceinline__ void
tangent_multi(Solver<NT, 0>& S, const TangentArgs& tg, long slot_in_launch)
{
  auto& L = S.L;
  const auto& P = S.P;
  const int n = S.d.n, ne = S.d.n_eq, ni = S.d.n_in;
  const long ntot = (long)n + ne + ni;
  for (int k = threadIdx.x; k < ST_COUNT; k += NT)
    L.stat()[k] = 0;
  {
    const State& Wr = *P.state();
    S.diag_mode = S.d.hessian != PQP_HESSIAN_DENSE && S.d.n_eq == 0 && Wr.c_diag != 0 && !(S.d.n_in > 0 && S.d.box != 0);
    S.ruiz_c = Wr.ruiz_c;
  }
  S.info.load(*P.info());
  const double c = S.ruiz_c;
  S.vload(L.x(), P.x(), n);
  S.vload(L.y(), P.y(), ne);
  S.vload(L.z(), P.z(), ni);
  cgptr dX = P.dlt_x(), dE = P.dlt_eq(), dI = P.dlt_in();
  for (int k = threadIdx.x; k < n; k += NT)
    L.dx()[k] = P.x()[k] / dX[k]; // x in the equilibrated space
  for (int i = threadIdx.x; i < ni; i += NT) {
    L.aflags()[i] = 0;
    L.slot_of()[i] = -1;
  }
  __syncthreads();
  // active sets at the solution:  C x + z - u >= 0,  C x + z - l <= 0
  if (ni > 0) {
    if (S.dm()) {
      cgptr cd = P.CTs();
      for (int i = threadIdx.x; i < ni; i += NT)
        L.Cdx()[i] = cd[i] * L.dx()[i];
      __syncthreads();
    } else {
      S.mv(P.CTs(), ni, n, ni, L.dx(), L.Cdx());
    }
    cgptr gu = P.u(), gl = P.l();
    for (int i = threadIdx.x; i < ni; i += NT) {
      const double ctz = L.Cdx()[i] / dI[i] + L.z()[i];
      const bool up = (ctz - gu[i]) >= 0., lo = (ctz - gl[i]) <= 0.;
      L.aflags()[i] = (up ? 1 : 0) | (lo ? 2 : 0) | ((up || lo) ? 4 : 0);
    }
    __syncthreads();
  }
  S.info.rho = tg.rho_new;
  S.info.mu_eq = tg.mu_new;
  S.info.mu_in = tg.mu_new;
  S.template factor_primal_block<false>();
  S.n_c = 0;
  S.n_slots = 0;
  S.r = ne;
  S.schur_dirty = true;
  S.apply_active_set();
  for (long row = 0; row < tg.n_dir; ++row) {
    cgptr rr = (cgptr)(tg.R + (slot_in_launch * tg.n_dir + row) * ntot);
    cgptr du = (cgptr)(tg.du ? tg.du + slot_in_launch * tg.du_stride + row * ni : nullptr);
    cgptr dl = (cgptr)(tg.dl ? tg.dl + slot_in_launch * tg.dl_stride + row * ni : nullptr);
    gptr o = (gptr)(tg.out + (slot_in_launch * tg.n_dir + row) * ntot);
    for (int k = threadIdx.x; k < n; k += NT)
      L.rx()[k] = -rr[k] * (dX[k] * c);
    for (int k = threadIdx.x; k < ne; k += NT)
      L.rd()[k] = -rr[n + k] * dE[k];
    for (int i = threadIdx.x; i < ni; i += NT) {
      const int a = L.slot_of()[i];
      if (a >= 0) {
        const int f = L.aflags()[i];
        double v = rr[n + ne + i];
        if (du && (f & 1))
          v -= du[i];
        if (dl && (f & 2))
          v -= dl[i];
        L.rd()[ne + a] = -v * dI[i]; // scaled once, by the row's own factor
      }
    }
    __syncthreads();
    (void)S.iterative_solve(tg.eps);
    for (int k = threadIdx.x; k < n; k += NT)
      o[k] = L.dx()[k] * dX[k];
    for (int k = threadIdx.x; k < ne; k += NT)
      o[n + k] = L.sd()[k] * dE[k] / c;
    for (int j = threadIdx.x; j < ni; j += NT) {
      const int a = L.slot_of()[j];
      o[n + ne + j] = a >= 0 ? L.sd()[ne + a] * dI[j] / c : 0.0;
    }
    __syncthreads(); // (the next direction rewrites the right-hand side and the solution)
  }
  {
    PQP_GLOBAL int* ga = P.act();
    PQP_GLOBAL int* fl = (PQP_GLOBAL int*)(tg.active ? tg.active + slot_in_launch * ni : nullptr);
    for (int i = threadIdx.x; i < ni; i += NT) {
      ga[i] = act_pack(act_cid(ga[i]), L.aflags()[i]);
      if (fl)
        fl[i] = L.aflags()[i] & 3;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    S.info.store(*P.info());
    State& Ww = *P.state();
    Ww.factor_valid = 0;
    Ww.primal_valid = 0; // (the block in HBM was factorised at rho_new)
    Ww.ls_valid = 0;
    Ww.dirty = 1;
  }
}

template<int NT>
__device__ __forceinline__ void
tangent_multi_body(const Batch& batch, const TangentArgs& tg, long slot, lptr lds_base)
{
  Solver<NT, 0> S(batch, tg.order ? (long)tg.order[slot] : tg.first + slot, lds_base);
  tangent_multi<NT>(S, tg, slot);
}

#endif // PQP_TANGENT_DEVICE

} // namespace pqp

// launchers (pqp_kernels.hip, translation units 26 and 27)
int pqp_launch_tangent_rhs(pqp_batch* h, const pqp::TangentRhsArgs& a, long count);
int pqp_launch_tangent_multi(pqp_batch* h, const pqp::TangentArgs& tg, long count);
int pqp_launch_tangent_multi_hbm(pqp_batch* h, const pqp::TangentArgs& tg, long count);

#endif
