// Backward pass of the closest-feasible QPLayer (QPFunction(structural_feasibility=False); reference
// bindings/python/proxsuite/torch/qplayer.py:371-610) on the device.  The reference assembles, per solved QP, a
// rectangular linear system K w = r and hands it to ProxQP as a QP with zero Hessian, K as equality constraints, no
// inequalities and primal_infeasibility_solving on: a dense (n_col, n_row, 0) QP of the kind this engine solves.
//   pqp_infeas_kkt_kernel   assembles K and r of every QP of a pass DIRECTLY in the model arrays (A, b) of an inner batch
//                           handle, where pqp_batch_init would have copied them
//   pqp_infeas_grad_kernel  turns the inner solution w = (dx, dlam, dnu, t, b5, b6) into the seven jacobians of the
//                           single-sided QP, in the forward handle's backward arrays (pqp_batch_get_backward)
// The QP is single-sided (G1 x <= u, every l at -1e20): dim = n, n_eq, n_in rows.  With s = G1 x - u,
// P1 = (min(s, 0) + z >= 0), P2 = (s <= 0), D1 = diag(P1), D2 = diag(P2), D1c = I - D1, D2c = I - D2:
//
//               dx    dlam   dnu    t        b5 (n_eq > 0)  b6
//   dim       [ H     A^T    G1^T   .        .              .       ]   r = -dl/dx
//   n_eq      [ A     .      .      .        .              .       ]       -dl/dlam
//   n_in      [ G1    .      .      D1c      .              .       ]       -dl/dnu
//   n_eq      [ .     -I     .      .        A              .       ]       -dl/dse
//   n_in      [ .     .      -I     -D1 D2   .              D2c G1  ]       -dl/dsi
#ifndef PQP_INFEAS_HPP
#define PQP_INFEAS_HPP

#include "pqp_solver.hpp"

namespace pqp {

__host__ __device__ inline int
infeas_rows(int dim, int ne, int ni)
{
  return dim + 2 * ni + 2 * ne;
}
__host__ __device__ inline int
infeas_cols(int dim, int ne, int ni)
{
  return 2 * dim + 2 * ni + ne + (ne > 0 ? dim : 0);
}

constexpr int INFEAS_TILE = 32; // rows of K per workgroup round; side of the LDS tile the transposed blocks go through

// One pass: the QPs first .. first + count - 1 of the forward handle are the slots 0 .. count - 1 of the inner one.
struct InfeasArgs
{
  const double* ld; // [count][dim + 2 n_eq + 2 n_in]: (dl/dx | dl/dlam | dl/dnu | dl/dse | dl/dsi) per slot
  long first, count;
  double *K, *r;    // the inner handle's A ([.][n_row * n_col], row-major) and b ([.][n_row])
  const double* w;  // the inner handle's x ([.][n_col])
  int* flags;       // [count][n_in]: bit 0 = P1, bit 1 = P2
  double* p2c;      // [count][n_in]: max(s, 0)
  // the formulas are single-sided: the workgroups of the FIRST pass also look at l of every QP of the call's range
  // [check_first, check_first + check_count) and raise *finite_l when an entry is above -1e20 (or NaN)
  int* finite_l;
  long check_first, check_count;
  int shares;       // workgroups per slot
};

#ifdef PQP_INFEAS_DEVICE

// Workgroup slot * shares + j takes the row tiles j, j + shares, ... of K of that slot.  A row is written by one
// wavefront, lane = column (coalesced; the blocks H, A, G1 are read by row the same way); the blocks A^T and G1^T go
// through an LDS tile, read by row of A / G1 and written by row of K.  Every entry is written, zeros included.
template<int NT>
__device__ __forceinline__ void
infeas_kkt_body(const Batch& batch, const InfeasArgs& a)
{
  constexpr int T = INFEAS_TILE, NW = NT / 64, TY = NT / T;
  __shared__ double tile[T][T + 1];
  __shared__ int rowflag[T];
  const int dim = batch.d.n, ne = batch.d.n_eq, ni = batch.d.n_in;
  const int n_row = infeas_rows(dim, ne, ni), n_col = infeas_cols(dim, ne, ni);
  const long slot = blockIdx.x / a.shares;
  const int share = (int)(blockIdx.x - slot * a.shares);
  const long q = a.first + slot;
  const double *H = batch.H + q * dim * dim, *A = batch.A + q * ne * dim, *C = batch.C + q * ni * dim;
  const double *u = batch.u + q * ni, *x = batch.x + q * dim, *z = batch.z + q * batch.d.nc;
  const double* ld = a.ld + slot * n_row;
  double *K = a.K + slot * (long)n_row * n_col, *r = a.r + slot * n_row;
  int* fl = a.flags + slot * ni;
  double* p2c = a.p2c + slot * ni;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_lam = dim, c_nu = dim + ne, c_t = dim + ne + ni, c_b5 = dim + ne + 2 * ni, c_b6 = c_b5 + (ne > 0 ? dim : 0);
  const int r_A = dim, r_G = dim + ne, r_se = dim + ne + ni, r_si = dim + 2 * ne + ni;

  if (share == 0)
    for (long qq = a.check_first + slot; qq < a.check_first + a.check_count; qq += a.count) {
      const double* l = batch.l + qq * ni;
      for (int i = threadIdx.x; i < ni; i += NT)
        if (!(l[i] <= -1.0e20))
          *a.finite_l = 1;
    }

  const int n_tiles = (n_row + T - 1) / T;
  for (int t = share; t < n_tiles; t += a.shares) {
    const int row0 = t * T, rows = (n_row - row0 < T) ? (n_row - row0) : T;
    __syncthreads(); // (rowflag of the previous round is no longer read)
    // P1 / P2 of the inequality rows of this tile: s_i = G1_i x - u_i, one wavefront per row
    for (int rr = wave; rr < rows; rr += NW) {
      const int row = row0 + rr;
      const int i = (row >= r_G && row < r_se) ? row - r_G : (row >= r_si ? row - r_si : -1);
      if (i < 0)
        continue;
      const double* g = C + (long)i * dim;
      double acc = 0.0;
      for (int k = lane; k < dim; k += 64)
        acc += g[k] * x[k];
      for (int m = 32; m > 0; m >>= 1)
        acc += __shfl_xor(acc, m);
      const double s = acc - u[i];
      const int f = ((fmin(s, 0.0) + z[i] >= 0.0) ? 1 : 0) | ((s <= 0.0) ? 2 : 0);
      if (lane == 0) {
        rowflag[rr] = f;
        if (row < r_se) { // (the rows of the last block recompute the same bits)
          fl[i] = f;
          p2c[i] = fmax(s, 0.0);
        }
      }
    }
    __syncthreads();
    for (int rr = wave; rr < rows; rr += NW) {
      const int row = row0 + rr;
      double* Kr = K + (long)row * n_col;
      if (row < r_A) {
        // [ H | (A^T, G1^T: the transposed pass below) | 0 ]
        const double* h = H + (long)row * dim;
        for (int c = lane; c < dim; c += 64)
          Kr[c] = h[c];
        for (int c = c_t + lane; c < n_col; c += 64)
          Kr[c] = 0.0;
      } else if (row < r_G) {
        const double* ar = A + (long)(row - r_A) * dim;
        for (int c = lane; c < n_col; c += 64)
          Kr[c] = c < dim ? ar[c] : 0.0;
      } else if (row < r_se) {
        const int i = row - r_G;
        const double *g = C + (long)i * dim, d1c = (rowflag[rr] & 1) ? 0.0 : 1.0;
        for (int c = lane; c < n_col; c += 64)
          Kr[c] = c < dim ? g[c] : (c == c_t + i ? d1c : 0.0);
      } else if (row < r_si) {
        const int i = row - r_se;
        const double* ar = A + (long)i * dim;
        for (int c = lane; c < n_col; c += 64)
          Kr[c] = c == c_lam + i ? -1.0 : ((c >= c_b5 && c < c_b6) ? ar[c - c_b5] : 0.0);
      } else {
        const int i = row - r_si, f = rowflag[rr];
        const double *g = C + (long)i * dim, d12 = (f & 3) == 3 ? -1.0 : 0.0;
        const bool d2c = (f & 2) == 0;
        for (int c = lane; c < n_col; c += 64)
          Kr[c] = c == c_nu + i ? -1.0 : (c == c_t + i ? d12 : ((c >= c_b6 && d2c) ? g[c - c_b6] : 0.0));
      }
      if (lane == 0)
        r[row] = -ld[row];
    }
    if (row0 < r_A) {
      // K[row][dim + j] = M[j][row], M = [A; G1] (n_eq + n_in rows of dim)
      const int tx = threadIdx.x % T, ty = threadIdx.x / T, nm = ne + ni;
      for (int j0 = 0; j0 < nm; j0 += T) {
        __syncthreads();
        for (int jj = ty; jj < T; jj += TY) {
          const int j = j0 + jj, col = row0 + tx;
          double v = 0.0;
          if (j < nm && col < dim)
            v = j < ne ? A[(long)j * dim + col] : C[(long)(j - ne) * dim + col];
          tile[jj][tx] = v;
        }
        __syncthreads();
        for (int ii = ty; ii < T; ii += TY) {
          const int row = row0 + ii, j = j0 + tx;
          if (row < r_A && j < nm)
            K[(long)row * n_col + dim + j] = tile[tx][ii];
        }
      }
    }
  }
}

// Element-wise, as pqp_backward_outer_kernel: workgroup slot * shares + j takes the j-th share of the entries of the QP
// of that slot.  dL_dH = (dx x^T + x dx^T) / 2, dL_dg = dx, dL_dA = dlam x^T + lam dx^T + se b5^T, dL_db = -dlam,
// dL_dC = dnu x^T + nus dx^T + P2c b6^T, dL_du = -dnu, dL_dl = 0.
template<int NT>
__device__ __forceinline__ void
infeas_grad_body(const Batch& batch, const InfeasArgs& a, const BackwardArgs& bw)
{
  const long n = batch.d.n, ne = batch.d.n_eq, ni = batch.d.n_in;
  const long n_col = infeas_cols((int)n, (int)ne, (int)ni);
  const long slot = blockIdx.x / a.shares, share = blockIdx.x - slot * a.shares;
  const long q = a.first + slot;
  const double* w = a.w + slot * n_col;
  const double *dx = w, *dlam = w + n, *dnu = w + n + ne, *b5 = w + n + ne + 2 * ni, *b6 = b5 + (ne > 0 ? n : 0);
  const double* p2c = a.p2c + slot * ni;
  const double *xs = batch.x + q * n, *ys = batch.y + q * ne, *zs = batch.z + q * batch.d.nc, *ses = batch.se + q * ne;
  double *oH = bw.dL_dH + q * n * n, *og = bw.dL_dg + q * n, *oA = bw.dL_dA + q * ne * n, *ob = bw.dL_db + q * ne;
  double *oC = bw.dL_dC + q * ni * n, *ou = bw.dL_du + q * ni, *ol = bw.dL_dl + q * ni;
  const long t0 = share * NT + threadIdx.x, step = (long)a.shares * NT;
  for (long o = t0; o < n * n; o += step) {
    const long i = o / n, k = o - i * n;
    oH[o] = 0.5 * (dx[i] * xs[k] + xs[i] * dx[k]);
  }
  for (long k = t0; k < n; k += step)
    og[k] = dx[k];
  for (long o = t0; o < ne * n; o += step) {
    const long i = o / n, k = o - i * n;
    oA[o] = dlam[i] * xs[k] + ys[i] * dx[k] + ses[i] * b5[k];
  }
  for (long k = t0; k < ne; k += step)
    ob[k] = -dlam[k];
  for (long o = t0; o < ni * n; o += step) {
    const long i = o / n, k = o - i * n;
    oC[o] = dnu[i] * xs[k] + zs[i] * dx[k] + p2c[i] * b6[k];
  }
  for (long i = t0; i < ni; i += step) {
    ou[i] = -dnu[i];
    ol[i] = 0.0;
  }
}

#endif // PQP_INFEAS_DEVICE

} // namespace pqp

#endif
