// Batched dense::estimate_minimal_eigen_value_of_symmetric_matrix (reference dense/helpers.hpp:24-166): ONE workgroup
// of 256 threads per matrix, `count` matrices per launch (pqp_estimate_min_eigenvalues of include/proxqp_hip.h).
//
//   PowerIteration  the reference's two loops restated step for step (helpers.hpp:24-113, 144-159): vectors in LDS, H in
//                   LDS when it fits beside them (eig_resident) and streamed from HBM otherwise, every mat-vec row read by
//                   consecutive lanes of one wavefront.  The stop decision is taken from a block reduction, which hands
//                   every thread the same value: uniform before the next barrier.
//   ExactMethod     Householder tridiagonalisation of a working copy (LDS when it fits, else a per-matrix slice of an HBM
//                   scratch buffer of the entry point), then the smallest eigenvalue of the tridiagonal matrix by
//                   multisection of its Sturm count: 256 shifts per round, one per thread.
//
// Per matrix the kernel also leaves ||H - H^T||_F and ||H||_F for the entry point's symmetry check.
// Only translation unit 19 of pqp_kernels.hip instantiates anything of this header (and pqp_capi.hip reads its host
// half: EigArgs, the LDS sizes and the launcher's declaration).
#ifndef PQP_EIG_HPP
#define PQP_EIG_HPP

#include "pqp_block.hpp"
#include "pqp_types.h"

namespace pqp {

constexpr int EIG_NT = 256;
// order up to which the matrix (PowerIteration) / the working copy (ExactMethod) lives in LDS beside the two vectors
constexpr int EIG_RESIDENT_MAX = 128;
constexpr int EIG_MAX_ROUNDS = 160; // of the multisection: 1074 + 53 bits at 8 bits per round are 141

struct EigArgs
{
  const double* H; // [count][n][n] row-major, device-readable, read only
  double* res;     // [count][3]: the estimate, ||H - H^T||_F, ||H||_F
  double* work;    // ExactMethod, not resident: [count][n][n] working copies
  double accuracy; // power_iteration_accuracy
  long nb;         // nb_power_iteration
  int n;
  int method; // pqp_eig_method
  int resident;
};

inline bool
eig_resident(int n)
{
  return n <= EIG_RESIDENT_MAX;
}

// dynamic LDS of a launch: the reduction scratch, two vectors of n and, when resident, n x n
inline size_t
eig_lds_bytes(int n, bool resident)
{
  return sizeof(double) * (size_t(2 * RED_VALS * (EIG_NT / WAVE)) + 2 * size_t(n) + (resident ? size_t(n) * size_t(n) : 0));
}

#if defined(PQP_EIG_DEVICE)

// out = M v (M symmetric, row i read by the consecutive lanes of one wavefront), optionally dom v - M v; returns this
// thread's share of v . out and of ||out||^2 (non-zero in lane 0 of every wavefront)
template<int NT, class MP>
__device__ __forceinline__ void
eig_matvec(MP M, int n, clptr v, lptr out, bool shifted, double dom, double& dot, double& nrm2)
{
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  dot = 0;
  nrm2 = 0;
  for (int i = wave; i < n; i += NW) {
    const long r = (long)i * n;
    double acc = 0;
    for (int j = lane; j < n; j += WAVE)
      acc += M[r + j] * v[j];
    acc = wave_sum(acc);
    if (shifted) { // helpers.hpp:98-99
      acc = -acc;
      acc += dom * v[i];
    }
    if (lane == 0) {
      out[i] = acc;
      dot += v[i] * acc;
      nrm2 += acc * acc;
    }
  }
}

// helpers.hpp:24-64 (shifted: 65-113, the iteration on dom I - H; the caller subtracts)
template<int NT, class MP>
__device__ __forceinline__ double
eig_power_loop(MP M, int n, lptr rhs, lptr dw, Reducer<NT>& R, bool shifted, double dom, double accuracy, long nb)
{
  const double start = 1. / sqrt((double)n);
  for (int i = threadIdx.x; i < n; i += NT)
    rhs[i] = start;
  __syncthreads();
  double dot, nrm2;
  eig_matvec<NT>(M, n, rhs, dw, shifted, dom, dot, nrm2);
  R.sum2(dot, nrm2);
  double eig = 0;
  for (long it = 0; it < nb; ++it) {
    const double nrm = sqrt(nrm2);
    for (int i = threadIdx.x; i < n; i += NT)
      rhs[i] = dw[i] / nrm;
    __syncthreads();
    eig_matvec<NT>(M, n, rhs, dw, shifted, dom, dot, nrm2);
    R.sum2(dot, nrm2);
    eig = dot;
    double err = 0;
    for (int i = threadIdx.x; i < n; i += NT) {
      // (a NaN must reach the reduction as the reference's infty_norm keeps it: fmax would drop it)
      const double e = fabs(dw[i] - eig * rhs[i]);
      err = (e != e || e > err) ? e : err;
    }
    // every thread holds the same reduced value: the branch is uniform over the workgroup
    const double bad = R.max(err != err ? __builtin_inf() : err);
    if (bad <= accuracy)
      break;
  }
  return eig;
}

// Householder tridiagonalisation of the symmetric n x n matrix A (both triangles kept), in place: afterwards the
// diagonal of A is the tridiagonal matrix's and A[k][k + 1] its off-diagonal.  v, p: two vectors of n in LDS.
template<int NT, class AP>
__device__ __forceinline__ void
eig_tridiagonalise(AP A, int n, lptr v, lptr p, Reducer<NT>& R)
{
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int k = 0; k + 2 < n; ++k) {
    const long rk = (long)k * n;
    double s = 0;
    for (int j = k + 2 + (int)threadIdx.x; j < n; j += NT) {
      const double x = A[rk + j];
      s += x * x;
    }
    const double sigma = R.sum(s);
    // the part of the column below the sub-diagonal is already zero (diagonal H, zero H): no reflector, and no division
    // by its zero norm
    if (sigma == 0.0)
      continue;
    const double alpha = A[rk + k + 1];
    const double beta = -copysign(sqrt(alpha * alpha + sigma), alpha);
    const double tau = (beta - alpha) / beta;
    const double scal = 1.0 / (alpha - beta);
    for (int j = k + 1 + (int)threadIdx.x; j < n; j += NT)
      v[j] = (j == k + 1) ? 1.0 : A[rk + j] * scal;
    __syncthreads();
    // p = tau A22 v on the trailing block, and p . v
    double pv = 0;
    for (int i = k + 1 + wave; i < n; i += NW) {
      const long r = (long)i * n;
      double acc = 0;
      for (int j = k + 1 + lane; j < n; j += WAVE)
        acc += A[r + j] * v[j];
      acc = wave_sum(acc) * tau;
      if (lane == 0) {
        p[i] = acc;
        pv += acc * v[i];
      }
    }
    const double hc = 0.5 * tau * R.sum(pv);
    if (threadIdx.x == 0) // (every thread has read alpha: the reduction above is a barrier)
      A[rk + k + 1] = beta;
    // A22 -= v w^T + w v^T with w = p - (tau / 2)(p . v) v
    for (int i = k + 1 + wave; i < n; i += NW) {
      const long r = (long)i * n;
      const double vi = v[i], wi = p[i] - hc * vi;
      for (int j = k + 1 + lane; j < n; j += WAVE) {
        const double vj = v[j], wj = p[j] - hc * vj;
        A[r + j] -= vi * wj + wi * vj;
      }
    }
    __syncthreads();
  }
}

// smallest eigenvalue of the tridiagonal matrix (diagonal d, SQUARED off-diagonal e2, both in LDS) inside the bracket
// (lo, hi] that Gershgorin's discs give: every thread runs the Sturm recurrence at a shift of its own
template<int NT>
__device__ __forceinline__ double
eig_multisection(clptr d, clptr e2, int n, double lo, double hi, Reducer<NT>& R)
{
  // count(a) = 0 and count(b) >= 1 throughout, count(x) = number of eigenvalues <= x (a zero pivot counts as negative)
  const double width = fmax(fabs(lo), fabs(hi)) * (4.0 * n) * 1.1102230246251565e-16 + 4.9406564584124654e-324;
  double a = lo - width, b = hi + width;
  for (int round = 0; round < EIG_MAX_ROUNDS; ++round) {
    // no double lies strictly inside the bracket (scale-free: matrices of norm 1e-8 and 1e8 end at the same relative place)
    if (!(nextafter(a, __builtin_inf()) < b))
      break;
    const double x = a + (b - a) * ((threadIdx.x + 1.0) / (NT + 1.0));
    double q = d[0] - x;
    if (q == 0.0)
      q = -2.2250738585072014e-308;
    int cnt = q < 0.0;
    for (int i = 1; i < n; ++i) {
      q = d[i] - x - e2[i - 1] / q;
      if (q == 0.0)
        q = -2.2250738585072014e-308; // a zero pivot: a tiny negative number
      cnt += q < 0.0;
    }
    const bool inside = x > a && x < b;
    const double na = R.max((inside && cnt == 0) ? x : a);
    const double nb = R.min((inside && cnt > 0) ? x : b);
    if (!(na < nb)) // (counts that are not monotone in the last bits: keep the bracket that is known to hold)
      break;
    a = na;
    b = nb;
  }
  return b;
}

template<int NT, class AP>
__device__ __forceinline__ double
eig_exact(AP A, int n, lptr v, lptr p, Reducer<NT>& R)
{
  eig_tridiagonalise<NT>(A, n, v, p, R);
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int i = threadIdx.x; i < n; i += NT) {
    const double di = A[(long)i * n + i];
    const double eu = i > 0 ? A[(long)(i - 1) * n + i] : 0.0, el = i + 1 < n ? A[(long)i * n + i + 1] : 0.0;
    v[i] = di;
    p[i] = el * el;
    const double rad = fabs(eu) + fabs(el);
    lo = fmin(lo, di - rad);
    hi = fmax(hi, di + rad);
  }
  lo = R.min(lo);
  hi = R.max(hi);
  return eig_multisection<NT>(v, p, n, lo, hi, R);
}

template<int NT, int METHOD>
__device__ __forceinline__ void
eig_body(const EigArgs& a, long q, lptr smem)
{
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int n = a.n;
  const long nn = (long)n * n;
  Reducer<NT> R(smem);
  lptr v = smem + 2 * RED_VALS * NW, p = v + n, Hs = p + n;
  cgptr H = (cgptr)(a.H + q * nn);
  const bool resident = a.resident != 0;
  if (resident) {
    for (long i = threadIdx.x; i < nn; i += NT)
      Hs[i] = H[i];
    __syncthreads();
  }
  // ||H - H^T||_F and ||H||_F
  double sd = 0, sn = 0;
  for (int i = wave; i < n; i += NW)
    for (int j = lane; j < n; j += WAVE) {
      const double x = resident ? Hs[(long)i * n + j] : H[(long)i * n + j];
      const double y = resident ? Hs[(long)j * n + i] : H[(long)j * n + i];
      sd += (x - y) * (x - y);
      sn += x * x;
    }
  R.sum2(sd, sn);
  double value;
  if constexpr (METHOD == PQP_EIG_POWER_ITERATION) {
    double dom, eig2;
    if (resident) {
      dom = eig_power_loop<NT>((clptr)Hs, n, v, p, R, false, 0.0, a.accuracy, a.nb);
      eig2 = eig_power_loop<NT>((clptr)Hs, n, v, p, R, true, dom, a.accuracy, a.nb);
    } else {
      dom = eig_power_loop<NT>(H, n, v, p, R, false, 0.0, a.accuracy, a.nb);
      eig2 = eig_power_loop<NT>(H, n, v, p, R, true, dom, a.accuracy, a.nb);
    }
    const double min_eig = dom - eig2;
    value = (dom < min_eig) ? dom : min_eig; // std::min(min_eigenvalue, dominant_eigen_value), helpers.hpp:158
  } else {
    // the working copy: the lower triangle of H mirrored (what a self-adjoint solver reads)
    if (resident) {
      for (int i = wave; i < n; i += NW)
        for (int j = lane; j < i; j += WAVE)
          Hs[(long)j * n + i] = Hs[(long)i * n + j];
      __syncthreads();
      value = eig_exact<NT>(Hs, n, v, p, R);
    } else {
      gptr W = (gptr)(a.work + q * nn);
      for (int i = wave; i < n; i += NW)
        for (int j = lane; j < n; j += WAVE)
          W[(long)i * n + j] = j <= i ? H[(long)i * n + j] : H[(long)j * n + i];
      __syncthreads(); // (orders the global accesses of the workgroup as it does the LDS ones)
      value = eig_exact<NT>(W, n, v, p, R);
    }
  }
  if (threadIdx.x == 0) {
    a.res[3 * q] = value;
    a.res[3 * q + 1] = sqrt(sd);
    a.res[3 * q + 2] = sqrt(sn);
  }
}

#endif // PQP_EIG_DEVICE

} // namespace pqp

// `p` may be dereferenced by a kernel as it is (device, pinned or managed memory); anything else is pageable host memory
inline bool
pqp_device_readable(const void* p)
{
#ifdef PQP_EMULATED
  (void)p; // (the emulated device is the host)
  return true;
#else
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError(); // (older runtimes report a pointer they do not know as an error: not a failure of this call)
    return false;
  }
  return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged;
#endif
}

// one workgroup per matrix on `stream` (pqp_kernels.hip, translation unit 19)
int pqp_launch_eig(const pqp::EigArgs& a, long count, hipStream_t stream);

#endif
