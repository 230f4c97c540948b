// Batches that share a model (batched MPC: one H, A, C for every QP; the QPLayer in training: Q, A, G are 2-D weights).
// The handle keeps its per-QP model arrays -- every solver kernel reads them as before -- and two small kernels move the
// shared part across that boundary on the device:
//   pqp_broadcast_kernel<256>  one array of `len` doubles -> dst + q * len for every QP q of a range: what
//                              pqp_batch_init_shared / pqp_batch_update_shared do instead of taking `count` copies over the
//                              host link (pqp_capi.hip: enqueue_setup)
//   pqp_sum_kernel<256>        out[e] = sum over the QPs q of a range of src[q * len + e]: the gradient of a shared
//                              parameter from the per-QP jacobians of a backward pass (pqp_batch_get_backward_sum)
#ifndef PQP_SHARED_HPP
#define PQP_SHARED_HPP

namespace pqp {

// QPs per workgroup of the broadcast: a thread loads its source elements once and stores them to this many QPs
constexpr int BCAST_QPS = 16;

// The order of pqp_sum_kernel, a function of (first, count) alone: the range is cut into chunks of PQP_SUM_CHUNK consecutive
// QPs starting at `first`; a chunk is added up sequentially in index order, starting from its first term; the chunk
// partials are then added sequentially in chunk order, starting from the first.  No atomics: the same bits on every
// device and on the emulator.
constexpr int PQP_SUM_CHUNK = 64;

#ifdef PQP_SHARED_DEVICE

struct alignas(16) BcastPair
{
  double a, b;
};

// Workgroup t + tiles * c: element tile t of QP chunk c (QPs first + c * BCAST_QPS ...).  A pure write stream.  `pairs`:
// `len` is even, so dst + q * len is 16-byte aligned for every q (dst is an allocation of the handle) and a lane stores
// 16 bytes; the source may be any 8-byte aligned device address and is read as doubles.
template<int NT>
__device__ __forceinline__ void
broadcast_body(const double* __restrict__ src, double* __restrict__ dst, long len, long first, long count, long tiles,
               bool pairs)
{
  const long c = (long)blockIdx.x / tiles, t = (long)blockIdx.x - c * tiles;
  const long q0 = first + c * BCAST_QPS, q1 = q0 + BCAST_QPS < first + count ? q0 + BCAST_QPS : first + count;
  if (pairs) {
    const long e = 2 * (t * NT + (long)threadIdx.x);
    if (e >= len)
      return;
    BcastPair v;
    v.a = src[e];
    v.b = src[e + 1];
    for (long q = q0; q < q1; ++q)
      *reinterpret_cast<BcastPair*>(dst + q * len + e) = v;
  } else {
    const long e = t * NT + (long)threadIdx.x;
    if (e >= len)
      return;
    const double v = src[e];
    for (long q = q0; q < q1; ++q)
      dst[q * len + e] = v;
  }
}

// Workgroup t + tiles * c: element tile t of chunk c of `chunk` consecutive QPs (the last one may be short); lane =
// element, so every read is a coalesced row.  out: [chunks][len].
template<int NT>
__device__ __forceinline__ void
sum_body(const double* __restrict__ src, double* __restrict__ out, long len, long first, long count, long chunk, long tiles)
{
  const long c = (long)blockIdx.x / tiles, t = (long)blockIdx.x - c * tiles;
  const long e = t * NT + (long)threadIdx.x;
  if (e >= len)
    return;
  const long q0 = first + c * chunk, q1 = q0 + chunk < first + count ? q0 + chunk : first + count;
  double acc = src[q0 * len + e];
  for (long q = q0 + 1; q < q1; ++q)
    acc += src[q * len + e];
  out[c * len + e] = acc;
}

#endif // PQP_SHARED_DEVICE

} // namespace pqp

#endif
