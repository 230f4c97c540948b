// The kernels of libproxqp_hip.so and their launchers.  Compiled once per kernel family (-DPQP_TU=k for every k of
// KERNEL_TUS in proxsuite_amd/_build.py, the objects built in parallel); PQP_TU undefined or 0 compiles everything in
// one translation unit (the CPU emulator build of tests/emu does that).
//   1  pqp_solve_kernel<256, 4, 1>    no box constraints, dense Hessian (the C2 kernel): 128 VGPRs per
//                                     lane, FOUR workgroups per CU -- launches that fill the device
//   7  pqp_solve_kernel<256, 3, 1>    the same solve with 168 VGPRs per lane, three workgroups per CU:
//                                     lower latency per QP, used when the launch leaves CUs idle anyway
//  15  pqp_solve_kernel<256, 2, 1>    ... 256 VGPRs, launches of at most two workgroups per CU
//  13  pqp_solve_kernel<256, 1, 1>    ... the whole register file, launches of at most one workgroup per CU
//   2  pqp_solve_kernel<256, 3, 0>    the general kernel: boxes, sparse Hessian types, PrimalLDLT
//  14  pqp_solve_kernel<256, 1, 0>    ... launches of at most one workgroup per CU
//   3  pqp_solve_kernel<512, 2, .>    256 VGPRs, one workgroup per CU
//   8  pqp_solve_kernel<512, 4, .>    128 VGPRs, two workgroups per CU: launches of more workgroups than CUs
//   4  pqp_solve_kernel<1024, 4, .>
//   5  pqp_backward_kernel<.>
//   6  pqp_setup_kernel<.>, pqp_order_kernel, pqp_pack_kernel and the host side of a solve launch:
//      pqp_plan_solve (which kernel) and pqp_launch_solve (order, events, enqueue)
#ifndef PQP_TU
#define PQP_TU 0
#endif
//  12  pqp_solve_kernel<256, 2, 2>    the diagonal-structure solver alone (H diagonal / zero, no equality, every inequality
//                                     row on one variable: BASELINE.json configs[4]): launches whose QPs ALL have it
//  16  pqp_diag_kernel<E, 2>          that solver as one wavefront per QP (pqp_diag.hpp), E = 1, 2, 4 register slots per vector
//   9  pqp_solve_hbm_kernel<1024, 4, .>  shapes whose per-QP vectors exceed the CU's 160 KiB of LDS: the
//                                     SAME solver with its "LDS" pointers typed as global memory and
//                                     carved out of a per-workgroup slice of an HBM scratch buffer (the
//                                     workgroup barrier orders global accesses within a workgroup as it
//                                     does LDS ones).  Slow per QP -- every vector access is an L1/L2 round
//                                     trip -- but it removes the size ceiling below 1024 rows.
#if PQP_TU == 9 || PQP_TU == 21 || PQP_TU == 24 || PQP_TU == 27
#define PQP_VECTORS_IN_HBM 1
#define PQP_LDS __attribute__((address_space(1)))
#define PQP_GLOBAL __attribute__((address_space(1)))
#endif
// 8 instead of 16 matrix loads in flight per lane in gemv for the 128-VGPR kernel (pqp_block.hpp)
#if PQP_TU == 1 && !defined(PQP_GEMV_DEEP_256)
#define PQP_GEMV_DEEP_256 0
#endif
// the translation units whose kernels run at 128 VGPRs per lane keep 4 instead of 8 MFMA k-steps of
// operand loads in flight in the Z / G build (+2 % at C2 and C4, profiles/r02_ab_compiler_flags.txt)
#if (PQP_TU == 1 || PQP_TU == 4 || PQP_TU == 8 || PQP_TU == 9 || PQP_TU == 21 || PQP_TU == 24 || PQP_TU == 27) && !defined(PQP_ZG_DEPTH)
#define PQP_ZG_DEPTH 4
#endif
// (the one-wavefront diagonal kernel is not short of scalar registers: its per-QP pointers are ordinary values -- the
// optimisation barriers that keep them from being hoisted in the workgroup kernels would pin them to SGPRs inside
// lane-divergent code here)
#if PQP_TU == 16 || PQP_TU == 17
#define PQP_OPAQUE_SCALAR(v)
#define PQP_OPAQUE_VECTOR(v)
#endif
//  17  pqp_dwave_kernel<WPS>          the DENSE solver as one wavefront per QP (pqp_dwave.hpp): dense Hessian, no box, n, n_eq,
//                                     n_in <= 128 -- the iteration of a solve; launches that fill the device
//  18  pqp_prologue_kernel<256>       the factorisation prologue of those solves (Solver::prologue), 256 threads per QP
//  19  pqp_eig_kernel<256, M>         batched minimal-eigenvalue estimates (pqp_eig.hpp), one workgroup per matrix: M = 0 the
//                                     reference's power iteration, 1 Householder tridiagonalisation + Sturm multisection
//  20  pqp_backward_multi_kernel<.>  the backward pass for K loss derivatives per QP (Solver::backward_multi): one
//                                     factorisation, K refined KKT solves; and pqp_backward_outer_kernel, which forms the
//                                     seven jacobians of pqp_batch_get_backward from one row of its output
//  21  pqp_backward_multi_hbm_kernel<1024>  the same on a slice of the HBM scratch buffer per workgroup (as 9): the
//                                     backward pass of the shapes whose per-QP vectors exceed the LDS
//  22  pqp_infeas_kkt_kernel<256>     the backward pass of the closest-feasible QPLayer (pqp_infeas.hpp): the linear system of
//                                     every QP of a pass, written into the model arrays of the inner handle that solves it;
//                                     and pqp_infeas_grad_kernel<256>, the seven jacobians from the inner solution
//  23  pqp_bwbox_kernel<.>          the backward pass of QPs WITH box constraints (Solver::backward_box): the constraint list
//                                     is [C; I], K loss derivatives per QP; and pqp_bwbox_outer_kernel, which forms the nine
//                                     jacobians (the seven of pqp_batch_get_backward, dL_dl_box, dL_du_box) from one row
//  24  pqp_bwbox_hbm_kernel<1024>     the same on a slice of the HBM scratch buffer per workgroup (as 9 and 21)
//  25  pqp_broadcast_kernel<256>     batches that share a model (pqp_shared.hpp): one model array written to every QP of a range
//                                     (pqp_batch_init_shared / pqp_batch_update_shared), and pqp_sum_kernel<256>, the sum of a
//                                     per-QP array over a range in a fixed order (pqp_batch_get_backward_sum)
//  26  pqp_tangent_multi_kernel<.>   forward-mode sensitivities (pqp_tangent.hpp): K tangents of (x, y, z) per QP on one
//                                     factorisation; and pqp_tangent_rhs_kernel<256>, which forms their right-hand sides
//                                     from the parameter tangents (each tangent matrix read once)
//  27  pqp_tangent_multi_hbm_kernel<1024>  the same on a slice of the HBM scratch buffer per workgroup (as 9, 21 and 24)
#if PQP_TU == 0 || PQP_TU == 22
#define PQP_INFEAS_DEVICE 1 // (pqp_host.hpp includes pqp_infeas.hpp for the launchers' argument record: the kernels' bodies with it here)
#endif
#include "pqp_host.hpp"
#include "pqp_dwave.hpp"
#if PQP_TU == 0 || PQP_TU == 19
#define PQP_EIG_DEVICE 1
#include "pqp_eig.hpp"
#endif

#if PQP_TU == 0 || PQP_TU == 25
#define PQP_SHARED_DEVICE 1
#include "pqp_shared.hpp"
#endif

#if PQP_TU == 0 || PQP_TU == 26 || PQP_TU == 27
#define PQP_TANGENT_DEVICE 1
#include "pqp_tangent.hpp"
#endif

#define PQP_TU_HAS(k) (PQP_TU == 0 || PQP_TU == (k))

// Waves per SIMD the register allocator must leave room for (512 / WPS VGPRs per lane): the
// knob that trades spills against resident workgroups per CU.  Compile-time only.
#ifndef PQP_WPS_256_DENSE
#define PQP_WPS_256_DENSE 4 // throughput variant of the C2 kernel (LDS: 4 x 40.9 KB fits the CU's 160 KB)
#endif
#ifndef PQP_WPS_256
#define PQP_WPS_256 3
#endif
#ifndef PQP_WPS_512
#define PQP_WPS_512 2
#endif
#ifndef PQP_WPS_512_DENSE
#define PQP_WPS_512_DENSE 4
#endif
#ifndef PQP_WPS_1024
#define PQP_WPS_1024 4
#endif

template<int NT, int WPS, int SPEC>
__global__ __launch_bounds__(NT, WPS) void
pqp_solve_kernel(pqp::Batch batch, long first, const int* __restrict__ order)
{
  HIP_DYNAMIC_SHARED(double, smem)
  // `order` (optional) is the dispatch order of the QPs: workgroups are handed out in blockIdx
  // order, so listing the expensive QPs first shortens the tail of the launch
  const long slot = order ? (long)order[blockIdx.x] : (long)blockIdx.x;
  pqp::solve_body<NT, SPEC>(batch, first + slot, (pqp::lptr)smem);
}

// "name<A,...>": a kernel as the build's kernel-resource record (build/obj/*/kernel_resources.json) spells it, from
// the template arguments that ARE instantiated (a variant library built with another PQP_WPS_* says so)
template<int... A>
static std::string
kernel_label(const char* name)
{
  std::string s = std::string(name) + "<";
  ((s += std::to_string(A) + ","), ...);
  s.back() = '>';
  return s;
}

// What every entry below does with its instantiation.  prepare: raise the kernel's dynamic-LDS limit where the launch
// needs more than the default 64 KiB (pqp_launch_solve does this before it starts the clock).  Otherwise: enqueue it
// over the QPs of the launch, workgroup i on QP range_first + (order ? order[i] : i), and note it as the handle's last
// kernel.  `extra`: kernel arguments behind (batch, first, order).
template<class K, class... Extra>
static int
enqueue(K* kernel, const std::string& label, pqp_batch* h, int threads, size_t lds, const int* order, bool prepare,
        Extra... extra)
{
  if (prepare) {
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return PQP_OK;
  }
  hipLaunchKernelGGL((kernel), dim3((unsigned)h->range_count), dim3(threads), lds, h->stream, h->dev, h->range_first,
                     order, extra...);
  HIP_TRY(hipGetLastError());
  h->last_kernel = label.c_str();
  return PQP_OK;
}

template<int NT, int WPS, int SPEC>
static int
enqueue_solve(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  static const std::string label = kernel_label<NT, WPS, SPEC>("pqp_solve_kernel");
  return enqueue(&pqp_solve_kernel<NT, WPS, SPEC>, label, h, NT, p.lds, order, prepare);
}

// One entry per translation unit, all of one signature: enqueue (or prepare) the instantiation the plan names.  An entry
// is named after the PRODUCT's instantiation; a variant library may compile another register budget into it.
using pqp_enqueue = int(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare);
pqp_enqueue pqp_enqueue_256_4_1, pqp_enqueue_256_3_1, pqp_enqueue_256_2_1, pqp_enqueue_256_1_1, pqp_enqueue_256_3_0,
  pqp_enqueue_256_1_0, pqp_enqueue_256_2_2, pqp_enqueue_diag_wave, pqp_enqueue_dense_wave, pqp_enqueue_prologue,
  pqp_enqueue_512_2, pqp_enqueue_512_4, pqp_enqueue_1024, pqp_enqueue_hbm;
#define PQP_SOLVE_ENTRY(name, NT, WPS, SPEC)                                                        \
  int name(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare) { return enqueue_solve<NT, WPS, SPEC>(h, p, order, prepare); }
#define PQP_SOLVE_ENTRY_1_0(name, NT, WPS, K_SPEC_1) /* both SPEC 1 (the plan's kernel is K_SPEC_1) and SPEC 0 */ \
  int name(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)                       \
  {                                                                                                 \
    return p.kernel == K_SPEC_1 ? enqueue_solve<NT, WPS, 1>(h, p, order, prepare) : enqueue_solve<NT, WPS, 0>(h, p, order, prepare); \
  }

#if PQP_TU_HAS(1)
PQP_SOLVE_ENTRY(pqp_enqueue_256_4_1, 256, PQP_WPS_256_DENSE, 1)
#endif
#if PQP_TU_HAS(7)
PQP_SOLVE_ENTRY(pqp_enqueue_256_3_1, 256, PQP_WPS_256, 1)
#endif
// One workgroup per CU: a launch of no more workgroups than the device has CUs (C1: 128 QPs, a single QP::solve())
// leaves every QP a CU of its own, so the whole register file of a SIMD may go to its wavefront -- no spills at all
// (100 spilled VGPRs at three per CU).  C1: 1.318 -> 1.245 ms (profiles/r04_ab_small_launch_budget.txt).
#if PQP_TU_HAS(13)
PQP_SOLVE_ENTRY(pqp_enqueue_256_1_1, 256, 1, 1)
#endif
#if PQP_TU_HAS(15)
PQP_SOLVE_ENTRY(pqp_enqueue_256_2_1, 256, 2, 1) // (up to two workgroups per CU: 256 VGPRs; 384 / 512 QPs of the C2 shape -3 %)
#endif
#if PQP_TU_HAS(14)
PQP_SOLVE_ENTRY(pqp_enqueue_256_1_0, 256, 1, 0) // (one workgroup per CU for the general kernel: boxes, sparse Hessian types, PrimalLDLT)
#endif
#if PQP_TU_HAS(2)
PQP_SOLVE_ENTRY(pqp_enqueue_256_3_0, 256, PQP_WPS_256, 0)
#endif
#ifndef PQP_WPS_256_DIAG
#define PQP_WPS_256_DIAG 2 // (two workgroups per CU at 256 VGPRs: 4.08 ms per 4096 C5 QPs against 4.29 ms with three at 168, profiles/r04_ab_diag_kernel.txt)
#endif
#if PQP_TU_HAS(12)
PQP_SOLVE_ENTRY(pqp_enqueue_256_2_2, 256, PQP_WPS_256_DIAG, 2)
#endif
// One WAVEFRONT per QP, every per-QP vector in registers: the diagonal-structure solver of pqp_diag.hpp
// (BASELINE.json configs[4]).  A workgroup is one wavefront; E = 4 register slots per vector serve dim <= 256, the
// range of the 256-thread kernel class.
#if PQP_TU_HAS(16)
#ifndef PQP_WPS_DIAG_WAVE
#define PQP_WPS_DIAG_WAVE 2
#endif
template<int E, int WPS>
__global__ __launch_bounds__(64, WPS) void
pqp_diag_kernel(pqp::Batch batch, long first, const int* __restrict__ order)
{
  HIP_DYNAMIC_SHARED(double, smem)
  const long slot = order ? (long)order[blockIdx.x] : (long)blockIdx.x;
  pqp::diag_solve_body<E>(batch, first + slot, (pqp::lptr)smem);
}

template<int E>
static int
enqueue_diag(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  static const std::string label = kernel_label<E, PQP_WPS_DIAG_WAVE>("pqp_diag_kernel");
  return enqueue(&pqp_diag_kernel<E, PQP_WPS_DIAG_WAVE>, label, h, 64, p.lds, order, prepare);
}

int
pqp_enqueue_diag_wave(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  switch (p.kernel) {
    case PQP_K_DIAG_1:
      return enqueue_diag<1>(h, p, order, prepare);
    case PQP_K_DIAG_2:
      return enqueue_diag<2>(h, p, order, prepare);
    default:
      return enqueue_diag<4>(h, p, order, prepare);
  }
}
#endif
// One WAVEFRONT per QP for DENSE QPs (pqp_dwave.hpp) behind the 256-thread factorisation prologue: two launches on the
// handle's stream, one pair of events around both and a third between them (pqp_launch_solve).
// (Cutting the launch into 2 - 8 chunks on streams of their own, so that a chunk's prologue runs beside the iteration
// kernel of the chunk before it, changes nothing: 7.67 - 7.93 ms against 7.69 ms per 2048 C2 QPs,
// profiles/r06_ab_dwave.txt -- the pair is bound by the bytes it moves, not by the order it moves them in.)
#if PQP_TU_HAS(18)
template<int NT>
__global__ __launch_bounds__(NT, 4) void
pqp_prologue_kernel(pqp::Batch batch, long first, const int* __restrict__ order)
{
  HIP_DYNAMIC_SHARED(double, smem)
  const long slot = order ? (long)order[blockIdx.x] : (long)blockIdx.x;
  pqp::Solver<NT, 1> S(batch, first + slot, (pqp::lptr)smem);
  S.prologue();
}

int
pqp_enqueue_prologue(pqp_batch* h, const LaunchPlan&, const int* order, bool prepare)
{
  // (the plan's LDS is the iteration kernel's; the prologue is the 256-thread solver's and carves that layout)
  static const std::string label = kernel_label<256>("pqp_prologue_kernel");
  return enqueue(&pqp_prologue_kernel<256>, label, h, 256, h->lds_solve, order, prepare);
}
#endif
#if PQP_TU_HAS(17)
#ifndef PQP_WPS_DENSE_WAVE
#define PQP_WPS_DENSE_WAVE 2
#endif
template<int WPS>
__global__ __launch_bounds__(64, WPS) void
pqp_dwave_kernel(pqp::Batch batch, long first, const int* __restrict__ order)
{
  HIP_DYNAMIC_SHARED(double, smem)
  const long slot = order ? (long)order[blockIdx.x] : (long)blockIdx.x;
  pqp::dwave_solve_body(batch, first + slot, (pqp::lptr)smem);
}

int
pqp_enqueue_dense_wave(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  static const std::string label = kernel_label<PQP_WPS_DENSE_WAVE>("pqp_dwave_kernel");
  return enqueue(&pqp_dwave_kernel<PQP_WPS_DENSE_WAVE>, label, h, 64, p.lds, order, prepare);
}
#endif
#if PQP_TU_HAS(3)
PQP_SOLVE_ENTRY_1_0(pqp_enqueue_512_2, 512, PQP_WPS_512, PQP_K_512_2_1)
#endif
#if PQP_TU_HAS(8)
PQP_SOLVE_ENTRY_1_0(pqp_enqueue_512_4, 512, PQP_WPS_512_DENSE, PQP_K_512_4_1)
#endif
#if PQP_TU_HAS(4)
PQP_SOLVE_ENTRY_1_0(pqp_enqueue_1024, 1024, PQP_WPS_1024, PQP_K_1024_1)
#endif

#if PQP_TU == 9 || (PQP_TU == 0 && defined(PQP_EMULATED_MFMA))
// (the single-translation-unit build exists for the CPU emulator only, where address spaces are plain
// pointers: there the kernel below is the ordinary solver running on a heap slice)
template<int NT, int WPS, int SPEC>
__global__ __launch_bounds__(NT, WPS) void
pqp_solve_hbm_kernel(pqp::Batch batch, long first, const int* __restrict__ order, double* scratch, long stride)
{
  const long slot = order ? (long)order[blockIdx.x] : (long)blockIdx.x;
  pqp::solve_body<NT, SPEC>(batch, first + slot, (pqp::lptr)(scratch + (long)blockIdx.x * stride));
}

template<int SPEC>
static int
enqueue_hbm(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  // (no dynamic LDS: workgroup i works on the i-th slice of p.lds bytes of the scratch buffer)
  static const std::string label = kernel_label<1024, PQP_WPS_1024, SPEC>("pqp_solve_hbm_kernel");
  return enqueue(&pqp_solve_hbm_kernel<1024, PQP_WPS_1024, SPEC>, label, h, 1024, 0, order, prepare, h->vec_scratch,
                 (long)((p.lds + 7) / 8));
}

int
pqp_enqueue_hbm(pqp_batch* h, const LaunchPlan& p, const int* order, bool prepare)
{
  return p.kernel == PQP_K_HBM_1 ? enqueue_hbm<1>(h, p, order, prepare) : enqueue_hbm<0>(h, p, order, prepare);
}
#endif

#if PQP_TU_HAS(19)
template<int NT, int METHOD>
__global__ __launch_bounds__(NT) void
pqp_eig_kernel(pqp::EigArgs a)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::eig_body<NT, METHOD>(a, (long)blockIdx.x, (pqp::lptr)smem);
}

template<int METHOD>
static int
launch_eig(const pqp::EigArgs& a, long count, hipStream_t stream)
{
  const size_t lds = pqp::eig_lds_bytes(a.n, a.resident != 0);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_eig_kernel<pqp::EIG_NT, METHOD>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pqp_eig_kernel<pqp::EIG_NT, METHOD>), dim3((unsigned)count), dim3(pqp::EIG_NT), lds, stream, a);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_eig(const pqp::EigArgs& a, long count, hipStream_t stream)
{
  return a.method == PQP_EIG_POWER_ITERATION ? launch_eig<PQP_EIG_POWER_ITERATION>(a, count, stream)
                                             : launch_eig<PQP_EIG_EXACT_METHOD>(a, count, stream);
}
#endif

#if PQP_TU_HAS(5)
template<int NT>
__global__ __launch_bounds__(NT, 2) void
pqp_backward_kernel(pqp::Batch batch, pqp::BackwardArgs bw)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::backward_body<NT>(batch, bw, (long)blockIdx.x, (pqp::lptr)smem);
}

template<int NT>
static int
launch_backward(pqp_batch* h, const pqp::BackwardArgs& bw, long count)
{
  if (h->lds_solve > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_backward_kernel<NT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_solve));
  hipLaunchKernelGGL((pqp_backward_kernel<NT>), dim3((unsigned)count), dim3(NT), h->lds_solve, h->stream,
                     h->dev, bw);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_backward(pqp_batch* h, const pqp::BackwardArgs& bw, long count)
{
  switch (h->nt) {
    case 256:
      return launch_backward<256>(h, bw, count);
    case 512:
      return launch_backward<512>(h, bw, count);
    default:
      return launch_backward<1024>(h, bw, count);
  }
}
#endif

#if PQP_TU_HAS(20)
template<int NT>
__global__ __launch_bounds__(NT, 2) void
pqp_backward_multi_kernel(pqp::Batch batch, pqp::BackwardMultiArgs bw)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::backward_multi_body<NT>(batch, bw, (long)blockIdx.x, (pqp::lptr)smem);
}

template<int NT>
static int
launch_backward_multi(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  if (h->lds_solve > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_backward_multi_kernel<NT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_solve));
  hipLaunchKernelGGL((pqp_backward_multi_kernel<NT>), dim3((unsigned)count), dim3(NT), h->lds_solve, h->stream,
                     h->dev, bw);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_backward_multi(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  switch (h->nt) {
    case 256:
      return launch_backward_multi<256>(h, bw, count);
    case 512:
      return launch_backward_multi<512>(h, bw, count);
    default:
      return launch_backward_multi<1024>(h, bw, count);
  }
}

// The seven jacobians of compute_backward_loss_ESG (the expressions at the end of Solver::backward) of the QPs of one
// backward_multi launch with n_rhs = 1, element-wise: workgroup i * shares + j takes the j-th share of the entries of the QP
// of slot i.  v: [count][n + n_eq + n_in] rows (dx_u, dy_u, dz_u); active: [count][n_in] flags; outputs over the whole batch.
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_backward_outer_kernel(pqp::Batch batch, pqp::BackwardArgs bw, const double* __restrict__ v,
                          const int* __restrict__ active, int shares)
{
  const long n = batch.d.n, ne = batch.d.n_eq, ni = batch.d.n_in;
  const long slot = blockIdx.x / shares, share = blockIdx.x - slot * shares;
  const long q = bw.order ? (long)bw.order[slot] : bw.first + slot;
  const double *dxu = v + slot * (n + ne + ni), *dyu = dxu + n, *dzu = dyu + ne;
  const int* fl = active + slot * ni;
  const double *xs = batch.x + q * n, *ys = batch.y + q * ne, *zs = batch.z + q * batch.d.nc;
  double *oH = bw.dL_dH + q * n * n, *og = bw.dL_dg + q * n, *oA = bw.dL_dA + q * ne * n, *ob = bw.dL_db + q * ne;
  double *oC = bw.dL_dC + q * ni * n, *ou = bw.dL_du + q * ni, *ol = bw.dL_dl + q * ni;
  const long t0 = share * NT + threadIdx.x, step = (long)shares * NT;
  for (long o = t0; o < n * n; o += step) {
    const long i = o / n, k = o - i * n;
    oH[o] = 0.5 * (dxu[i] * xs[k] + xs[i] * dxu[k]);
  }
  for (long k = t0; k < n; k += step)
    og[k] = dxu[k];
  for (long o = t0; o < ne * n; o += step) {
    const long i = o / n, k = o - i * n;
    oA[o] = dyu[i] * xs[k] + ys[i] * dxu[k];
  }
  for (long k = t0; k < ne; k += step)
    ob[k] = -dyu[k];
  for (long o = t0; o < ni * n; o += step) {
    const long i = o / n, k = o - i * n;
    oC[o] = dzu[i] * xs[k] + zs[i] * dxu[k];
  }
  for (long i = t0; i < ni; i += step) {
    ou[i] = (fl[i] & 1) ? -dzu[i] : 0.0;
    ol[i] = (fl[i] & 2) ? -dzu[i] : 0.0;
  }
}

int
pqp_launch_backward_outer(pqp_batch* h, const pqp::BackwardArgs& bw, const double* v, const int* active, long count)
{
  const long n = h->dev.d.n, rows = std::max<long>(n, std::max<long>(h->dev.d.n_eq, h->dev.d.n_in));
  const long shares = std::min<long>(64, std::max<long>(1, (rows * n + 255) / 256));
  hipLaunchKernelGGL((pqp_backward_outer_kernel<256>), dim3((unsigned)(count * shares)), dim3(256), 0, h->stream, h->dev, bw, v,
                     active, (int)shares);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU == 21 || (PQP_TU == 0 && defined(PQP_EMULATED_MFMA))
// (as pqp_solve_hbm_kernel: workgroup i works on the i-th slice of the handle's scratch buffer; no dynamic LDS)
template<int NT>
__global__ __launch_bounds__(NT, PQP_WPS_1024) void
pqp_backward_multi_hbm_kernel(pqp::Batch batch, pqp::BackwardMultiArgs bw, double* scratch, long stride)
{
  pqp::backward_multi_body<NT>(batch, bw, (long)blockIdx.x, (pqp::lptr)(scratch + (long)blockIdx.x * stride));
}

int
pqp_launch_backward_multi_hbm(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  hipLaunchKernelGGL((pqp_backward_multi_hbm_kernel<1024>), dim3((unsigned)count), dim3(1024), 0, h->stream, h->dev, bw,
                     h->vec_scratch, (long)((h->lds_solve + 7) / 8));
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU_HAS(23)
template<int NT>
__global__ __launch_bounds__(NT, 2) void
pqp_bwbox_kernel(pqp::Batch batch, pqp::BackwardMultiArgs bw)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::backward_box_body<NT>(batch, bw, (long)blockIdx.x, (pqp::lptr)smem);
}

template<int NT>
static int
launch_bwbox(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  if (h->lds_solve > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_bwbox_kernel<NT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_solve));
  hipLaunchKernelGGL((pqp_bwbox_kernel<NT>), dim3((unsigned)count), dim3(NT), h->lds_solve, h->stream, h->dev, bw);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_bwbox(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  switch (h->nt) {
    case 256:
      return launch_bwbox<256>(h, bw, count);
    case 512:
      return launch_bwbox<512>(h, bw, count);
    default:
      return launch_bwbox<1024>(h, bw, count);
  }
}

// The nine jacobians of a box-constrained QP from one row of a backward_box launch with n_rhs = 1, element-wise and shared
// out as in pqp_backward_outer_kernel.  v: [count][n + n_eq + n_in + n] rows (dx_u, dy_u, dz_in_u, dz_box_u); active:
// [count][n_in + n] flags; outputs over the whole batch.  dL_dC covers the n_in general rows: the identity block of
// [C; I] has no parameter; its rows give dL_du_box / dL_dl_box (length n).
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_bwbox_outer_kernel(pqp::Batch batch, pqp::BackwardArgs bw, double* __restrict__ dL_dlb, double* __restrict__ dL_dub,
                       const double* __restrict__ v, const int* __restrict__ active, int shares)
{
  const long n = batch.d.n, ne = batch.d.n_eq, ni = batch.d.n_in, nc = batch.d.nc;
  const long slot = blockIdx.x / shares, share = blockIdx.x - slot * shares;
  const long q = bw.order ? (long)bw.order[slot] : bw.first + slot;
  const double *dxu = v + slot * (n + ne + nc), *dyu = dxu + n, *dzu = dyu + ne;
  const int* fl = active + slot * nc;
  const double *xs = batch.x + q * n, *ys = batch.y + q * ne, *zs = batch.z + q * nc;
  double *oH = bw.dL_dH + q * n * n, *og = bw.dL_dg + q * n, *oA = bw.dL_dA + q * ne * n, *ob = bw.dL_db + q * ne;
  double *oC = bw.dL_dC + q * ni * n, *ou = bw.dL_du + q * ni, *ol = bw.dL_dl + q * ni;
  double *oub = dL_dub + q * n, *olb = dL_dlb + q * n;
  const long t0 = share * NT + threadIdx.x, step = (long)shares * NT;
  for (long o = t0; o < n * n; o += step) {
    const long i = o / n, k = o - i * n;
    oH[o] = 0.5 * (dxu[i] * xs[k] + xs[i] * dxu[k]);
  }
  for (long k = t0; k < n; k += step)
    og[k] = dxu[k];
  for (long o = t0; o < ne * n; o += step) {
    const long i = o / n, k = o - i * n;
    oA[o] = dyu[i] * xs[k] + ys[i] * dxu[k];
  }
  for (long k = t0; k < ne; k += step)
    ob[k] = -dyu[k];
  for (long o = t0; o < ni * n; o += step) {
    const long i = o / n, k = o - i * n;
    oC[o] = dzu[i] * xs[k] + zs[i] * dxu[k];
  }
  for (long i = t0; i < ni; i += step) {
    ou[i] = (fl[i] & 1) ? -dzu[i] : 0.0;
    ol[i] = (fl[i] & 2) ? -dzu[i] : 0.0;
  }
  for (long k = t0; k < nc - ni; k += step) {
    oub[k] = (fl[ni + k] & 1) ? -dzu[ni + k] : 0.0;
    olb[k] = (fl[ni + k] & 2) ? -dzu[ni + k] : 0.0;
  }
}

int
pqp_launch_bwbox_outer(pqp_batch* h, const pqp::BackwardArgs& bw, double* dL_dlb, double* dL_dub, const double* v,
                       const int* active, long count)
{
  const long n = h->dev.d.n, rows = std::max<long>(n, std::max<long>(h->dev.d.n_eq, h->dev.d.n_in));
  const long shares = std::min<long>(64, std::max<long>(1, (rows * n + 255) / 256));
  hipLaunchKernelGGL((pqp_bwbox_outer_kernel<256>), dim3((unsigned)(count * shares)), dim3(256), 0, h->stream, h->dev, bw,
                     dL_dlb, dL_dub, v, active, (int)shares);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU == 24 || (PQP_TU == 0 && defined(PQP_EMULATED_MFMA))
// (as pqp_backward_multi_hbm_kernel: workgroup i works on the i-th slice of the handle's scratch buffer; no dynamic LDS)
template<int NT>
__global__ __launch_bounds__(NT, PQP_WPS_1024) void
pqp_bwbox_hbm_kernel(pqp::Batch batch, pqp::BackwardMultiArgs bw, double* scratch, long stride)
{
  pqp::backward_box_body<NT>(batch, bw, (long)blockIdx.x, (pqp::lptr)(scratch + (long)blockIdx.x * stride));
}

int
pqp_launch_bwbox_hbm(pqp_batch* h, const pqp::BackwardMultiArgs& bw, long count)
{
  hipLaunchKernelGGL((pqp_bwbox_hbm_kernel<1024>), dim3((unsigned)count), dim3(1024), 0, h->stream, h->dev, bw,
                     h->vec_scratch, (long)((h->lds_solve + 7) / 8));
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU_HAS(26)
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_tangent_rhs_kernel(pqp::Batch batch, pqp::TangentRhsArgs a)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::tangent_rhs_body<NT>(batch, a, smem);
}

// R[slot][k][:] of every QP of the launch and every direction: workgroup slot * n_dir + k
int
pqp_launch_tangent_rhs(pqp_batch* h, const pqp::TangentRhsArgs& a, long count)
{
  const size_t lds = pqp::tangent_rhs_lds_bytes(h->dev.d.n, h->dev.d.n_eq, h->dev.d.n_in, 256);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_tangent_rhs_kernel<256>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pqp_tangent_rhs_kernel<256>), dim3((unsigned)(count * a.n_dir)), dim3(256), lds, h->stream, h->dev, a);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

template<int NT>
__global__ __launch_bounds__(NT, 2) void
pqp_tangent_multi_kernel(pqp::Batch batch, pqp::TangentArgs tg)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::tangent_multi_body<NT>(batch, tg, (long)blockIdx.x, (pqp::lptr)smem);
}

template<int NT>
static int
launch_tangent_multi(pqp_batch* h, const pqp::TangentArgs& tg, long count)
{
  if (h->lds_solve > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_tangent_multi_kernel<NT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_solve));
  hipLaunchKernelGGL((pqp_tangent_multi_kernel<NT>), dim3((unsigned)count), dim3(NT), h->lds_solve, h->stream, h->dev, tg);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_tangent_multi(pqp_batch* h, const pqp::TangentArgs& tg, long count)
{
  switch (h->nt) {
    case 256:
      return launch_tangent_multi<256>(h, tg, count);
    case 512:
      return launch_tangent_multi<512>(h, tg, count);
    default:
      return launch_tangent_multi<1024>(h, tg, count);
  }
}
#endif

#if PQP_TU == 27 || (PQP_TU == 0 && defined(PQP_EMULATED_MFMA))
// (as pqp_backward_multi_hbm_kernel: workgroup i works on the i-th slice of the handle's scratch buffer; no dynamic LDS)
template<int NT>
__global__ __launch_bounds__(NT, PQP_WPS_1024) void
pqp_tangent_multi_hbm_kernel(pqp::Batch batch, pqp::TangentArgs tg, double* scratch, long stride)
{
  pqp::tangent_multi_body<NT>(batch, tg, (long)blockIdx.x, (pqp::lptr)(scratch + (long)blockIdx.x * stride));
}

int
pqp_launch_tangent_multi_hbm(pqp_batch* h, const pqp::TangentArgs& tg, long count)
{
  hipLaunchKernelGGL((pqp_tangent_multi_hbm_kernel<1024>), dim3((unsigned)count), dim3(1024), 0, h->stream, h->dev, tg,
                     h->vec_scratch, (long)((h->lds_solve + 7) / 8));
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU_HAS(22)
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_infeas_kkt_kernel(pqp::Batch batch, pqp::InfeasArgs a)
{
  pqp::infeas_kkt_body<NT>(batch, a);
}

template<int NT>
__global__ __launch_bounds__(NT) void
pqp_infeas_grad_kernel(pqp::Batch batch, pqp::InfeasArgs a, pqp::BackwardArgs bw)
{
  pqp::infeas_grad_body<NT>(batch, a, bw);
}

// (a.shares is set here: row tiles of K per slot, spread until the launch has a few workgroups per CU)
int
pqp_launch_infeas_kkt(pqp_batch* h, pqp::InfeasArgs a)
{
  const pqp::Dims& d = h->dev.d;
  const long tiles = (pqp::infeas_rows(d.n, d.n_eq, d.n_in) + pqp::INFEAS_TILE - 1) / pqp::INFEAS_TILE;
  a.shares = (int)std::min<long>(tiles, std::max<long>(1, (4L * h->n_cu + a.count - 1) / a.count));
  hipLaunchKernelGGL((pqp_infeas_kkt_kernel<256>), dim3((unsigned)(a.count * a.shares)), dim3(256), 0, h->stream, h->dev, a);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_infeas_grad(pqp_batch* h, pqp::InfeasArgs a, const pqp::BackwardArgs& bw)
{
  const long n = h->dev.d.n, rows = std::max<long>(n, std::max<long>(h->dev.d.n_eq, h->dev.d.n_in));
  a.shares = (int)std::min<long>(64, std::max<long>(1, (rows * n + 255) / 256));
  hipLaunchKernelGGL((pqp_infeas_grad_kernel<256>), dim3((unsigned)(a.count * a.shares)), dim3(256), 0, h->stream, h->dev, a, bw);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU_HAS(25)
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_broadcast_kernel(const double* __restrict__ src, double* __restrict__ dst, long len, long first, long count, long tiles,
                     int pairs)
{
  pqp::broadcast_body<NT>(src, dst, len, first, count, tiles, pairs != 0);
}

template<int NT>
__global__ __launch_bounds__(NT) void
pqp_sum_kernel(const double* __restrict__ src, double* __restrict__ out, long len, long first, long count, long chunk,
               long tiles)
{
  pqp::sum_body<NT>(src, out, len, first, count, chunk, tiles);
}

// src (device memory, `len` doubles) -> dst + q * len for q in [first, first + count), on the handle's stream
int
pqp_launch_broadcast(pqp_batch* h, const double* src, double* dst, long len, long first, long count)
{
  if (len <= 0 || count <= 0)
    return PQP_OK;
  const int pairs = len % 2 == 0;
  const long per_tile = pairs ? 2 * 256 : 256;
  const long tiles = (len + per_tile - 1) / per_tile, chunks = (count + pqp::BCAST_QPS - 1) / pqp::BCAST_QPS;
  hipLaunchKernelGGL((pqp_broadcast_kernel<256>), dim3((unsigned)(tiles * chunks)), dim3(256), 0, h->stream, src, dst, len,
                     first, count, tiles, pairs);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

// out[c * len + e] = sum of src[q * len + e] over the c-th chunk of `chunk` QPs of [first, first + count), sequentially in
// index order, on the handle's stream
int
pqp_launch_sum(pqp_batch* h, const double* src, double* out, long len, long first, long count, long chunk)
{
  if (len <= 0 || count <= 0)
    return PQP_OK;
  const long tiles = (len + 255) / 256, chunks = (count + chunk - 1) / chunk;
  hipLaunchKernelGGL((pqp_sum_kernel<256>), dim3((unsigned)(tiles * chunks)), dim3(256), 0, h->stream, src, out, len, first,
                     count, chunk, tiles);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}
#endif

#if PQP_TU_HAS(6)
template<int NT>
__global__ __launch_bounds__(NT) void
pqp_setup_kernel(pqp::Batch batch, long first)
{
  HIP_DYNAMIC_SHARED(double, smem)
  pqp::setup_body<NT>(batch, first + (long)blockIdx.x, (pqp::lptr)smem);
}

// Dispatch order for the next whole-batch launch: QP i goes to position
// rank(i) = #{ j : cycles_j > cycles_i  or  (cycles_j == cycles_i and j < i) }  (descending by the
// device cycles of the solve that just finished; O(B^2) compares, a few microseconds for B ~ 10^3-10^4).
__global__ __launch_bounds__(64) void
pqp_order_kernel(const long long* __restrict__ stats, int stride, int B, int* __restrict__ order)
{
  // keys are compared as 32-bit values (cycle counts are clamped to 2^32 - 1: an ordering
  // heuristic, exactness of huge counts does not matter)
  constexpr int TILE = 4096;
  __shared__ unsigned tile[TILE];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const long long raw = (i < B) ? stats[(long)i * stride] : 0;
  const unsigned ci = raw > 0xffffffffll ? 0xffffffffu : (raw < 0 ? 0u : (unsigned)raw);
  int rank = 0;
  for (int j0 = 0; j0 < B; j0 += TILE) {
    const int cnt = (B - j0 < TILE) ? (B - j0) : TILE;
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
      const long long r = stats[(long)(j0 + t) * stride];
      tile[t] = r > 0xffffffffll ? 0xffffffffu : (r < 0 ? 0u : (unsigned)r);
    }
    __syncthreads();
    const int split = (i - j0 < 0) ? 0 : ((i - j0 < cnt) ? (i - j0) : cnt); // j < i  <=>  t < split
    for (int t = 0; t < split; ++t)
      rank += (tile[t] >= ci) ? 1 : 0;
    for (int t = split; t < cnt; ++t)
      rank += (tile[t] > ci) ? 1 : 0;
  }
  if (i < B)
    order[rank] = i;
}

template<int NT>
static int
launch_setup(pqp_batch* h)
{
  if (h->lds_setup > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pqp_setup_kernel<NT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_setup));
  // only the QPs [setup_first, setup_first + setup_count) carry a queued command
  hipLaunchKernelGGL((pqp_setup_kernel<NT>), dim3((unsigned)h->setup_count), dim3(NT), h->lds_setup, h->stream,
                     h->dev, h->setup_first);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

int
pqp_launch_setup(pqp_batch* h)
{
  switch (h->nt) {
    case 256:
      return launch_setup<256>(h);
    case 512:
      return launch_setup<512>(h);
    default:
      return launch_setup<1024>(h);
  }
}

int
pqp_launch_order(pqp_batch* h, long count)
{
  hipLaunchKernelGGL((pqp_order_kernel), dim3((unsigned)((count + 63) / 64)), dim3(64), 0, h->stream,
                     reinterpret_cast<const long long*>(h->dev.stats), (int)pqp::ST_COUNT, (int)count, h->d_order);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

// (x, y, z, status, iter) of the QPs first .. first+count-1 packed into one row-major
// [count][n + n_eq + n_c + 2] fp64 buffer: the payload of the path's only collective (the final
// all_gather of a sharded batch), built on the device so that the gather never touches the host.
__global__ __launch_bounds__(256) void
pqp_pack_kernel(pqp::Batch batch, long first, long count, double* __restrict__ out)
{
  const int n = batch.d.n, ne = batch.d.n_eq, nc = batch.d.nc;
  const long width = (long)n + ne + nc + 2;
  const long total = count * width;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
    const long i = o / width;
    const int k = (int)(o - i * width);
    const long q = first + i;
    double v;
    if (k < n)
      v = batch.x[q * n + k];
    else if (k < n + ne)
      v = batch.y[q * ne + (k - n)];
    else if (k < n + ne + nc)
      v = batch.z[q * nc + (k - n - ne)];
    else if (k == n + ne + nc)
      v = (double)batch.info[q].status;
    else
      v = (double)batch.info[q].iter;
    out[o] = v;
  }
}

int
pqp_launch_pack(pqp_batch* h, long first, long count, double* out, hipStream_t stream)
{
  const long width = (long)h->dev.d.n + h->dev.d.n_eq + h->dev.d.nc + 2;
  long blocks = (count * width + 255) / 256;
  if (blocks > 4096)
    blocks = 4096;
  if (blocks < 1)
    blocks = 1;
  hipLaunchKernelGGL((pqp_pack_kernel), dim3((unsigned)blocks), dim3(256), 0, stream, h->dev, first, count, out);
  HIP_TRY(hipGetLastError());
  return PQP_OK;
}

// Every QP OF THE LAUNCH (its range or its subset) has diagonal structure: the signature, and the flag the set-up kernel
// left for each of them (known once it has run: pqp_batch_flush).  (a general QP or a never-initialised slot
// elsewhere in the handle no longer sends a launch of structured QPs to the 6.5 x slower kernel.)
static bool
diag_structure(const pqp_batch* h, long first, long count, const std::vector<int>* subset)
{
  const pqp::Dims& dd = h->dev.d;
  if (!pqp::diag_structure_signature(dd.hessian, dd.n_eq, dd.n_in, dd.box) || h->c_diag.empty())
    return false;
  if (subset)
    return std::all_of(subset->begin(), subset->end(), [&](int q) { return h->c_diag[size_t(q)] != 0; });
  const size_t hi = std::min(h->c_diag.size(), size_t(first + count));
  return std::all_of(h->c_diag.begin() + std::min(size_t(first), hi), h->c_diag.begin() + hi, [](char c) { return c != 0; });
}

// A launch of `count` dense QPs goes to the one-wavefront kernel (pqp_dwave.hpp) behind the factorisation prologue.
// PQP_DENSE_KERNEL=workgroup / wave forces either (the A/B partners of the tests; read per launch).  By default the
// one-wavefront form takes the launches made of full resident rounds (see below).
static bool
dense_wave(const pqp_batch* h, long count)
{
  if (!pqp::dwave_signature(h->dev.d))
    return false;
  const char* e = std::getenv("PQP_DENSE_KERNEL");
  if (e && e[0] == 'w' && e[1] == 'o') // "workgroup"
    return false;
  if (e && e[0] == 'w' && e[1] == 'a') // "wave"
    return true;
  // Measured on C2-shaped batches, both kernels at 22 batch sizes (profiles/r06_ab_dwave.txt sections 5 and 17): the
  // one-wavefront kernel keeps 8 QPs per CU resident; it wins from 0.6 of a resident round upwards (1280 QPs on 256 CUs: +7 %;
  // 2048: +10 %) and in later rounds whenever the last one is empty or at least 0.4 full (3072: +6 %, 4096: +5 %); a thinner
  // last round is run at a lone wavefront's latency and ties or loses 1 - 2 % (2304, 2560), and below 0.6 of a round the
  // workgroup kernel's four wavefronts per QP win outright (1024 QPs: 4.4 against 5.2 ms).  Five other shapes of the
  // signature behave the same way (section 10).
  const long round = 8L * h->n_cu, rem = count % round;
  if (count < 64) // (whatever the device: a handful of QPs is a latency problem -- and the one-CU emulated device of the CPU tests
    return false; //  dispatches small launches as a real one does)
  if (count < round)
    return 5 * count >= 3 * round;
  return rem == 0 || 5 * rem >= 2 * round;
}

LaunchPlan
pqp_plan_solve(const pqp_batch* h, long first, long count, const std::vector<int>* subset)
{
  const pqp::Dims& dd = h->dev.d;
  // SPEC = 1: no box constraints, dense Hessian, PrimalDualLDLT engine -- all known at compile time
  const bool common = dd.box == 0 && dd.hessian == PQP_HESSIAN_DENSE && dd.backend != PQP_BACKEND_PRIMAL_LDLT;
  const long n_cu = h->n_cu;
  const auto workgroup = [h](pqp_kernel k) { return LaunchPlan{ k, h->nt, h->lds_solve, false }; };
  if (h->vec_scratch) // per-QP vectors beyond the LDS of a CU: the solver runs on an HBM slice per workgroup
    return workgroup(common ? PQP_K_HBM_1 : PQP_K_HBM_0);
  switch (h->nt) {
    case 256:
      if (!common) {
        if (diag_structure(h, first, count, subset)) {
          // PQP_DIAG_KERNEL=workgroup forces the 256-thread form of that solver (its A/B partner in the tests; read per
          // launch: they switch it between two solves)
          const char* e = std::getenv("PQP_DIAG_KERNEL");
          if ((e && e[0] == 'w') || dd.n > 256)
            return workgroup(PQP_K_256_2_2);
          // register slots per vector by dimension: 1 (dim <= 64), 2 (<= 128), 4 (<= 256) -- a slot is a pass of every
          // element-wise loop over all 64 lanes, so a QP of dim 60 does a quarter of the vector instructions of one of dim 200
          const int slots = dd.n <= 64 ? 1 : (dd.n <= 128 ? 2 : 4);
          return LaunchPlan{ slots == 1 ? PQP_K_DIAG_1 : (slots == 2 ? PQP_K_DIAG_2 : PQP_K_DIAG_4), 64,
                             pqp::diag_lds_bytes(slots), false };
        }
        return workgroup(count <= n_cu ? PQP_K_256_1_0 : PQP_K_256_3_0);
      }
      if (dense_wave(h, count))
        return LaunchPlan{ PQP_K_DWAVE, 64, pqp::dwave_lds_bytes(), true };
      // more workgroups than three per CU can hold at once: the four-per-CU build; otherwise the
      // launch is latency-bound and the build with the larger register budget is faster per QP
      if (count > 3 * n_cu && 4 * h->lds_solve <= 160 * 1024)
        return workgroup(PQP_K_256_4_1);
      if (count <= n_cu)
        return workgroup(PQP_K_256_1_1); // a CU per QP: the whole register file
      return workgroup(count <= 2 * n_cu ? PQP_K_256_2_1 : PQP_K_256_3_1);
    case 512:
      // (same rule as for 256 threads: the smaller register budget only when it buys a second resident workgroup)
      if (count > n_cu && 2 * h->lds_solve <= 160 * 1024)
        return workgroup(common ? PQP_K_512_4_1 : PQP_K_512_4_0);
      return workgroup(common ? PQP_K_512_2_1 : PQP_K_512_2_0);
    default:
      return workgroup(common ? PQP_K_1024_1 : PQP_K_1024_0);
  }
}

// the translation-unit entry of every pqp_kernel, in the order of the enum
static pqp_enqueue* const ENTRY_OF[PQP_K_COUNT] = {
  pqp_enqueue_256_4_1, pqp_enqueue_256_3_1, pqp_enqueue_256_2_1, pqp_enqueue_256_1_1, pqp_enqueue_256_3_0, pqp_enqueue_256_1_0,
  pqp_enqueue_256_2_2, pqp_enqueue_diag_wave, pqp_enqueue_diag_wave, pqp_enqueue_diag_wave, pqp_enqueue_dense_wave,
  pqp_enqueue_512_2, pqp_enqueue_512_2, pqp_enqueue_512_4, pqp_enqueue_512_4, pqp_enqueue_1024, pqp_enqueue_1024,
  pqp_enqueue_hbm, pqp_enqueue_hbm
};

// One solve launch, as solve_impl left it in h->range_* / h->subset_*: planned once, then timed and enqueued here and
// nowhere else -- ev0, the kernel(s), ev1, and ev_mid behind the prologue of a two-kernel launch.
int
pqp_launch_solve(pqp_batch* h)
{
  const LaunchPlan p = pqp_plan_solve(h, h->range_first, h->range_count, h->subset_host);
  // PQP_PRIMAL_REUSE=0: every solve factorises its primal block as if State::primal_valid did not exist (the A/B
  // partner of the tests and of the measurements; read per launch, like PQP_DENSE_KERNEL)
  const char* reuse = std::getenv("PQP_PRIMAL_REUSE");
  h->dev.primal_reuse = (reuse && reuse[0] == '0') ? 0 : 1;
  // dispatch order of the QPs (workgroups are handed out in blockIdx order): the subset list, else the learned
  // longest-first order of a whole-batch launch, else none
  const bool whole = h->range_first == 0 && h->range_count == h->dev.B;
  const int* order = h->subset_order ? h->subset_order : ((h->lpt && h->order_valid && whole) ? h->d_order : nullptr);
  h->prologue_timed = false;
  if (p.prologue)
    if (int rc = pqp_enqueue_prologue(h, p, order, true))
      return rc;
  if (int rc = ENTRY_OF[p.kernel](h, p, order, true))
    return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  if (p.prologue) {
    if (int rc = pqp_enqueue_prologue(h, p, order, false))
      return rc;
    HIP_TRY(hipEventRecord(h->ev_mid, h->stream));
    h->prologue_timed = true;
  }
  if (int rc = ENTRY_OF[p.kernel](h, p, order, false))
    return rc;
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  return PQP_OK;
}
#endif
