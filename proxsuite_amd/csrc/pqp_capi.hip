// libproxqp_hip.so -- host side of the C-ABI declared in include/proxqp_hip.h:
// HBM layout of a batch, the host mirror of the reference's settings state machine
// (dense/wrapper.hpp init/update, helpers.hpp:174-189, 678-763) and the launches of
// the two kernels (setup = init/update + Ruiz; solve = qp_solve on every QP).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pqp_host.hpp"
#include "pqp_diag.hpp"
#include "pqp_eig.hpp"
#include "pqp_shared.hpp"
#include "pqp_tangent.hpp"

namespace {

thread_local std::string g_err;

bool
absent(double v)
{
  return std::isnan(v);
}

// reference dense/wrapper.hpp:81-113
int
dense_backend_choice(int backend, int64_t dim, int64_t n_eq, int64_t n_in, bool box)
{
  if (backend != PQP_BACKEND_AUTOMATIC)
    return backend;
  int64_t n_constraints = n_in + (box ? dim : 0);
  double threshold = 1.5, frequence = 0.2, d = double(dim);
  double PrimalDualLDLTCost =
    0.5 * std::pow(double(n_eq) / d, 2) +
    0.17 * (std::pow(double(n_eq) / d, 3) + std::pow(double(n_constraints) / d, 3)) +
    frequence * std::pow(double(n_eq + n_constraints) / d, 2) / d;
  double PrimalLDLTCost = threshold * ((0.5 * double(n_eq) + double(n_constraints)) / d + frequence / d);
  return PrimalDualLDLTCost > PrimalLDLTCost ? PQP_BACKEND_PRIMAL_LDLT : PQP_BACKEND_PRIMAL_DUAL_LDLT;
}

} // namespace

int
pqp_fail(int code, const std::string& msg)
{
  g_err = msg;
  return code;
}

namespace {

template<typename T>
int
dalloc(pqp_batch* h, T** p, size_t count)
{
  void* q = nullptr;
  size_t bytes = (count ? count : 1) * sizeof(T);
  HIP_TRY(hipMalloc(&q, bytes));
  HIP_TRY(hipMemset(q, 0, bytes));
  h->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return PQP_OK;
}

// grow-only device buffer of the handle: at least `count` elements behind *p (its contents are not kept)
template<typename T>
int
grow(pqp_batch* h, T** p, size_t* cap, size_t count)
{
  if (*p && *cap >= count)
    return PQP_OK;
  if (*p) {
    h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), static_cast<void*>(*p)), h->allocs.end());
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
  }
  if (int rc = dalloc(h, p, count))
    return rc;
  *cap = count;
  return PQP_OK;
}

int
upload_settings(pqp_batch* h)
{
  if (!h->settings_dirty)
    return PQP_OK;
  // users write into the host records at any time, so every solve has to look at them; the
  // upload itself is skipped when nothing changed since the last one
  const size_t bytes = h->settings.size() * sizeof(pqp_settings);
  if (h->settings_uploaded.size() == h->settings.size() &&
      std::memcmp(h->settings_uploaded.data(), h->settings.data(), bytes) == 0)
    return PQP_OK;
  HIP_TRY(hipMemcpy(h->d_settings, h->settings.data(), bytes, hipMemcpyHostToDevice));
  h->settings_uploaded = h->settings;
  // the host copy stays "dirty" for ever: users hold raw pointers into it and may
  // write at any time (reference: qp.settings is a public member)
  return PQP_OK;
}

int
check_idx(pqp_batch* h, int64_t idx)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (idx < -1 || idx >= h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
  return PQP_OK;
}

// an asynchronous solve still in flight is waited for before anything else touches the handle
int
settle(pqp_batch* h)
{
  return (h && h->solve_in_flight) ? pqp_batch_wait(h) : PQP_OK;
}

// the device copy of the results of QP idx (-1: all) is about to change outside a solve: its host mirror is stale
void
mirror_stale(pqp_batch* h, int64_t idx)
{
  if (!h->host_results)
    return;
  if (idx < 0)
    std::fill(h->mirror_fresh.begin(), h->mirror_fresh.end(), char(0));
  else
    h->mirror_fresh[size_t(idx)] = 0;
}

// copies `count` QPs worth of one model array
int
copy_in(double* dst_base, const double* src, int64_t idx, int64_t B, size_t per_qp)
{
  if (!src || per_qp == 0)
    return PQP_OK;
  if (idx < 0) {
    HIP_TRY(hipMemcpy(dst_base, src, per_qp * size_t(B) * sizeof(double), hipMemcpyDefault));
  } else {
    HIP_TRY(hipMemcpy(dst_base + size_t(idx) * per_qp, src, per_qp * sizeof(double), hipMemcpyDefault));
  }
  return PQP_OK;
}

int
copy_out(double* dst, const double* src_base, int64_t idx, int64_t B, size_t per_qp)
{
  if (!dst || per_qp == 0)
    return PQP_OK;
  if (idx < 0) {
    HIP_TRY(hipMemcpy(dst, src_base, per_qp * size_t(B) * sizeof(double), hipMemcpyDefault));
  } else {
    HIP_TRY(hipMemcpy(dst, src_base + size_t(idx) * per_qp, per_qp * sizeof(double), hipMemcpyDefault));
  }
  return PQP_OK;
}

// the scalar half of QP::init / QP::update that lives in `settings`
// (reference dense/wrapper.hpp:375, 754-759; helpers.hpp:174-189, 678-705)
void
host_settings_state_machine(pqp_settings& st, bool is_init, int precond_flag, double rho, double mu_eq,
                            double mu_in, double min_eig)
{
  if (is_init)
    st.compute_preconditioner = precond_flag;
  else
    st.update_preconditioner = precond_flag;
  if (!absent(rho))
    st.default_rho = rho;
  if (!absent(mu_eq))
    st.default_mu_eq = mu_eq;
  if (!absent(mu_in))
    st.default_mu_in = mu_in;
  if (!absent(min_eig))
    st.default_H_eigenvalue_estimate = min_eig;
  // results.info.minimal_H_eigenvalue_estimate always equals
  // settings.default_H_eigenvalue_estimate (results.hpp:175-194, helpers.hpp:181-186)
  st.default_rho += std::fabs(st.default_H_eigenvalue_estimate);
}

// copies `count` QPs worth of one model array to the QPs lo .. lo + count - 1
int
copy_in_range(double* dst_base, const double* src, int64_t lo, int64_t count, size_t per_qp)
{
  if (!src || per_qp == 0 || count == 0)
    return PQP_OK;
  HIP_TRY(hipMemcpy(dst_base + size_t(lo) * per_qp, src, per_qp * size_t(count) * sizeof(double), hipMemcpyDefault));
  return PQP_OK;
}

// `p` is memory of device `device`, which a kernel of the handle may read in place
bool
device_resident(const void* p, int device)
{
#ifdef PQP_EMULATED_MFMA
  (void)p, (void)device; // (the emulated device is the host: every shared array takes the staging path there)
  return false;
#else
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError(); // (an address the runtime does not know: pageable host memory)
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == device;
#endif
}

// init / update of the QPs lo .. hi - 1.  An array whose bit is set in `shared_mask` (PQP_SHARED_*) holds ONE QP's worth,
// given to every QP of the range by the broadcast kernel (pqp_shared.hpp); the others hold hi - lo QPs' worth.
int
enqueue_setup_range(pqp_batch* h, int64_t lo, int64_t hi, int shared_mask, bool update_call, const double* H, const double* g,
                    const double* A, const double* b, const double* C, const double* l, const double* u,
                    const double* l_box, const double* u_box, int precond_flag, double rho, double mu_eq,
                    double mu_in, double min_eig, const double* min_eig_per_qp)
{
  if (int rc = settle(h))
    return rc;
  // (setup resets or rescales the results by the initial guess, helpers.hpp:522-572)
  if (lo == 0 && hi == h->dev.B)
    mirror_stale(h, -1);
  else
    for (int64_t q = lo; q < hi; ++q)
      mirror_stale(h, q);
  const pqp::Dims& d = h->dev.d;
  // wrapper.hpp:367-372, 542-546, 736-741, 846-850
  if (!d.box && (l_box || u_box))
    return fail(PQP_ERR_INVALID_ARGUMENT,
                "wrong model setup: the QP object is designed without box constraints, but is "
                "initialized or updated with lower or upper box inequalities.");
  PQP_ON_DEVICE(h->device);
  // one queued command per QP: run what is pending before stacking another one
  for (int64_t q = lo; q < hi; ++q)
    if (h->cmd[size_t(q)].op != pqp::CMD_NONE) {
      if (int rc = pqp_batch_flush(h))
        return rc;
      break;
    }
  const size_t n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  pqp::Batch& D = h->dev;
  struct In
  {
    double* dst;
    const double* src;
    size_t per_qp;
    int bit;
  };
  const In in[9] = { { D.H, H, n * n, PQP_SHARED_H },   { D.g, g, n, PQP_SHARED_G },   { D.A, A, ne * n, PQP_SHARED_A },
                     { D.b, b, ne, PQP_SHARED_B },      { D.C, C, ni * n, PQP_SHARED_C }, { D.l, l, ni, PQP_SHARED_L },
                     { D.u, u, ni, PQP_SHARED_U },      { D.l_box, l_box, n, PQP_SHARED_LBOX },
                     { D.u_box, u_box, n, PQP_SHARED_UBOX } };
  // the shared arrays that live on the host are staged side by side (the broadcasts run on the handle's stream while
  // the next blocking copy is made); those on the handle's device are read in place
  bool staged[9] = {};
  size_t stage = 0;
  for (int k = 0; k < 9; ++k)
    if (in[k].src && in[k].per_qp && (shared_mask & in[k].bit) && !device_resident(in[k].src, h->device)) {
      staged[k] = true;
      stage += in[k].per_qp;
    }
  if (stage)
    if (int rc = grow(h, &h->shared_stage, &h->shared_stage_cap, stage))
      return rc;
  bool launched = false;
  stage = 0;
  for (int k = 0; k < 9; ++k) {
    const In& a = in[k];
    if (!a.src || a.per_qp == 0)
      continue;
    if (!(shared_mask & a.bit)) {
      if (int rc = copy_in_range(a.dst, a.src, lo, hi - lo, a.per_qp))
        return rc;
      continue;
    }
    const double* src = a.src;
    if (staged[k]) {
      HIP_TRY(hipMemcpy(h->shared_stage + stage, a.src, a.per_qp * sizeof(double), hipMemcpyDefault));
      src = h->shared_stage + stage;
      stage += a.per_qp;
    }
    if (int rc = pqp_launch_broadcast(h, src, a.dst, long(a.per_qp), long(lo), long(hi - lo)))
      return rc;
    launched = true;
  }
  if (launched) // the call returns when the source arrays (and the staging buffer) may be overwritten
    HIP_TRY(hipStreamSynchronize(h->stream));
  for (int64_t q = lo; q < hi; ++q) {
    pqp_settings& st = h->settings[size_t(q)];
    bool is_init = !update_call || !h->is_initialized[size_t(q)];
    // (the _eig entries: a host array with one value per addressed QP; the scalar entries pass nullptr)
    double me = min_eig_per_qp ? min_eig_per_qp[q - lo] : min_eig;
    if (update_call && is_init)
      me = std::numeric_limits<double>::quiet_NaN(); // wrapper.hpp:743-746 does not forward it
    host_settings_state_machine(st, is_init, precond_flag, rho, mu_eq, mu_in, me);
    pqp::Cmd c{};
    c.op = is_init ? pqp::CMD_INIT : pqp::CMD_UPDATE;
    c.preconditioner = precond_flag;
    c.matrices_given = (H || A || C) ? 1 : 0;
    c.rho = rho;
    c.mu_eq = mu_eq;
    c.mu_in = mu_in;
    c.min_eig = me;
    h->cmd[size_t(q)] = c;
    if (h->cmd_settings.size() != h->settings.size())
      h->cmd_settings = h->settings;
    h->cmd_settings[size_t(q)] = st;
    if (is_init) {
      h->is_initialized[size_t(q)] = 1;
    } else {
      // setup() -> work.cleanup() clears is_initialized except on the keep-everything
      // WARM_START_WITH_PREVIOUS_RESULT path (helpers.hpp:522-572, workspace.hpp:372)
      bool ppu = !absent(rho) || !absent(mu_eq) || !absent(mu_in);
      bool keep = st.initial_guess == PQP_WARM_START_WITH_PREVIOUS_RESULT && !c.matrices_given && !ppu;
      if (!keep)
        h->is_initialized[size_t(q)] = 0;
    }
  }
  h->cmd_pending = true;
  return PQP_OK;
}

int
enqueue_setup(pqp_batch* h, int64_t idx, bool update_call, const double* H, const double* g,
              const double* A, const double* b, const double* C, const double* l, const double* u,
              const double* l_box, const double* u_box, int precond_flag, double rho, double mu_eq,
              double mu_in, double min_eig, const double* min_eig_per_qp = nullptr)
{
  if (int rc = check_idx(h, idx))
    return rc;
  return enqueue_setup_range(h, idx < 0 ? 0 : idx, idx < 0 ? h->dev.B : idx + 1, 0, update_call, H, g, A, b, C, l, u, l_box,
                             u_box, precond_flag, rho, mu_eq, mu_in, min_eig, min_eig_per_qp);
}

int
enqueue_setup_shared(pqp_batch* h, int64_t first, int64_t count, int shared_mask, bool update_call, const double* H,
                     const double* g, const double* A, const double* b, const double* C, const double* l, const double* u,
                     const double* l_box, const double* u_box, int precond_flag, double rho, double mu_eq, double mu_in,
                     double min_eig)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (first < 0 || count < 0 || first > h->dev.B || count > h->dev.B - first)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP range outside the batch");
  if (count == 0)
    return PQP_OK;
  return enqueue_setup_range(h, first, first + count, shared_mask, update_call, H, g, A, b, C, l, u, l_box, u_box,
                             precond_flag, rho, mu_eq, mu_in, min_eig, nullptr);
}

} // namespace

extern "C" {

const char*
pqp_last_error(void)
{
  return g_err.c_str();
}

int
pqp_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int
pqp_batch_create(int64_t batch_size, int64_t dim, int64_t n_eq, int64_t n_in, int box_constraints,
                 int hessian_type, int dense_backend, int device, pqp_batch** out)
{
  if (!out)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null output handle");
  *out = nullptr;
  if (dim <= 0) // reference dense/model.hpp:65-68
    return fail(PQP_ERR_INVALID_ARGUMENT,
                "wrong argument size: the dimension wrt the primal variable x should be strictly positive.");
  if (batch_size < 0 || n_eq < 0 || n_in < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "negative size");
  if (hessian_type < PQP_HESSIAN_ZERO || hessian_type > PQP_HESSIAN_DIAGONAL)
    return fail(PQP_ERR_INVALID_ARGUMENT, "unknown hessian type");
  int ndev = pqp_device_count();
  if (ndev <= 0)
    return fail(PQP_ERR_NO_DEVICE, "no HIP device: libproxqp_hip has no CPU fallback");
  if (device < 0 || device >= ndev)
    return fail(PQP_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  PQP_ON_DEVICE(device);

  pqp_batch* h = new pqp_batch();
  h->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      h->n_cu = cus;
    // wall_clock64() of the device: constant-rate counter, rate in kHz (100 MHz on CDNA) -> Info timings
    int khz = 0;
    h->dev.wall_us_per_tick =
      (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) ? 1.0e3 / double(khz)
                                                                                                      : 1.0e-2;
  }
  h->backend = dense_backend_choice(dense_backend, dim, n_eq, n_in, box_constraints != 0);
  pqp::Dims& d = h->dev.d;
  d.n = int(dim);
  d.n_eq = int(n_eq);
  d.n_in = int(n_in);
  d.box = box_constraints ? 1 : 0;
  d.nc = int(n_in + (box_constraints ? dim : 0));
  d.nd = d.n_eq + d.nc;
  d.ntot = d.n + d.nd;
  d.hessian = hessian_type;
  d.backend = h->backend;
  d._pad = 0;
  h->dev.B = batch_size;
  const int need = d.nd > d.n ? d.nd : d.n;
  h->nt = need <= 256 ? 256 : (need <= 512 ? 512 : 1024);
  // Above 1024 rows the 1024-thread kernel walks its one-thread-per-row stages in chunks (the reference has no size
  // limit, dense/model.hpp:65-68; linalg/dense/factorize.hpp:360-370 switches to a blocked factorisation there).  What
  // bounds a batch here: the 16-bit constraint ids of the persistent slot list and the LDS of the set-up kernel
  // (2 (n + n_eq + n_c) doubles of Ruiz scaling).
  if (need > PQP_MAX_ROWS || pqp::setup_lds_bytes(d, 1024) > 160 * 1024) {
    delete h;
    return fail(PQP_ERR_UNSUPPORTED, "max(n, n_eq + n_in (+ n)) > " + std::to_string(PQP_MAX_ROWS) +
                                       " (or n + n_eq + n_in (+ n) > ~10000) is not supported by this build");
  }
#if PQP_CHUNK_ALL
  if (const char* e = std::getenv("PQP_TEST_NT_MAX")) { // test hook of the emulator variant: a workgroup narrower than the rows
    const int f = std::atoi(e);
    if ((f == 256 || f == 512) && h->nt > f)
      h->nt = f;
  }
#endif
  if (const char* e = std::getenv("PQP_SCHEDULE"))
    h->lpt = std::string(e) == "lpt";
  h->dev.rep_phase = 0;
  h->dev.rep_count = 1;
  h->dev.trace = nullptr;
  h->dev.trace_slot = nullptr;
  h->dev.trace_cap = 0;
  if (const char* e = std::getenv("PQP_REPEAT_PHASE")) // (only the instrumented build reads them: traffic attribution)
    h->dev.rep_phase = std::atoi(e);
  if (const char* e = std::getenv("PQP_REPEAT_COUNT"))
    h->dev.rep_count = std::atoi(e);
  h->lds_solve = pqp::lds_bytes(d, h->nt);
  h->lds_setup = pqp::setup_lds_bytes(d, h->nt);
  // per-QP vector state beyond the 160 KiB of LDS of one CU (e.g. n = 760 with 837 constraint rows): the
  // solver then runs with 1024 threads on a slice of HBM per workgroup (allocated below)
  // (PQP_FORCE_HBM_VECTORS=1: any shape takes that path -- test hook: small problems through the large-shape kernel)
  const char* force_hbm = std::getenv("PQP_FORCE_HBM_VECTORS");
  const bool vectors_in_hbm = h->lds_solve > 160 * 1024 || (force_hbm && force_hbm[0] == '1');
  if (vectors_in_hbm)
    h->nt = 1024;
  const size_t B = size_t(batch_size), n = size_t(dim), ne = size_t(n_eq), ni = size_t(n_in),
               nc = size_t(d.nc), nd = size_t(d.nd);
  pqp::Batch& D = h->dev;
  int rc = 0;
#define ALLOC(ptr, cnt)                                                                             \
  if ((rc = dalloc(h, &(ptr), (cnt)))) {                                                            \
    pqp_batch_destroy(h);                                                                           \
    return rc;                                                                                      \
  }                                                                                                 \
  if (B > 0 && size_t(cnt) % B == 0 && (void*)(ptr) != (void*)h->d_order && (void*)(ptr) != (void*)h->d_cmd)           \
    h->per_qp.push_back({ reinterpret_cast<char*>(ptr), (size_t(cnt) / B) * sizeof(*(ptr)) });
  ALLOC(D.H, B * n * n)
  ALLOC(D.g, B * n)
  ALLOC(D.A, B * ne * n)
  ALLOC(D.b, B * ne)
  ALLOC(D.C, B * ni * n)
  ALLOC(D.u, B * ni)
  ALLOC(D.l, B * ni)
  ALLOC(D.u_box, B * n)
  ALLOC(D.l_box, B * n)
  ALLOC(D.Hs, B * n * n)
  ALLOC(D.gs, B * n)
  ALLOC(D.As, B * ne * n)
  ALLOC(D.ATs, B * ne * n)
  ALLOC(D.bs, B * ne)
  ALLOC(D.Cs, B * ni * n)
  ALLOC(D.CTs, B * ni * n)
  ALLOC(D.us, B * ni)
  ALLOC(D.ls, B * ni)
  ALLOC(D.ubs, B * n)
  ALLOC(D.lbs, B * n)
  ALLOC(D.is, B * n)
  ALLOC(D.delta, B * size_t(d.ntot))
  ALLOC(D.x, B * n)
  ALLOC(D.y, B * ne)
  ALLOC(D.z, B * nc)
  ALLOC(D.se, B * ne)
  ALLOC(D.si, B * nc)
  ALLOC(D.info, B)
  ALLOC(D.state, B)
  ALLOC(D.F, B * n * n)
  ALLOC(D.WL, B * n * n)
  ALLOC(D.WU, B * n * n)
  ALLOC(D.dF, B * n)
  ALLOC(D.Zr, B * nd * n)
  ALLOC(D.Zc, B * nd * n)
  ALLOC(D.G, B * nd * nd)
  ALLOC(D.WS, B * nd * nd)
  ALLOC(D.LS, B * nd * nd)
  ALLOC(D.dS, B * nd)
  ALLOC(D.act, B * nc)
  ALLOC(D.stats, B * size_t(pqp::ST_COUNT))
  if (vectors_in_hbm) {
    h->lds_solve = pqp::lds_bytes(d, h->nt);
    h->lds_setup = pqp::setup_lds_bytes(d, h->nt);
    if ((rc = dalloc(h, &h->vec_scratch, B * ((h->lds_solve + 7) / 8)))) {
      pqp_batch_destroy(h);
      return rc;
    }
  }
  ALLOC(h->d_order, B)
  ALLOC(h->d_settings, B)
  ALLOC(h->d_cmd, B)
#undef ALLOC
  D.settings = h->d_settings;
  D.cmd = h->d_cmd;

  // host-side defaults: Settings(dense_backend) (settings.hpp:213-315), Results(...)
  // (results.hpp:90-144), Model bounds +-sqrt(DBL_MAX) (model.hpp:70-91), Ruiz delta = 1
  h->settings.resize(B);
  for (auto& s : h->settings)
    pqp_settings_default(&s, h->backend);
  h->cmd.assign(B, pqp::Cmd{});
  h->is_initialized.assign(B, 0);
  h->c_diag.assign(B, 0);
  {
    std::vector<pqp_info> info(B);
    for (auto& i : info)
      pqp_info_default(&i, h->backend);
    if (B)
      HIP_TRY(hipMemcpy(D.info, info.data(), B * sizeof(pqp_info), hipMemcpyHostToDevice));
    std::vector<pqp::State> st(B);
    for (auto& s : st) {
      std::memset(&s, 0, sizeof(s));
      s.ruiz_c = 1.0;
    }
    if (B)
      HIP_TRY(hipMemcpy(D.state, st.data(), B * sizeof(pqp::State), hipMemcpyHostToDevice));
    const double ib = std::sqrt(std::numeric_limits<double>::max());
    std::vector<double> tmp;
    auto fill = [&](double* dst, size_t cnt, double v) -> int {
      if (!cnt)
        return PQP_OK;
      tmp.assign(cnt, v);
      HIP_TRY(hipMemcpy(dst, tmp.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
      return PQP_OK;
    };
    if ((rc = fill(D.u, B * ni, +ib)) || (rc = fill(D.l, B * ni, -ib)) ||
        (rc = fill(D.u_box, B * n, +ib)) || (rc = fill(D.l_box, B * n, -ib)) ||
        (rc = fill(D.delta, B * size_t(d.ntot), 1.0)) || (rc = fill(D.is, B * n, 1.0))) {
      pqp_batch_destroy(h);
      return rc;
    }
  }
  HIP_TRY(hipEventCreate(&h->ev0));
  HIP_TRY(hipEventCreate(&h->ev1));
  HIP_TRY(hipEventCreate(&h->ev_mid));
  *out = h;
  return PQP_OK;
}

void
pqp_batch_destroy(pqp_batch* h)
{
  if (!h)
    return;
  (void)settle(h);
  pqp_batch_destroy(h->inner);
  DeviceGuard guard_(h->device);
  for (void* p : h->host_allocs)
    (void)hipHostFree(p);
  if (h->owned_stream)
    (void)hipStreamDestroy(h->owned_stream);
  for (void* p : h->allocs)
    (void)hipFree(p);
  if (h->trace_dev)
    (void)hipFree(h->trace_dev);
  if (h->trace_slot_dev)
    (void)hipFree(h->trace_slot_dev);
  if (h->ev0)
    (void)hipEventDestroy(h->ev0);
  if (h->ev1)
    (void)hipEventDestroy(h->ev1);
  if (h->ev_mid)
    (void)hipEventDestroy(h->ev_mid);
  delete h;
}

int64_t
pqp_batch_size(const pqp_batch* h)
{
  return h ? h->dev.B : 0;
}

int
pqp_batch_dense_backend(const pqp_batch* h)
{
  return h ? h->backend : PQP_BACKEND_AUTOMATIC;
}

pqp_settings*
pqp_batch_settings(pqp_batch* h, int64_t idx)
{
  if (!h || idx < 0 || idx >= h->dev.B)
    return nullptr;
  return &h->settings[size_t(idx)];
}

int
pqp_batch_init(pqp_batch* h, int64_t idx, const double* H, const double* g, const double* A,
               const double* b, const double* C, const double* l, const double* u,
               const double* l_box, const double* u_box, int compute_preconditioner, double rho,
               double mu_eq, double mu_in, double manual_minimal_H_eigenvalue)
{
  if (h && h->dev.d.box == 0 && (l_box || u_box))
    return fail(PQP_ERR_INVALID_ARGUMENT,
                "wrong model setup: the QP object is designed without box constraints, but is "
                "initialized with lower or upper box inequalities."); // wrapper.hpp:542-546
  return enqueue_setup(h, idx, false, H, g, A, b, C, l, u, l_box, u_box, compute_preconditioner ? 1 : 0,
                       rho, mu_eq, mu_in, manual_minimal_H_eigenvalue);
}

int
pqp_batch_update(pqp_batch* h, int64_t idx, const double* H, const double* g, const double* A,
                 const double* b, const double* C, const double* l, const double* u,
                 const double* l_box, const double* u_box, int update_preconditioner, double rho,
                 double mu_eq, double mu_in, double manual_minimal_H_eigenvalue)
{
  return enqueue_setup(h, idx, true, H, g, A, b, C, l, u, l_box, u_box, update_preconditioner ? 1 : 0,
                       rho, mu_eq, mu_in, manual_minimal_H_eigenvalue);
}

int
pqp_batch_init_shared(pqp_batch* h, int64_t first, int64_t count, const double* H, const double* g, const double* A,
                      const double* b, const double* C, const double* l, const double* u, const double* l_box,
                      const double* u_box, int shared_mask, int compute_preconditioner, double rho, double mu_eq,
                      double mu_in, double manual_minimal_H_eigenvalue)
{
  if (h && h->dev.d.box == 0 && (l_box || u_box))
    return fail(PQP_ERR_INVALID_ARGUMENT,
                "wrong model setup: the QP object is designed without box constraints, but is "
                "initialized with lower or upper box inequalities."); // wrapper.hpp:542-546
  return enqueue_setup_shared(h, first, count, shared_mask, false, H, g, A, b, C, l, u, l_box, u_box,
                              compute_preconditioner ? 1 : 0, rho, mu_eq, mu_in, manual_minimal_H_eigenvalue);
}

int
pqp_batch_update_shared(pqp_batch* h, int64_t first, int64_t count, const double* H, const double* g, const double* A,
                        const double* b, const double* C, const double* l, const double* u, const double* l_box,
                        const double* u_box, int shared_mask, int update_preconditioner, double rho, double mu_eq,
                        double mu_in, double manual_minimal_H_eigenvalue)
{
  return enqueue_setup_shared(h, first, count, shared_mask, true, H, g, A, b, C, l, u, l_box, u_box,
                              update_preconditioner ? 1 : 0, rho, mu_eq, mu_in, manual_minimal_H_eigenvalue);
}

int
pqp_batch_init_eig(pqp_batch* h, int64_t idx, const double* H, const double* g, const double* A,
                   const double* b, const double* C, const double* l, const double* u,
                   const double* l_box, const double* u_box, int compute_preconditioner, double rho,
                   double mu_eq, double mu_in, const double* manual_minimal_H_eigenvalue)
{
  if (h && h->dev.d.box == 0 && (l_box || u_box))
    return fail(PQP_ERR_INVALID_ARGUMENT,
                "wrong model setup: the QP object is designed without box constraints, but is "
                "initialized with lower or upper box inequalities."); // wrapper.hpp:542-546
  return enqueue_setup(h, idx, false, H, g, A, b, C, l, u, l_box, u_box, compute_preconditioner ? 1 : 0,
                       rho, mu_eq, mu_in, std::numeric_limits<double>::quiet_NaN(), manual_minimal_H_eigenvalue);
}

int
pqp_batch_update_eig(pqp_batch* h, int64_t idx, const double* H, const double* g, const double* A,
                     const double* b, const double* C, const double* l, const double* u,
                     const double* l_box, const double* u_box, int update_preconditioner, double rho,
                     double mu_eq, double mu_in, const double* manual_minimal_H_eigenvalue)
{
  return enqueue_setup(h, idx, true, H, g, A, b, C, l, u, l_box, u_box, update_preconditioner ? 1 : 0,
                       rho, mu_eq, mu_in, std::numeric_limits<double>::quiet_NaN(), manual_minimal_H_eigenvalue);
}

// dense::estimate_minimal_eigen_value_of_symmetric_matrix on `count` matrices in one launch (pqp_eig.hpp)
int
pqp_estimate_min_eigenvalues(int device, int64_t count, int64_t n, const double* H, int method,
                             double power_iteration_accuracy, int64_t nb_power_iteration, double* out, void* stream)
{
  if (count < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "negative number of matrices");
  if (count == 0)
    return PQP_OK;
  if (!H || !out)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  if (method != PQP_EIG_POWER_ITERATION && method != PQP_EIG_EXACT_METHOD)
    return fail(PQP_ERR_INVALID_ARGUMENT, "unknown eigenvalue estimate method");
  if (n < 1) // (the reference's Eigen calls have nothing to work on)
    return fail(PQP_ERR_INVALID_ARGUMENT, "the order of H should be strictly positive.");
  if (n > PQP_MAX_ROWS)
    return fail(PQP_ERR_UNSUPPORTED, "order of H > " + std::to_string(PQP_MAX_ROWS) + " is not supported by this build");
  if (count > 0x7fffffffll)
    return fail(PQP_ERR_UNSUPPORTED, "more than 2^31 - 1 matrices in one call");
  int ndev = pqp_device_count();
  if (ndev <= 0)
    return fail(PQP_ERR_NO_DEVICE, "no HIP device: libproxqp_hip has no CPU fallback");
  if (device < 0 || device >= ndev)
    return fail(PQP_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  PQP_ON_DEVICE(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // everything the call allocates, freed on every way out
  struct Scratch
  {
    std::vector<void*> p;
    ~Scratch()
    {
      for (void* q : p)
        (void)hipFree(q);
    }
    int get(void** out, size_t bytes)
    {
      HIP_TRY(hipMalloc(out, bytes));
      p.push_back(*out);
      return PQP_OK;
    }
  } scratch;
  const size_t nn = size_t(n) * size_t(n), B = size_t(count);
  pqp::EigArgs a{};
  a.n = int(n);
  a.method = method;
  a.accuracy = power_iteration_accuracy;
  a.nb = long(nb_power_iteration);
  a.H = H;
  if (!pqp_device_readable(H)) { // host input: staged to the device in one copy
    void* d = nullptr;
    if (int rc = scratch.get(&d, B * nn * sizeof(double)))
      return rc;
    HIP_TRY(hipMemcpyAsync(d, H, B * nn * sizeof(double), hipMemcpyHostToDevice, st));
    a.H = static_cast<const double*>(d);
  }
  // per matrix: the estimate, ||H - H^T||_F and ||H||_F
  void* d_res = nullptr;
  if (int rc = scratch.get(&d_res, B * 3 * sizeof(double)))
    return rc;
  a.res = static_cast<double*>(d_res);
  // PQP_EIG_RESIDENT=0 / 1 forces the streamed / the LDS-resident form where both exist (the A/B partners of
  // scripts/eig_bench.py and of the tests; read per call)
  a.resident = pqp::eig_resident(a.n) ? 1 : 0;
  if (const char* e = std::getenv("PQP_EIG_RESIDENT"))
    a.resident = (e[0] == '1' && pqp::eig_lds_bytes(a.n, true) <= 160 * 1024) ? 1 : (e[0] == '0' ? 0 : a.resident);
  if (method == PQP_EIG_EXACT_METHOD && !a.resident) { // the working copy of the tridiagonalisation: a slice of HBM per matrix
    void* w = nullptr;
    if (int rc = scratch.get(&w, B * nn * sizeof(double)))
      return rc;
    a.work = static_cast<double*>(w);
  }
  if (int rc = pqp_launch_eig(a, long(count), st))
    return rc;
  std::vector<double> res(B * 3);
  HIP_TRY(hipMemcpyAsync(res.data(), d_res, B * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // helpers.hpp:131-134: !H.isApprox(H^T, eps)  <=>  ||H - H^T||_F > eps min(||H||_F, ||H^T||_F)  (a zero matrix passes)
  for (size_t q = 0; q < B; ++q)
    if (!(res[3 * q + 1] <= std::numeric_limits<double>::epsilon() * res[3 * q + 2]))
      return fail(PQP_ERR_INVALID_ARGUMENT, "H is not symmetric. (matrix " + std::to_string(q) + " of the batch)");
  std::vector<double> vals(B);
  for (size_t q = 0; q < B; ++q)
    vals[q] = res[3 * q];
  HIP_TRY(hipMemcpy(out, vals.data(), B * sizeof(double), hipMemcpyDefault));
  return PQP_OK;
}

int
pqp_batch_warm_start(pqp_batch* h, int64_t idx, const double* x, const double* y, const double* z)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (!x && !y && !z) // helpers.hpp:724-725
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  mirror_stale(h, idx);
  PQP_ON_DEVICE(h->device);
  // the guess must land after any queued cleanup of the results
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const pqp::Dims& d = h->dev.d;
  int rc = 0;
  if ((rc = copy_in(h->dev.x, x, idx, h->dev.B, size_t(d.n))) ||
      (rc = copy_in(h->dev.y, y, idx, h->dev.B, size_t(d.n_eq))) ||
      (rc = copy_in(h->dev.z, z, idx, h->dev.B, size_t(d.nc))))
    return rc;
  const int64_t lo = idx < 0 ? 0 : idx, hi = idx < 0 ? h->dev.B : idx + 1;
  for (int64_t q = lo; q < hi; ++q)
    h->settings[size_t(q)].initial_guess = PQP_WARM_START; // helpers.hpp:727
  return PQP_OK;
}

int
pqp_batch_cleanup(pqp_batch* h, int64_t idx)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (int rc = settle(h))
    return rc;
  mirror_stale(h, idx);
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const int64_t lo = idx < 0 ? 0 : idx, hi = idx < 0 ? h->dev.B : idx + 1;
  for (int64_t q = lo; q < hi; ++q) {
    pqp::Cmd c{};
    c.op = pqp::CMD_CLEANUP;
    h->cmd[size_t(q)] = c;
    h->is_initialized[size_t(q)] = 0;
  }
  h->cmd_pending = true;
  return pqp_batch_flush(h);
}

// A slot handed to a NEW QP object (the C++ facade recycles the slots of its pools): everything a
// freshly created batch holds for that QP -- Settings(dense_backend), Results, Model (zero matrices,
// bounds +-sqrt(DBL_MAX)), workspace flags, Ruiz delta = 1 (reference dense/wrapper.hpp:140-333: every
// constructor starts from defaults).
int
pqp_batch_reset_qp(pqp_batch* h, int64_t idx)
{
  if (!h || idx < 0 || idx >= h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
  if (int rc = settle(h))
    return rc;
  mirror_stale(h, idx);
  PQP_ON_DEVICE(h->device);
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const size_t q = size_t(idx);
  for (const auto& a : h->per_qp)
    HIP_TRY(hipMemset(a.base + q * a.bytes_per_qp, 0, a.bytes_per_qp));
  pqp::Batch& D = h->dev;
  const pqp::Dims& d = D.d;
  const size_t n = size_t(d.n), ni = size_t(d.n_in);
  pqp_info info;
  pqp_info_default(&info, h->backend);
  HIP_TRY(hipMemcpy(D.info + q, &info, sizeof(info), hipMemcpyHostToDevice));
  pqp::State st;
  std::memset(&st, 0, sizeof(st));
  st.ruiz_c = 1.0;
  HIP_TRY(hipMemcpy(D.state + q, &st, sizeof(st), hipMemcpyHostToDevice));
  const double ib = std::sqrt(std::numeric_limits<double>::max());
  std::vector<double> tmp;
  auto fill = [&](double* dst, size_t cnt, double v) -> int {
    if (!cnt)
      return PQP_OK;
    tmp.assign(cnt, v);
    HIP_TRY(hipMemcpy(dst, tmp.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    return PQP_OK;
  };
  int rc = 0;
  if ((rc = fill(D.u + q * ni, ni, +ib)) || (rc = fill(D.l + q * ni, ni, -ib)) ||
      (rc = fill(D.u_box + q * n, n, +ib)) || (rc = fill(D.l_box + q * n, n, -ib)) ||
      (rc = fill(D.delta + q * size_t(d.ntot), size_t(d.ntot), 1.0)) || (rc = fill(D.is + q * n, n, 1.0)))
    return rc;
  pqp_settings_default(&h->settings[q], h->backend);
  h->settings_dirty = true;
  h->settings_uploaded.clear(); // (the slice of d_settings was zeroed above: force a re-upload)
  h->cmd[q] = pqp::Cmd{};
  h->is_initialized[q] = 0;
  h->c_diag[q] = 0;
  h->order_valid = false;
  return PQP_OK;
}

int
pqp_batch_flush(pqp_batch* h)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (!h->cmd_pending || h->dev.B == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = upload_settings(h))
    return rc;
  // only the span of QPs that carry a command is uploaded and launched (a BatchQP filled QP by
  // QP through the facade flushes once per QP: B launches of one workgroup, not B launches of B)
  size_t lo = h->cmd.size(), hi = 0;
  for (size_t q = 0; q < h->cmd.size(); ++q)
    if (h->cmd[q].op != pqp::CMD_NONE) {
      lo = std::min(lo, q);
      hi = q + 1;
    }
  if (lo < hi) {
    HIP_TRY(hipMemcpy(h->d_cmd + lo, h->cmd.data() + lo, (hi - lo) * sizeof(pqp::Cmd), hipMemcpyHostToDevice));
    // init / update run under the settings of the moment they were called
    bool stale = false;
    if (h->cmd_settings.size() == h->settings.size()) {
      std::vector<pqp_settings> snap(h->settings.begin() + long(lo), h->settings.begin() + long(hi));
      for (size_t q = lo; q < hi; ++q)
        if ((h->cmd[q].op == pqp::CMD_INIT || h->cmd[q].op == pqp::CMD_UPDATE) &&
            std::memcmp(&h->cmd_settings[q], &h->settings[q], sizeof(pqp_settings)) != 0) {
          snap[q - lo] = h->cmd_settings[q];
          stale = true;
        }
      if (stale)
        HIP_TRY(hipMemcpy(h->d_settings + lo, snap.data(), (hi - lo) * sizeof(pqp_settings), hipMemcpyHostToDevice));
    }
    h->setup_first = long(lo);
    h->setup_count = long(hi - lo);
    if (int rc = pqp_launch_setup(h))
      return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    {
      const pqp::Dims& dd = h->dev.d;
      if (h->nt == 256 && pqp::diag_structure_signature(dd.hessian, dd.n_eq, dd.n_in, dd.box)) {
        // which QPs have diagonal structure (decided by the kernel that just ran, from the model's data)
        std::vector<pqp::State> stt(hi - lo);
        HIP_TRY(hipMemcpy(stt.data(), h->dev.state + lo, (hi - lo) * sizeof(pqp::State), hipMemcpyDeviceToHost));
        for (size_t q = lo; q < hi; ++q)
          h->c_diag[q] = stt[q - lo].c_diag != 0;
      }
    }
    if (stale) // back to the live settings for the solve
      HIP_TRY(hipMemcpy(h->d_settings + lo, h->settings.data() + lo, (hi - lo) * sizeof(pqp_settings),
                        hipMemcpyHostToDevice));
    for (size_t q = lo; q < hi; ++q)
      h->cmd[q].op = pqp::CMD_NONE;
  }
  h->cmd_pending = false;
  return PQP_OK;
}

int
pqp_batch_set_stream(pqp_batch* h, void* stream)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (int rc = settle(h)) // (a solve in flight stays on the stream it was launched on)
    return rc;
  if (h->owned_stream && static_cast<hipStream_t>(stream) != h->owned_stream) {
    PQP_ON_DEVICE(h->device);
    (void)hipStreamDestroy(h->owned_stream);
    h->owned_stream = nullptr;
  }
  h->stream = static_cast<hipStream_t>(stream);
  return PQP_OK;
}

int
pqp_batch_own_stream(pqp_batch* h)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (h->owned_stream)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  HIP_TRY(hipStreamCreateWithFlags(&h->owned_stream, hipStreamNonBlocking));
  h->stream = h->owned_stream;
  return PQP_OK;
}

int
pqp_batch_set_schedule(pqp_batch* h, int longest_first)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  h->lpt = longest_first != 0;
  return PQP_OK;
}

int
pqp_batch_solve(pqp_batch* h)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  return pqp_batch_solve_range(h, 0, h->dev.B);
}

constexpr int PQP_TRACE_RECORDS = 4096; // per verbose QP and launch, the header record included (256 KB)

// settings.verbose: the slab of per-iteration records for the verbose QPs of the launch about to be enqueued
// (pqp::Batch::trace); no verbose QP: the kernel gets a null pointer and the previous trace is dropped
static int
prepare_trace(pqp_batch* h, const int64_t* idx, int64_t first, int64_t count)
{
  h->dev.trace = nullptr;
  h->dev.trace_slot = nullptr;
  h->dev.trace_cap = 0;
  h->trace_host.clear();
  int64_t nv = 0;
  for (int64_t i = 0; i < count; ++i)
    nv += h->settings[size_t(idx ? idx[i] : first + i)].verbose != 0;
  if (nv == 0) {
    h->trace_slot.clear();
    return PQP_OK;
  }
  h->trace_slot.assign(size_t(h->dev.B), -1);
  int slot = 0;
  for (int64_t i = 0; i < count; ++i) {
    const size_t q = size_t(idx ? idx[i] : first + i);
    if (h->settings[q].verbose != 0)
      h->trace_slot[q] = slot++;
  }
  const size_t slot_bytes = size_t(PQP_TRACE_RECORDS) * 8 * sizeof(double);
  if (nv > h->trace_slots) {
    if (h->trace_dev)
      (void)hipFree(h->trace_dev);
    h->trace_dev = nullptr;
    h->trace_slots = 0;
    HIP_TRY(hipMalloc((void**)&h->trace_dev, size_t(nv) * slot_bytes));
    h->trace_slots = nv;
  }
  if (!h->trace_slot_dev)
    HIP_TRY(hipMalloc((void**)&h->trace_slot_dev, size_t(h->dev.B) * sizeof(int)));
  // (a synchronous copy: a verbose solve is a debugging run)
  HIP_TRY(hipMemcpy(h->trace_slot_dev, h->trace_slot.data(), size_t(h->dev.B) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(h->trace_dev, 0, size_t(nv) * slot_bytes, h->stream)); // (on the launch stream: ordered in front of the kernel)
  h->dev.trace = h->trace_dev;
  h->dev.trace_slot = h->trace_slot_dev;
  h->dev.trace_cap = PQP_TRACE_RECORDS;
  return PQP_OK;
}

// the lines of one traced QP, in the reference's format (dense/solver.hpp:1478-1485 and :1021-1027)
static void
print_trace(const double* slot)
{
  const int64_t n = int64_t(slot[0]);
  for (int64_t k = 1; k <= n; ++k) {
    const double* r = slot + k * 8;
    if (r[0] == 1.0)
      std::printf("\033[1;32m[outer iteration %lld]\033[0m\n| primal residual=%.2e | dual residual=%.2e | duality gap=%.2e | "
                  "mu_in=%.2e | rho=%.2e\n",
                  (long long)r[1], r[2], r[3], r[4], r[5], r[6]);
    else
      std::printf("\033[1;34m[inner iteration %lld]\033[0m\n| inner residual=%.2e | alpha=%.2e\n", (long long)r[1], r[2], r[3]);
  }
  if (slot[1] > 0)
    std::printf("(%lld more iteration lines not recorded: the trace holds %d)\n", (long long)slot[1], PQP_TRACE_RECORDS - 1);
}

// settings.verbose (reference dense/utils.hpp:33-131 header, dense/solver.hpp:1789-1830 statistics): the
// whole solve of a QP runs inside one kernel, which records the per-iteration lines of the reference's report
// (pqp::Batch::trace); the header, those lines and the final statistics block are printed here once the launch has
// finished, one block per verbose QP, in index order.
static int
verbose_report(pqp_batch* h, const int64_t* idx, int64_t first, int64_t count)
{
  bool any = false;
  for (int64_t i = 0; i < count && !any; ++i)
    any = h->settings[size_t(idx ? idx[i] : first + i)].verbose != 0;
  if (!any)
    return PQP_OK;
  if (h->dev.trace) {
    int nv = 0;
    for (int s : h->trace_slot)
      nv = std::max(nv, s + 1);
    h->trace_host.resize(size_t(nv) * PQP_TRACE_RECORDS * 8);
    HIP_TRY(hipMemcpy(h->trace_host.data(), h->trace_dev, h->trace_host.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  const pqp::Dims& d = h->dev.d;
  static const char* const status_name[] = { "Solved", "Maximum number of iterations reached", "Primal infeasible",
                                             "Solved closest primal feasible", "Dual infeasible", "Solver not run" };
  for (int64_t i = 0; i < count; ++i) {
    const int64_t q = idx ? idx[i] : first + i;
    const pqp_settings& st = h->settings[size_t(q)];
    if (!st.verbose)
      continue;
    pqp_info info;
    HIP_TRY(hipMemcpy(&info, h->dev.info + q, sizeof(info), hipMemcpyDeviceToHost));
    std::printf("-------------------------------------------------------------------------------------------------\n"
                "ProxQP dense backend, batched on MI355X (QP %lld of the batch)\n"
                "problem:  \n          variables n = %d, equality constraints n_eq = %d,\n"
                "          inequality constraints n_in = %d\n"
                "settings: \n          backend = dense,\n          eps_abs = %g eps_rel = %g\n"
                "          eps_prim_inf = %g, eps_dual_inf = %g,\n          rho = %g, mu_eq = %g, mu_in = %g,\n"
                "          max_iter = %lld, max_iter_in = %lld,\n          box constraints: %s, \n"
                "          dense backend: %s, \n          problem type: %s, \n          scaling: %s, \n"
                "          timings: %s, \n",
                (long long)q, d.n, d.n_eq, d.n_in, st.eps_abs, st.eps_rel, st.eps_primal_inf, st.eps_dual_inf, info.rho,
                info.mu_eq, info.mu_in, (long long)st.max_iter, (long long)st.max_iter_in, d.box ? "on" : "off",
                h->backend == PQP_BACKEND_PRIMAL_LDLT ? "PrimalLDLT" : "PrimalDualLDLT",
                d.hessian == PQP_HESSIAN_DENSE
                  ? "Quadratic Program"
                  : (d.hessian == PQP_HESSIAN_ZERO ? "Linear Program" : "Quadratic Program with diagonal Hessian"),
                st.compute_preconditioner ? "on" : "off", st.compute_timings ? "on" : "off");
    if (!h->trace_host.empty() && h->trace_slot[size_t(q)] >= 0)
      print_trace(h->trace_host.data() + size_t(h->trace_slot[size_t(q)]) * PQP_TRACE_RECORDS * 8);
    std::printf("-------------------SOLVER STATISTICS-------------------\n"
                "outer iter:     %lld\ntotal iter:     %lld\nmu updates:     %lld\nrho updates:    %lld\n"
                "objective:      %g\nstatus:         %s\n",
                (long long)info.iter_ext, (long long)info.iter, (long long)info.mu_updates,
                (long long)info.rho_updates, info.objValue,
                (info.status >= 0 && info.status <= 5) ? status_name[info.status] : "?");
    if (st.compute_timings)
      std::printf("run time [\xce\xbcs]:  %g\n", info.solve_time);
    std::printf("--------------------------------------------------------\n");
  }
  std::fflush(stdout);
  return PQP_OK;
}

// Host-side bookkeeping of a finished solve (qp_solve ends with work.is_initialized = true, solver.hpp:1836)
static int
finish_solve(pqp_batch* h)
{
  const int64_t* idx = h->flight_idx.empty() ? nullptr : h->flight_idx.data();
  const int64_t first = h->flight_first, count = h->flight_count;
  for (int64_t i = 0; i < count; ++i) {
    const size_t q = size_t(idx ? idx[i] : first + i);
    h->is_initialized[q] = 1;
    if (h->host_results)
      h->mirror_fresh[q] = 1; // the epilogue of the solve wrote the mirror of this QP
  }
  return verbose_report(h, idx, first, count);
}

// one launch of the solve kernel over a range or a subset; `async`: return once it is enqueued
static int
solve_impl(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, bool async)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (int rc = settle(h))
    return rc;
  std::vector<int> order;
  if (idx) {
    if (count < 0 || count > h->dev.B)
      return fail(PQP_ERR_INVALID_ARGUMENT, "subset larger than the batch");
    if (count == 0)
      return PQP_OK;
    order.resize(static_cast<size_t>(count));
    std::vector<char> seen(static_cast<size_t>(h->dev.B), 0);
    for (int64_t i = 0; i < count; ++i) {
      if (idx[i] < 0 || idx[i] >= h->dev.B)
        return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
      if (seen[size_t(idx[i])]) // two workgroups on one QP would race on its x / y / z / state / factors
        return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_solve_subset: a QP index is listed twice");
      seen[size_t(idx[i])] = 1;
      order[size_t(i)] = int(idx[i]);
    }
  } else {
    if (first < 0 || count < 0 || first + count > h->dev.B)
      return fail(PQP_ERR_INVALID_ARGUMENT, "solve range [" + std::to_string(first) + ", " +
                                              std::to_string(first + count) + ") outside the batch of " +
                                              std::to_string(h->dev.B) + " QPs");
    if (count == 0)
      return PQP_OK;
  }
  PQP_ON_DEVICE(h->device);
  if (int rc = pqp_batch_flush(h))
    return rc;
  if (int rc = upload_settings(h))
    return rc;
  if (int rc = prepare_trace(h, idx, first, count))
    return rc;
  int rc = 0;
  if (idx) {
    // the dispatch-order array doubles as the subset list (a learned order is dropped)
    HIP_TRY(hipMemcpy(h->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    h->order_valid = false;
    h->range_first = 0;
    h->range_count = long(count);
    h->subset_order = h->d_order;
    h->subset_host = &order;
    rc = pqp_launch_solve(h);
    h->subset_order = nullptr;
    h->subset_host = nullptr;
    h->flight_idx.assign(idx, idx + count);
  } else {
    h->range_first = first;
    h->range_count = count;
    rc = pqp_launch_solve(h);
    h->flight_idx.clear();
    if (!rc && h->lpt && first == 0 && count == h->dev.B && count > 1) {
      // feedback for the next whole-batch launch: order by the device cycles this solve took (same stream: ordered
      // behind the solve, in front of the next launch)
      rc = pqp_launch_order(h, long(count));
      h->order_valid = rc == 0;
    }
  }
  if (rc)
    return rc;
  h->flight_first = long(first);
  h->flight_count = long(count);
  h->solve_in_flight = true;
  return async ? PQP_OK : pqp_batch_wait(h);
}

int
pqp_batch_wait(pqp_batch* h)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (!h->solve_in_flight)
    return PQP_OK;
  PQP_ON_DEVICE(h->device);
  h->solve_in_flight = false;
  HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  h->last_prologue_ms = 0.f;
  if (h->prologue_timed)
    HIP_TRY(hipEventElapsedTime(&h->last_prologue_ms, h->ev0, h->ev_mid));
  return finish_solve(h);
}

int
pqp_batch_solve_range(pqp_batch* h, int64_t first, int64_t count)
{
  return solve_impl(h, first, count, nullptr, false);
}

int
pqp_batch_solve_subset(pqp_batch* h, const int64_t* idx, int64_t count)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  if (count == 0)
    return PQP_OK;
  return solve_impl(h, 0, count, idx, false);
}

int
pqp_batch_solve_async(pqp_batch* h)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  return solve_impl(h, 0, h->dev.B, nullptr, true);
}

int
pqp_batch_solve_range_async(pqp_batch* h, int64_t first, int64_t count)
{
  return solve_impl(h, first, count, nullptr, true);
}

int
pqp_batch_solve_subset_async(pqp_batch* h, const int64_t* idx, int64_t count)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  if (count == 0)
    return PQP_OK;
  return solve_impl(h, 0, count, idx, true);
}

// Host-resident results: pinned, device-mapped mirrors of (x, y, z, se, si, Info) that the solve kernel's epilogue
// writes beside the device arrays (pqp::Batch::hx ...).
int
pqp_batch_enable_host_results(pqp_batch* h, int enable)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (int rc = settle(h))
    return rc;
  if ((enable != 0) == h->host_results)
    return PQP_OK;
  PQP_ON_DEVICE(h->device);
  pqp::Batch& D = h->dev;
  if (!enable) {
    for (void* p : h->host_allocs)
      (void)hipHostFree(p);
    h->host_allocs.clear();
    D.hx = D.hy = D.hz = D.hse = D.hsi = nullptr;
    D.hinfo = nullptr;
    h->m_x = h->m_y = h->m_z = h->m_se = h->m_si = nullptr;
    h->m_info = nullptr;
    h->host_results = false;
    return PQP_OK;
  }
  const pqp::Dims& d = D.d;
  const size_t B = size_t(D.B);
  auto halloc = [&](size_t bytes, void** host, void** dev) -> int {
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocMapped));
    h->host_allocs.push_back(p);
    std::memset(p, 0, bytes ? bytes : 8);
    void* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, p, 0));
    *host = p;
    *dev = dp;
    return PQP_OK;
  };
  int rc = 0;
  if ((rc = halloc(B * size_t(d.n) * 8, (void**)&h->m_x, (void**)&D.hx)) ||
      (rc = halloc(B * size_t(d.n_eq) * 8, (void**)&h->m_y, (void**)&D.hy)) ||
      (rc = halloc(B * size_t(d.nc) * 8, (void**)&h->m_z, (void**)&D.hz)) ||
      (rc = halloc(B * size_t(d.n_eq) * 8, (void**)&h->m_se, (void**)&D.hse)) ||
      (rc = halloc(B * size_t(d.nc) * 8, (void**)&h->m_si, (void**)&D.hsi)) ||
      (rc = halloc(B * sizeof(pqp_info), (void**)&h->m_info, (void**)&D.hinfo))) {
    for (void* p : h->host_allocs)
      (void)hipHostFree(p);
    h->host_allocs.clear();
    D.hx = D.hy = D.hz = D.hse = D.hsi = nullptr;
    D.hinfo = nullptr;
    return rc;
  }
  h->mirror_fresh.assign(B, 0);
  h->host_results = true;
  return PQP_OK;
}

int
pqp_batch_host_results(pqp_batch* h, const double** x, const double** y, const double** z, const double** se,
                       const double** si, const pqp_info** info)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (!h->host_results)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_enable_host_results has not been called on this batch");
  if (int rc = settle(h))
    return rc;
  if (x)
    *x = h->m_x;
  if (y)
    *y = h->m_y;
  if (z)
    *z = h->m_z;
  if (se)
    *se = h->m_se;
  if (si)
    *si = h->m_si;
  if (info)
    *info = h->m_info;
  return PQP_OK;
}

int
pqp_batch_host_results_fresh(pqp_batch* h, int64_t idx)
{
  if (!h || !h->host_results || idx < -1 || idx >= h->dev.B)
    return 0;
  if (settle(h))
    return 0;
  if (idx >= 0)
    return h->mirror_fresh[size_t(idx)] ? 1 : 0;
  for (char c : h->mirror_fresh)
    if (!c)
      return 0;
  return 1;
}

int
pqp_batch_host_results_fresh_range(pqp_batch* h, int64_t first, int64_t count)
{
  if (!h || !h->host_results || first < 0 || count < 0 || first + count > h->dev.B)
    return 0;
  if (settle(h))
    return 0;
  for (int64_t q = first; q < first + count; ++q)
    if (!h->mirror_fresh[size_t(q)])
      return 0;
  return 1;
}

int
pqp_batch_copy_qp(pqp_batch* dst, int64_t dst_idx, pqp_batch* src, int64_t src_idx)
{
  if (!dst || !src)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (dst_idx < 0 || dst_idx >= dst->dev.B || src_idx < 0 || src_idx >= src->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
  const pqp::Dims &a = dst->dev.d, &b = src->dev.d;
  if (a.n != b.n || a.n_eq != b.n_eq || a.n_in != b.n_in || a.box != b.box || a.hessian != b.hessian ||
      dst->per_qp.size() != src->per_qp.size())
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_copy_qp: the two batches hold QPs of different shapes");
  if (int rc = settle(src))
    return rc;
  if (int rc = settle(dst))
    return rc;
  mirror_stale(dst, dst_idx);
  PQP_ON_DEVICE(src->device);
  if (int rc = pqp_batch_flush(src))
    return rc;
  if (int rc = pqp_batch_flush(dst))
    return rc;
  for (size_t k = 0; k < src->per_qp.size(); ++k) {
    const size_t nb = src->per_qp[k].bytes_per_qp;
    if (nb != dst->per_qp[k].bytes_per_qp)
      return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_copy_qp: layout mismatch");
    HIP_TRY(hipMemcpy(dst->per_qp[k].base + size_t(dst_idx) * nb, src->per_qp[k].base + size_t(src_idx) * nb, nb,
                      hipMemcpyDefault));
  }
  dst->settings[size_t(dst_idx)] = src->settings[size_t(src_idx)];
  dst->is_initialized[size_t(dst_idx)] = src->is_initialized[size_t(src_idx)];
  dst->c_diag[size_t(dst_idx)] = src->c_diag[size_t(src_idx)];
  dst->settings_dirty = true;
  dst->settings_uploaded.clear(); // (d_settings was overwritten by the array copy: force a re-upload)
  return PQP_OK;
}

// What every backward entry checks before it touches the device, in this order: the handle, the subset list (`order`
// receives it) or the range, box constraints, the loss derivatives (`ld_required` false: the tangent entries, which have none).
static int
backward_check(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, const double* loss_derivatives,
               std::vector<int>& order, bool ld_required = true)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (idx) {
    if (count < 0 || count > h->dev.B)
      return fail(PQP_ERR_INVALID_ARGUMENT, "subset larger than the batch");
    order.resize(size_t(count));
    std::vector<char> seen(size_t(h->dev.B), 0);
    for (int64_t i = 0; i < count; ++i) {
      if (idx[i] < 0 || idx[i] >= h->dev.B)
        return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
      if (seen[size_t(idx[i])])
        return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward_subset: a QP index is listed twice");
      seen[size_t(idx[i])] = 1;
      order[size_t(i)] = int(idx[i]);
    }
  } else if (first < 0 || count < 0 || first + count > h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "backward range outside the batch");
  if (h->dev.d.box)
    return fail(PQP_ERR_UNSUPPORTED, "compute_backward is defined for QPs without box constraints "
                                     "(reference dense/compute_ECJ.hpp ignores them)");
  if (ld_required && !loss_derivatives)
    return fail(PQP_ERR_INVALID_ARGUMENT, "loss_derivatives is required");
  return PQP_OK;
}

// ... and once the handle is settled and its device current: queued commands run, and no QP of the launch may be dual
// infeasible -- the reference throws for one (compute_ECJ.hpp:37-45)
static int
backward_ready(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx)
{
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const size_t B = size_t(h->dev.B);
  std::vector<pqp_info> info;
  if (idx) {
    std::vector<pqp_info> all(B);
    HIP_TRY(hipMemcpy(all.data(), h->dev.info, B * sizeof(pqp_info), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; ++i)
      info.push_back(all[size_t(idx[i])]);
  } else {
    info.resize(size_t(count));
    HIP_TRY(hipMemcpy(info.data(), h->dev.info + first, size_t(count) * sizeof(pqp_info), hipMemcpyDeviceToHost));
  }
  for (int64_t i = 0; i < count; ++i)
    if (info[size_t(i)].status == PQP_DUAL_INFEASIBLE)
      return fail(PQP_ERR_INVALID_ARGUMENT,
                  "the QP problem is not feasible, so computing the derivatives is not valid in this setting. "
                  "Try enabling infeasible solving if the problem is only primally infeasible.");
  return PQP_OK;
}

// the arrays pqp_batch_get_backward serves ([B][...], allocated at the first backward call of the handle)
static int
backward_arrays(pqp_batch* h)
{
  if (h->bw_dH)
    return PQP_OK;
  const pqp::Dims& d = h->dev.d;
  const size_t B = size_t(h->dev.B), n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  int rc = 0;
  if ((rc = dalloc(h, &h->bw_dH, B * n * n)) || (rc = dalloc(h, &h->bw_dg, B * n)) ||
      (rc = dalloc(h, &h->bw_dA, B * ne * n)) || (rc = dalloc(h, &h->bw_db, B * ne)) ||
      (rc = dalloc(h, &h->bw_dC, B * ni * n)) || (rc = dalloc(h, &h->bw_du, B * ni)) ||
      (rc = dalloc(h, &h->bw_dl, B * ni)) || (rc = dalloc(h, &h->bw_ld, B * (n + ne + ni))))
    return rc;
  return PQP_OK;
}

static int
backward_impl(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, const double* loss_derivatives,
              double eps, double rho_backward, double mu_backward)
{
  std::vector<int> order;
  if (int rc = backward_check(h, first, count, idx, loss_derivatives, order))
    return rc;
  if (count == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = backward_ready(h, first, count, idx))
    return rc;
  const pqp::Dims& d = h->dev.d;
  const size_t B = size_t(h->dev.B), n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  const size_t ntot = n + ne + ni;
  if (int rc = backward_arrays(h))
    return rc;
  HIP_TRY(hipMemcpy(h->bw_ld, loss_derivatives, size_t(count) * ntot * sizeof(double), hipMemcpyDefault));
  if (int rc = upload_settings(h))
    return rc;
  pqp::BackwardArgs bw{};
  bw.ld = h->bw_ld;
  bw.eps = eps;
  bw.rho_new = rho_backward;
  bw.mu_new = mu_backward;
  bw.dL_dH = h->bw_dH;
  bw.dL_dg = h->bw_dg;
  bw.dL_dA = h->bw_dA;
  bw.dL_db = h->bw_db;
  bw.dL_dC = h->bw_dC;
  bw.dL_du = h->bw_du;
  bw.dL_dl = h->bw_dl;
  bw.first = long(first);
  bw.order = nullptr;
  if (idx) {
    // (the dispatch-order array doubles as the subset list: a learned order is dropped)
    HIP_TRY(hipMemcpy(h->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    h->order_valid = false;
    bw.order = h->d_order;
  }
  int rc;
  if (h->vec_scratch) {
    // per-QP vectors in HBM: the K-row kernel's HBM form with one row per QP, then the seven jacobians from that row
    if ((rc = grow(h, &h->bwm_out, &h->bwm_out_cap, size_t(count) * ntot)) ||
        (rc = grow(h, &h->bwm_active, &h->bwm_active_cap, size_t(count) * ni)))
      return rc;
    pqp::BackwardMultiArgs m{};
    m.ld = h->bw_ld;
    m.eps = eps;
    m.rho_new = rho_backward;
    m.mu_new = mu_backward;
    m.out = h->bwm_out;
    m.active = h->bwm_active;
    m.n_rhs = 1;
    m.first = bw.first;
    m.order = bw.order;
    if ((rc = pqp_launch_backward_multi_hbm(h, m, long(count))) ||
        (rc = pqp_launch_backward_outer(h, bw, h->bwm_out, h->bwm_active, long(count))))
      return rc;
  } else if ((rc = pqp_launch_backward(h, bw, long(count))))
    return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PQP_OK;
}

static int
backward_multi_impl(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, int64_t n_rhs,
                    const double* loss_derivatives, double eps, double rho_backward, double mu_backward, double* out,
                    int32_t* active)
{
  std::vector<int> order;
  if (int rc = backward_check(h, first, count, idx, loss_derivatives, order))
    return rc;
  if (!out)
    return fail(PQP_ERR_INVALID_ARGUMENT, "out is required");
  if (n_rhs < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "n_rhs is negative");
  const pqp::Dims& d = h->dev.d;
  const size_t ni = size_t(d.n_in), ntot = size_t(d.n) + size_t(d.n_eq) + ni;
  // count * n_rhs * ntot doubles must be addressable
  const size_t lim = std::numeric_limits<int64_t>::max() / sizeof(double);
  if (count > 0 && n_rhs > 0 && ntot > 0 && (size_t(n_rhs) > lim / size_t(count) || size_t(count) * size_t(n_rhs) > lim / ntot))
    return fail(PQP_ERR_INVALID_ARGUMENT, "count * n_rhs * (dim + n_eq + n_in) overflows");
  if (count == 0 || n_rhs == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = backward_ready(h, first, count, idx))
    return rc;
  const size_t total = size_t(count) * size_t(n_rhs) * ntot, nflags = size_t(count) * ni;
  // host arrays are staged through buffers of the handle; device (or pinned / managed) memory is used in place
  const bool ld_in_place = pqp_device_readable(loss_derivatives), out_in_place = pqp_device_readable(out);
  const bool active_in_place = !active || pqp_device_readable(active);
  int rc = 0;
  if (!ld_in_place) {
    if ((rc = grow(h, &h->bwm_ld, &h->bwm_ld_cap, total)))
      return rc;
    HIP_TRY(hipMemcpy(h->bwm_ld, loss_derivatives, total * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!out_in_place && (rc = grow(h, &h->bwm_out, &h->bwm_out_cap, total)))
    return rc;
  if (!active_in_place && (rc = grow(h, &h->bwm_active, &h->bwm_active_cap, nflags)))
    return rc;
  if ((rc = upload_settings(h)))
    return rc;
  pqp::BackwardMultiArgs m{};
  m.ld = ld_in_place ? loss_derivatives : h->bwm_ld;
  m.eps = eps;
  m.rho_new = rho_backward;
  m.mu_new = mu_backward;
  m.out = out_in_place ? out : h->bwm_out;
  m.active = active ? (active_in_place ? reinterpret_cast<int*>(active) : h->bwm_active) : nullptr;
  m.n_rhs = long(n_rhs);
  m.first = long(first);
  m.order = nullptr;
  if (idx) {
    HIP_TRY(hipMemcpy(h->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    h->order_valid = false;
    m.order = h->d_order;
  }
  // (the epilogue rewrites Info of every QP of the launch: a host mirror of it no longer holds what the device holds)
  for (int64_t i = 0; i < count; ++i)
    mirror_stale(h, idx ? idx[i] : first + i);
  if ((rc = h->vec_scratch ? pqp_launch_backward_multi_hbm(h, m, long(count)) : pqp_launch_backward_multi(h, m, long(count))))
    return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (!out_in_place)
    HIP_TRY(hipMemcpy(out, h->bwm_out, total * sizeof(double), hipMemcpyDeviceToHost));
  if (!active_in_place && nflags)
    HIP_TRY(hipMemcpy(active, h->bwm_active, nflags * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PQP_OK;
}

int
pqp_batch_backward_multi(pqp_batch* h, int64_t first, int64_t count, int64_t n_rhs, const double* loss_derivatives,
                         double eps, double rho_backward, double mu_backward, double* out, int32_t* active)
{
  return backward_multi_impl(h, first, count, nullptr, n_rhs, loss_derivatives, eps, rho_backward, mu_backward, out, active);
}

int
pqp_batch_backward_multi_subset(pqp_batch* h, const int64_t* idx, int64_t count, int64_t n_rhs,
                                const double* loss_derivatives, double eps, double rho_backward, double mu_backward,
                                double* out, int32_t* active)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  return backward_multi_impl(h, 0, count, idx, n_rhs, loss_derivatives, eps, rho_backward, mu_backward, out, active);
}

// pqp_batch_tangent_multi / _subset: the checks, the staging and the state rules of backward_multi_impl; two launches
// (the right-hand sides R from the tangent arrays, then the K-tangent solve) on the handle's stream
static int
tangent_multi_impl(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, int64_t n_dir, const double* dH,
                   const double* dg, const double* dA, const double* db, const double* dC, const double* dl,
                   const double* du, int shared_mask, double eps, double rho, double mu, double* out, int32_t* active,
                   double* rhs)
{
  std::vector<int> order;
  if (int rc = backward_check(h, first, count, idx, nullptr, order, false))
    return rc;
  if (!out)
    return fail(PQP_ERR_INVALID_ARGUMENT, "out is required");
  if (n_dir < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "n_dir is negative");
  const pqp::Dims& d = h->dev.d;
  const size_t n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in), ntot = n + ne + ni;
  // count * n_dir * (the largest tangent array of one QP and direction) doubles must be addressable, and the assembly
  // kernel runs one workgroup per (QP, direction)
  const size_t widest = std::max(ntot, n * std::max(n, std::max(ne, ni)));
  const size_t lim = std::numeric_limits<int64_t>::max() / sizeof(double);
  if (count > 0 && n_dir > 0 &&
      (size_t(n_dir) > lim / size_t(count) || size_t(count) * size_t(n_dir) > lim / widest ||
       size_t(count) * size_t(n_dir) > size_t(std::numeric_limits<int>::max())))
    return fail(PQP_ERR_INVALID_ARGUMENT, "count * n_dir * (size of a tangent) overflows");
  if (count == 0 || n_dir == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = backward_ready(h, first, count, idx))
    return rc;
  const size_t K = size_t(n_dir), total = size_t(count) * K * ntot, nflags = size_t(count) * ni;
  // host arrays are staged through buffers of the handle (the tangents packed one behind the other in tg_stage); device
  // (or pinned / managed) memory is used in place
  const double* src[7] = { dH, dg, dA, db, dC, dl, du };
  const size_t per_dir[7] = { n * n, n, ne * n, ne, ni * n, ni, ni };
  static const int bit[7] = { PQP_SHARED_H, PQP_SHARED_G, PQP_SHARED_A, PQP_SHARED_B, PQP_SHARED_C, PQP_SHARED_L, PQP_SHARED_U };
  size_t len[7], off[7], staged = 0;
  bool in_place[7];
  for (int t = 0; t < 7; ++t) {
    len[t] = ((shared_mask & bit[t]) ? size_t(1) : size_t(count)) * K * per_dir[t];
    if (len[t] == 0)
      src[t] = nullptr; // (an array of no elements is a zero tangent)
    in_place[t] = !src[t] || pqp_device_readable(src[t]);
    off[t] = staged;
    if (!in_place[t])
      staged += len[t];
  }
  const bool out_in_place = pqp_device_readable(out), rhs_in_place = rhs && pqp_device_readable(rhs);
  const bool active_in_place = !active || pqp_device_readable(active);
  int rc = 0;
  if (staged && (rc = grow(h, &h->tg_stage, &h->tg_stage_cap, staged)))
    return rc;
  const double* dev[7];
  for (int t = 0; t < 7; ++t) {
    dev[t] = src[t];
    if (!in_place[t]) {
      HIP_TRY(hipMemcpy(h->tg_stage + off[t], src[t], len[t] * sizeof(double), hipMemcpyHostToDevice));
      dev[t] = h->tg_stage + off[t];
    }
  }
  if (!rhs_in_place && (rc = grow(h, &h->tg_rhs, &h->tg_rhs_cap, total)))
    return rc;
  if (!out_in_place && (rc = grow(h, &h->bwm_out, &h->bwm_out_cap, total)))
    return rc;
  if (!active_in_place && (rc = grow(h, &h->bwm_active, &h->bwm_active_cap, nflags)))
    return rc;
  if ((rc = upload_settings(h)))
    return rc;
  pqp::TangentRhsArgs a{};
  a.dH = dev[0];
  a.dg = dev[1];
  a.dA = dev[2];
  a.db = dev[3];
  a.dC = dev[4];
  a.shared_mask = shared_mask;
  a.R = rhs_in_place ? rhs : h->tg_rhs;
  a.n_dir = long(n_dir);
  a.first = long(first);
  a.order = nullptr;
  pqp::TangentArgs m{};
  m.R = a.R;
  m.dl = dev[5];
  m.du = dev[6];
  m.dl_stride = (shared_mask & PQP_SHARED_L) ? 0 : long(K * ni);
  m.du_stride = (shared_mask & PQP_SHARED_U) ? 0 : long(K * ni);
  m.eps = eps;
  m.rho_new = rho;
  m.mu_new = mu;
  m.out = out_in_place ? out : h->bwm_out;
  m.active = active ? (active_in_place ? reinterpret_cast<int*>(active) : h->bwm_active) : nullptr;
  m.n_dir = long(n_dir);
  m.first = long(first);
  m.order = nullptr;
  if (idx) {
    HIP_TRY(hipMemcpy(h->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    h->order_valid = false;
    a.order = m.order = h->d_order;
  }
  // (the epilogue rewrites Info of every QP of the launch: a host mirror of it no longer holds what the device holds)
  for (int64_t i = 0; i < count; ++i)
    mirror_stale(h, idx ? idx[i] : first + i);
  if ((rc = pqp_launch_tangent_rhs(h, a, long(count))))
    return rc;
  if ((rc = h->vec_scratch ? pqp_launch_tangent_multi_hbm(h, m, long(count)) : pqp_launch_tangent_multi(h, m, long(count))))
    return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (!out_in_place)
    HIP_TRY(hipMemcpy(out, h->bwm_out, total * sizeof(double), hipMemcpyDeviceToHost));
  if (rhs && !rhs_in_place)
    HIP_TRY(hipMemcpy(rhs, h->tg_rhs, total * sizeof(double), hipMemcpyDeviceToHost));
  if (!active_in_place && nflags)
    HIP_TRY(hipMemcpy(active, h->bwm_active, nflags * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PQP_OK;
}

int
pqp_batch_tangent_multi(pqp_batch* h, int64_t first, int64_t count, int64_t n_dir, const double* dH, const double* dg,
                        const double* dA, const double* db, const double* dC, const double* dl, const double* du,
                        int shared_mask, double eps, double rho, double mu, double* out, int32_t* active, double* rhs)
{
  return tangent_multi_impl(h, first, count, nullptr, n_dir, dH, dg, dA, db, dC, dl, du, shared_mask, eps, rho, mu, out, active,
                            rhs);
}

int
pqp_batch_tangent_multi_subset(pqp_batch* h, const int64_t* idx, int64_t count, int64_t n_dir, const double* dH,
                               const double* dg, const double* dA, const double* db, const double* dC, const double* dl,
                               const double* du, int shared_mask, double eps, double rho, double mu, double* out,
                               int32_t* active, double* rhs)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  return tangent_multi_impl(h, 0, count, idx, n_dir, dH, dg, dA, db, dC, dl, du, shared_mask, eps, rho, mu, out, active, rhs);
}

// pqp_batch_backward_box / _subset: backward_multi_impl for a box handle, rows and flags over the n_in + n rows of [C; I];
// n_rhs == 1 also forms the nine jacobians from the row
static int
backward_box_impl(pqp_batch* h, int64_t first, int64_t count, const int64_t* idx, int64_t n_rhs,
                  const double* loss_derivatives, double eps, double rho_backward, double mu_backward, double* out,
                  int32_t* active)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (!h->dev.d.box)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward_box is defined for handles created with box_constraints: "
                                          "pqp_batch_backward, pqp_batch_backward_range / _subset and "
                                          "pqp_batch_backward_multi / _multi_subset serve this one");
  std::vector<int> order;
  if (idx) {
    if (count < 0 || count > h->dev.B)
      return fail(PQP_ERR_INVALID_ARGUMENT, "subset larger than the batch");
    order.resize(size_t(count));
    std::vector<char> seen(size_t(h->dev.B), 0);
    for (int64_t i = 0; i < count; ++i) {
      if (idx[i] < 0 || idx[i] >= h->dev.B)
        return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
      if (seen[size_t(idx[i])])
        return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward_box_subset: a QP index is listed twice");
      seen[size_t(idx[i])] = 1;
      order[size_t(i)] = int(idx[i]);
    }
  } else if (first < 0 || count < 0 || first + count > h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "backward range outside the batch");
  if (!loss_derivatives)
    return fail(PQP_ERR_INVALID_ARGUMENT, "loss_derivatives is required");
  if (n_rhs < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "n_rhs is negative");
  const pqp::Dims& d = h->dev.d;
  const size_t nc = size_t(d.nc), ntot = size_t(d.n) + size_t(d.n_eq) + nc;
  const size_t lim = std::numeric_limits<int64_t>::max() / sizeof(double);
  if (count > 0 && n_rhs > 0 && (size_t(n_rhs) > lim / size_t(count) || size_t(count) * size_t(n_rhs) > lim / ntot))
    return fail(PQP_ERR_INVALID_ARGUMENT, "count * n_rhs * (dim + n_eq + n_in + dim) overflows");
  if (count == 0 || n_rhs == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = backward_ready(h, first, count, idx))
    return rc;
  const size_t total = size_t(count) * size_t(n_rhs) * ntot, nflags = size_t(count) * nc;
  const bool ld_in_place = pqp_device_readable(loss_derivatives), out_in_place = out && pqp_device_readable(out);
  const bool active_in_place = active && pqp_device_readable(active);
  const bool jacobians = n_rhs == 1; // (they are formed from the row and the flags: both are kept then, asked for or not)
  int rc = 0;
  if (!ld_in_place) {
    if ((rc = grow(h, &h->bwm_ld, &h->bwm_ld_cap, total)))
      return rc;
    HIP_TRY(hipMemcpy(h->bwm_ld, loss_derivatives, total * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!out_in_place && (rc = grow(h, &h->bwm_out, &h->bwm_out_cap, total)))
    return rc;
  if (!active_in_place && (active || jacobians) && (rc = grow(h, &h->bwm_active, &h->bwm_active_cap, nflags)))
    return rc;
  if (jacobians) {
    if ((rc = backward_arrays(h)))
      return rc;
    const size_t B = size_t(h->dev.B), n = size_t(d.n);
    if (!h->bw_dlb && ((rc = dalloc(h, &h->bw_dlb, B * n)) || (rc = dalloc(h, &h->bw_dub, B * n))))
      return rc;
  }
  if ((rc = upload_settings(h)))
    return rc;
  pqp::BackwardMultiArgs m{};
  m.ld = ld_in_place ? loss_derivatives : h->bwm_ld;
  m.eps = eps;
  m.rho_new = rho_backward;
  m.mu_new = mu_backward;
  m.out = out_in_place ? out : h->bwm_out;
  m.active = active_in_place ? reinterpret_cast<int*>(active) : ((active || jacobians) ? h->bwm_active : nullptr);
  m.n_rhs = long(n_rhs);
  m.first = long(first);
  m.order = nullptr;
  if (idx) {
    HIP_TRY(hipMemcpy(h->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    h->order_valid = false;
    m.order = h->d_order;
  }
  for (int64_t i = 0; i < count; ++i)
    mirror_stale(h, idx ? idx[i] : first + i);
  if ((rc = h->vec_scratch ? pqp_launch_bwbox_hbm(h, m, long(count)) : pqp_launch_bwbox(h, m, long(count))))
    return rc;
  if (jacobians) {
    pqp::BackwardArgs bw{};
    bw.dL_dH = h->bw_dH;
    bw.dL_dg = h->bw_dg;
    bw.dL_dA = h->bw_dA;
    bw.dL_db = h->bw_db;
    bw.dL_dC = h->bw_dC;
    bw.dL_du = h->bw_du;
    bw.dL_dl = h->bw_dl;
    bw.first = m.first;
    bw.order = m.order;
    if ((rc = pqp_launch_bwbox_outer(h, bw, h->bw_dlb, h->bw_dub, m.out, m.active, long(count))))
      return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out && !out_in_place)
    HIP_TRY(hipMemcpy(out, h->bwm_out, total * sizeof(double), hipMemcpyDeviceToHost));
  if (active && !active_in_place && nflags)
    HIP_TRY(hipMemcpy(active, h->bwm_active, nflags * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PQP_OK;
}

int
pqp_batch_backward_box(pqp_batch* h, int64_t first, int64_t count, int64_t n_rhs, const double* loss_derivatives,
                       double eps, double rho_backward, double mu_backward, double* out, int32_t* active)
{
  return backward_box_impl(h, first, count, nullptr, n_rhs, loss_derivatives, eps, rho_backward, mu_backward, out, active);
}

int
pqp_batch_backward_box_subset(pqp_batch* h, const int64_t* idx, int64_t count, int64_t n_rhs,
                              const double* loss_derivatives, double eps, double rho_backward, double mu_backward,
                              double* out, int32_t* active)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  // (an empty subset has no list to read: it is the empty range)
  return backward_box_impl(h, 0, count, count > 0 ? idx : nullptr, n_rhs, loss_derivatives, eps, rho_backward, mu_backward, out,
                           active);
}

int
pqp_batch_get_backward_box(pqp_batch* h, int64_t idx, double* dL_dl_box, double* dL_du_box)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (!h->bw_dlb)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward_box with n_rhs == 1 has not been called on this batch");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  const size_t n = size_t(h->dev.d.n);
  const int64_t B = h->dev.B;
  int rc = 0;
  if ((rc = copy_out(dL_dl_box, h->bw_dlb, idx, B, n)) || (rc = copy_out(dL_du_box, h->bw_dub, idx, B, n)))
    return rc;
  return PQP_OK;
}

int
pqp_batch_backward_range(pqp_batch* h, int64_t first, int64_t count, const double* loss_derivatives, double eps,
                         double rho_backward, double mu_backward)
{
  return backward_impl(h, first, count, nullptr, loss_derivatives, eps, rho_backward, mu_backward);
}

int
pqp_batch_backward_subset(pqp_batch* h, const int64_t* idx, int64_t count, const double* loss_derivatives, double eps,
                          double rho_backward, double mu_backward)
{
  if (!h || (count > 0 && !idx))
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  return backward_impl(h, 0, count, idx, loss_derivatives, eps, rho_backward, mu_backward);
}

int
pqp_batch_backward(pqp_batch* h, const double* loss_derivatives, double eps, double rho_backward,
                   double mu_backward)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  return pqp_batch_backward_range(h, 0, h->dev.B, loss_derivatives, eps, rho_backward, mu_backward);
}

// bytes of device memory one QP of an inner handle of shape (n, n_eq, 0) takes: the matrices of pqp_batch_create (model,
// equilibrated copies, primal block, Z, Gram and Schur blocks); the vectors are noise beside them
static double
inner_bytes_per_qp(double n, double ne)
{
  return 8.0 * (5.0 * n * n + 3.0 * ne * n + 2.0 * ne * n + 3.0 * ne * ne);
}

int
pqp_batch_backward_closest_feasible(pqp_batch* h, int64_t first, int64_t count, const double* loss_derivatives, double eps,
                                    double rho, int64_t max_iter, int64_t qps_per_pass, double* solution, int32_t* flags)
{
  std::vector<int> order;
  if (int rc = backward_check(h, first, count, nullptr, loss_derivatives, order))
    return rc;
  if (qps_per_pass < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "qps_per_pass is negative");
  if (count == 0)
    return PQP_OK;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (int rc = backward_ready(h, first, count, nullptr))
    return rc;
  const pqp::Dims& d = h->dev.d;
  const size_t ni = size_t(d.n_in);
  const int n_row = pqp::infeas_rows(d.n, d.n_eq, d.n_in), n_col = pqp::infeas_cols(d.n, d.n_eq, d.n_in);
  // QPs per pass: the caller's, else what a byte budget holds (a policy constant, not a measurement: an inner QP of a
  // (100, 50, 200) layer takes ~50 MB of model and factors, 2048 of them at once would take ~100 GB)
  int64_t pass = qps_per_pass;
  if (pass == 0) {
    double budget = 16.0 * 1024.0 * 1024.0 * 1024.0;
    if (const char* e = std::getenv("PQP_INFEAS_BACKWARD_BYTES"))
      budget = std::atof(e);
    const double fit = std::floor(budget / inner_bytes_per_qp(n_col, n_row));
    pass = fit < 1.0 ? 1 : (fit > double(count) ? count : int64_t(fit));
  }
  pass = std::min(pass, count);
  if (h->inner && h->inner->dev.B < pass) {
    pqp_batch_destroy(h->inner);
    h->inner = nullptr;
  }
  if (!h->inner)
    // (a shape beyond the engine's size limits: PQP_ERR_UNSUPPORTED from here)
    if (int rc = pqp_batch_create(pass, n_col, n_row, 0, 0, PQP_HESSIAN_ZERO, PQP_BACKEND_AUTOMATIC, h->device, &h->inner))
      return rc;
  pqp_batch* in = h->inner;
  if (int rc = pqp_batch_set_stream(in, h->stream))
    return rc;
  // the reference's settings of the inner QP (qplayer.py:516-520); everything else at its default
  for (auto& st : in->settings) {
    pqp_settings_default(&st, in->backend);
    st.primal_infeasibility_solving = 1;
    st.eps_abs = eps;
    st.max_iter = max_iter;
    st.default_rho = rho;
    st.refactor_rho_threshold = rho;
  }
  in->settings_dirty = true;
  int rc = 0;
  if ((rc = backward_arrays(h)) || (rc = grow(h, &h->inf_p2c, &h->inf_p2c_cap, size_t(pass) * ni)))
    return rc;
  if (!h->inf_finite_l && (rc = dalloc(h, &h->inf_finite_l, 1)))
    return rc;
  const bool ld_in_place = pqp_device_readable(loss_derivatives);
  const bool flags_in_place = flags && pqp_device_readable(flags);
  if (!ld_in_place) {
    if ((rc = grow(h, &h->inf_ld, &h->inf_ld_cap, size_t(count) * size_t(n_row))))
      return rc;
    HIP_TRY(hipMemcpy(h->inf_ld, loss_derivatives, size_t(count) * size_t(n_row) * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!flags_in_place && (rc = grow(h, &h->inf_flags, &h->inf_flags_cap, size_t(pass) * ni)))
    return rc;
  HIP_TRY(hipMemsetAsync(h->inf_finite_l, 0, sizeof(int), h->stream));
  pqp::BackwardArgs bw{};
  bw.dL_dH = h->bw_dH;
  bw.dL_dg = h->bw_dg;
  bw.dL_dA = h->bw_dA;
  bw.dL_db = h->bw_db;
  bw.dL_dC = h->bw_dC;
  bw.dL_du = h->bw_du;
  bw.dL_dl = h->bw_dl;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t done = 0; done < count; done += pass) {
    const int64_t cnt = std::min(pass, count - done);
    pqp::InfeasArgs a{};
    a.ld = (ld_in_place ? loss_derivatives : h->inf_ld) + size_t(done) * size_t(n_row);
    a.first = long(first + done);
    a.count = long(cnt);
    a.K = in->dev.A;
    a.r = in->dev.b;
    a.w = in->dev.x;
    a.flags = flags_in_place ? reinterpret_cast<int*>(flags) + size_t(done) * ni : h->inf_flags;
    a.p2c = h->inf_p2c;
    a.finite_l = h->inf_finite_l;
    a.check_first = long(first);
    a.check_count = done == 0 ? long(count) : 0;
    if ((rc = settle(in)) || (rc = pqp_launch_infeas_kkt(h, a)))
      return rc;
    if (done == 0) {
      int finite_l = 0;
      HIP_TRY(hipStreamSynchronize(h->stream));
      HIP_TRY(hipMemcpy(&finite_l, h->inf_finite_l, sizeof(int), hipMemcpyDeviceToHost));
      if (finite_l)
        return fail(PQP_ERR_INVALID_ARGUMENT, "the closest-feasible backward is defined for single-sided inequalities: a QP "
                                              "of the range has a lower bound above -1e20");
    }
    // QP::init on the model already in place (H = 0 and g = 0 since the handle was created: no array is given, nothing
    // is copied), then the engine's ordinary set-up and solve
    if (cnt == in->dev.B)
      rc = pqp_batch_init(in, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nan, nan,
                          nan, nan);
    else
      for (int64_t q = 0; q < cnt && !rc; ++q)
        rc = pqp_batch_init(in, q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nan, nan,
                            nan, nan);
    if (rc || (rc = pqp_batch_solve_range(in, 0, cnt)) || (rc = pqp_launch_infeas_grad(h, a, bw)))
      return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (solution)
      HIP_TRY(hipMemcpy(solution + size_t(done) * size_t(n_col), in->dev.x, size_t(cnt) * size_t(n_col) * sizeof(double),
                        hipMemcpyDefault));
    if (flags && !flags_in_place && ni)
      HIP_TRY(hipMemcpy(flags + size_t(done) * ni, h->inf_flags, size_t(cnt) * ni * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return PQP_OK;
}

int
pqp_batch_get_backward(pqp_batch* h, int64_t idx, double* dL_dH, double* dL_dg, double* dL_dA, double* dL_db,
                       double* dL_dC, double* dL_du, double* dL_dl)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (!h->bw_dH)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward has not been called on this batch");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  const pqp::Dims& d = h->dev.d;
  const size_t n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  const int64_t B = h->dev.B;
  int rc = 0;
  if ((rc = copy_out(dL_dH, h->bw_dH, idx, B, n * n)) || (rc = copy_out(dL_dg, h->bw_dg, idx, B, n)) ||
      (rc = copy_out(dL_dA, h->bw_dA, idx, B, ne * n)) || (rc = copy_out(dL_db, h->bw_db, idx, B, ne)) ||
      (rc = copy_out(dL_dC, h->bw_dC, idx, B, ni * n)) || (rc = copy_out(dL_du, h->bw_du, idx, B, ni)) ||
      (rc = copy_out(dL_dl, h->bw_dl, idx, B, ni)))
    return rc;
  return PQP_OK;
}

// The sums over the QPs first .. first + count - 1 of what pqp_batch_get_backward / pqp_batch_get_backward_box hand out per
// QP, in the order of pqp_shared.hpp: every sum is formed in a buffer of the handle and copied to its (host or device)
// destination on the handle's stream.
int
pqp_batch_get_backward_sum(pqp_batch* h, int64_t first, int64_t count, double* dL_dH, double* dL_dg, double* dL_dA,
                           double* dL_db, double* dL_dC, double* dL_du, double* dL_dl, double* dL_dl_box,
                           double* dL_du_box)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (first < 0 || count < 0 || first > h->dev.B || count > h->dev.B - first)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP range outside the batch");
  const pqp::Dims& d = h->dev.d;
  if (!d.box && (dL_dl_box || dL_du_box))
    return fail(PQP_ERR_INVALID_ARGUMENT, "the batch has no box constraints: there is no dL_dl_box / dL_du_box to sum");
  if (!h->bw_dH)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward has not been called on this batch");
  if ((dL_dl_box || dL_du_box) && !h->bw_dlb)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_backward_box with n_rhs == 1 has not been called on this batch");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  const size_t n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  struct Out
  {
    double* dst;
    const double* src;
    size_t len;
  };
  const Out out[9] = { { dL_dH, h->bw_dH, n * n }, { dL_dg, h->bw_dg, n },  { dL_dA, h->bw_dA, ne * n },
                       { dL_db, h->bw_db, ne },    { dL_dC, h->bw_dC, ni * n }, { dL_du, h->bw_du, ni },
                       { dL_dl, h->bw_dl, ni },    { dL_dl_box, h->bw_dlb, n }, { dL_du_box, h->bw_dub, n } };
  // [the sums, side by side][the chunk partials of the array being summed]
  const size_t chunks = (size_t(count) + pqp::PQP_SUM_CHUNK - 1) / pqp::PQP_SUM_CHUNK;
  size_t total = 0, widest = 0;
  for (const Out& o : out)
    if (o.dst) {
      total += o.len;
      widest = std::max(widest, o.len);
    }
  if (total == 0)
    return PQP_OK;
  if (int rc = grow(h, &h->sum_partial, &h->sum_partial_cap, total + (chunks > 1 ? chunks * widest : 0)))
    return rc;
  double *res = h->sum_partial, *partial = h->sum_partial + total;
  for (const Out& o : out) {
    if (!o.dst || o.len == 0)
      continue;
    int rc = 0;
    if (count == 0)
      HIP_TRY(hipMemsetAsync(res, 0, o.len * sizeof(double), h->stream));
    else if (chunks == 1)
      rc = pqp_launch_sum(h, o.src, res, long(o.len), long(first), long(count), pqp::PQP_SUM_CHUNK);
    else if (!(rc = pqp_launch_sum(h, o.src, partial, long(o.len), long(first), long(count), pqp::PQP_SUM_CHUNK)))
      rc = pqp_launch_sum(h, partial, res, long(o.len), 0, long(chunks), long(chunks));
    if (rc)
      return rc;
    HIP_TRY(hipMemcpyAsync(o.dst, res, o.len * sizeof(double), hipMemcpyDefault, h->stream));
    res += o.len;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PQP_OK;
}

int
pqp_batch_get_results(pqp_batch* h, int64_t idx, double* x, double* y, double* z, double* se, double* si,
                      pqp_info* info)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const pqp::Dims& d = h->dev.d;
  const pqp::Batch& D = h->dev;
  // the host mirrors serve the call when they hold what the device holds (no device-to-host copy)
  const bool mirrored = pqp_batch_host_results_fresh(h, idx) != 0;
  const double *sx = mirrored ? h->m_x : D.x, *sy = mirrored ? h->m_y : D.y, *sz = mirrored ? h->m_z : D.z,
               *sse = mirrored ? h->m_se : D.se, *ssi = mirrored ? h->m_si : D.si;
  const pqp_info* sinfo = mirrored ? h->m_info : D.info;
  int rc = 0;
  if ((rc = copy_out(x, sx, idx, D.B, size_t(d.n))) || (rc = copy_out(y, sy, idx, D.B, size_t(d.n_eq))) ||
      (rc = copy_out(z, sz, idx, D.B, size_t(d.nc))) || (rc = copy_out(se, sse, idx, D.B, size_t(d.n_eq))) ||
      (rc = copy_out(si, ssi, idx, D.B, size_t(d.nc))))
    return rc;
  if (info) {
    if (idx < 0)
      HIP_TRY(hipMemcpy(info, sinfo, size_t(D.B) * sizeof(pqp_info), hipMemcpyDefault));
    else
      HIP_TRY(hipMemcpy(info, sinfo + idx, sizeof(pqp_info), hipMemcpyDefault));
  }
  return PQP_OK;
}

int
pqp_batch_result_device_ptrs(pqp_batch* h, double** x, double** y, double** z)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  if (x)
    *x = h->dev.x;
  if (y)
    *y = h->dev.y;
  if (z)
    *z = h->dev.z;
  return PQP_OK;
}

int
pqp_batch_pack_results(pqp_batch* h, int64_t first, int64_t count, double* out, void* stream)
{
  if (!h || !out)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  if (first < 0 || count < 0 || first + count > h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pack range outside the batch");
  if (count == 0)
    return PQP_OK;
  // (on the launch stream of a solve in flight the pack kernel is ordered behind it: no host wait)
  if (static_cast<hipStream_t>(stream) != h->stream || h->cmd_pending)
    if (int rc = settle(h))
      return rc;
  PQP_ON_DEVICE(h->device);
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  return pqp_launch_pack(h, long(first), long(count), out, static_cast<hipStream_t>(stream));
}

int
pqp_batch_get_scaled(pqp_batch* h, int64_t idx, double* H, double* g, double* A, double* b, double* C,
                     double* l, double* u, double* delta, double* c)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (idx < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_get_scaled addresses one QP");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  if (h->cmd_pending)
    if (int rc = pqp_batch_flush(h))
      return rc;
  const pqp::Dims& d = h->dev.d;
  const pqp::Batch& D = h->dev;
  const size_t n = size_t(d.n), ne = size_t(d.n_eq), ni = size_t(d.n_in);
  int rc = 0;
  if ((rc = copy_out(H, D.Hs, idx, D.B, n * n)) || (rc = copy_out(g, D.gs, idx, D.B, n)) ||
      (rc = copy_out(A, D.As, idx, D.B, ne * n)) || (rc = copy_out(b, D.bs, idx, D.B, ne)) ||
      (rc = copy_out(C, D.Cs, idx, D.B, ni * n)) || (rc = copy_out(l, D.ls, idx, D.B, ni)) ||
      (rc = copy_out(u, D.us, idx, D.B, ni)) || (rc = copy_out(delta, D.delta, idx, D.B, size_t(d.ntot))))
    return rc;
  if (c) {
    pqp::State s;
    HIP_TRY(hipMemcpy(&s, D.state + idx, sizeof(s), hipMemcpyDefault));
    *c = s.ruiz_c;
  }
  return PQP_OK;
}

// Diagnostic: the dual Schur block of QP `idx` as the last solve left it in HBM (DenseBackend::PrimalDualLDLT):
// inverse factor W_S (nd x nd, row-major, lower, unit diagonal), D_S (nd), the Gram cache G (nd x nd, by
// constraint id: equality a -> a, inequality i -> n_eq + i), the slot list (nc ints: constraint id of the
// inequality slot j, -1 for a hole) and meta = {n_slots, n_c, ls_valid, ls_edited}, mus = {mu_eq, mu_in} the
// factor was built for.  The identity W_S (M_J + G_JJ) W_S^T = D_S can then be checked on the host
// (tests: accuracy of the rank-1 row appends / deletions on the real device).
int
pqp_batch_get_schur_factor(pqp_batch* h, int64_t idx, double* WS, double* dS, double* G, int32_t* slots,
                           int64_t* meta, double* mus)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (idx < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_get_schur_factor addresses one QP");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  const pqp::Dims& d = h->dev.d;
  const pqp::Batch& D = h->dev;
  const size_t nd = size_t(d.nd), nc = size_t(d.nc);
  int rc = 0;
  if ((rc = copy_out(WS, D.WS, idx, D.B, nd * nd)) || (rc = copy_out(dS, D.dS, idx, D.B, nd)) ||
      (rc = copy_out(G, D.G, idx, D.B, nd * nd)))
    return rc;
  if (slots && nc) {
    std::vector<int> raw(nc);
    HIP_TRY(hipMemcpy(raw.data(), D.act + size_t(idx) * nc, nc * sizeof(int), hipMemcpyDefault));
    for (size_t j = 0; j < nc; ++j)
      slots[j] = pqp::act_cid(raw[j]); // (bits 16-17 carry the persistent up / low flags)
  }
  pqp::State s;
  HIP_TRY(hipMemcpy(&s, D.state + idx, sizeof(s), hipMemcpyDefault));
  if (meta) {
    meta[0] = s.n_slots;
    meta[1] = s.n_c;
    meta[2] = s.ls_valid;
    meta[3] = s.ls_edited;
  }
  if (mus) {
    mus[0] = s.mu_eq_fact;
    mus[1] = s.mu_in_fact;
  }
  return PQP_OK;
}

// Diagnostic: the primal block of QP `idx` as the last solve left it in HBM (layouts: include/proxqp_hip.h).  The
// tests judge every stage of setup_factorization against its own inputs: the LDL^T of H_s + rho I, the explicit
// inverse W = L^{-1}, Z = B W^T and the Gram matrix G (pqp_batch_get_schur_factor hands out G) -- or, with the
// PrimalLDLT engine, the pair (W, D) of P_J.
int
pqp_batch_get_primal_factor(pqp_batch* h, int64_t idx, double* F, double* dF, double* WL, double* WU, double* Zr,
                            double* Zc, int64_t* meta, double* rho, double* i_scaled)
{
  if (int rc = check_idx(h, idx))
    return rc;
  if (idx < 0)
    return fail(PQP_ERR_INVALID_ARGUMENT, "pqp_batch_get_primal_factor addresses one QP");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  const pqp::Dims& d = h->dev.d;
  const pqp::Batch& D = h->dev;
  const size_t n = size_t(d.n), nd = size_t(d.nd);
  int rc = 0;
  if ((rc = copy_out(F, D.F, idx, D.B, n * n)) || (rc = copy_out(dF, D.dF, idx, D.B, n)) ||
      (rc = copy_out(WL, D.WL, idx, D.B, n * n)) || (rc = copy_out(WU, D.WU, idx, D.B, n * n)) ||
      (rc = copy_out(Zr, D.Zr, idx, D.B, nd * n)) || (rc = copy_out(Zc, D.Zc, idx, D.B, n * nd)) ||
      (rc = copy_out(i_scaled, D.is, idx, D.B, n)))
    return rc;
  pqp::State s;
  HIP_TRY(hipMemcpy(&s, D.state + idx, sizeof(s), hipMemcpyDefault));
  if (meta) {
    meta[0] = s.factor_valid;
    // (Solver::set_diag_mode: the signature of the batch and the per-QP structure of C found by init / update)
    meta[1] = (pqp::diag_structure_signature(d.hessian, d.n_eq, d.n_in, d.box) && s.c_diag != 0) ? 1 : 0;
    meta[2] = d.backend;
    meta[3] = d.hessian;
  }
  if (rho)
    *rho = s.rho_fact;
  return PQP_OK;
}

int
pqp_batch_get_stats(pqp_batch* h, int64_t* stats)
{
  if (!h || !stats)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  static_assert(PQP_STATS_COUNT == pqp::ST_COUNT, "stats record size");
  static_assert(sizeof(long long) == sizeof(int64_t), "stats element size");
  if (int rc = settle(h))
    return rc;
  PQP_ON_DEVICE(h->device);
  HIP_TRY(hipMemcpy(stats, h->dev.stats, size_t(h->dev.B) * pqp::ST_COUNT * sizeof(int64_t), hipMemcpyDefault));
  return PQP_OK;
}

int
pqp_batch_get_trace(pqp_batch* h, int64_t idx, double* records, int64_t capacity, int64_t* n_records)
{
  if (!h || !n_records)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null argument");
  if (idx < 0 || idx >= h->dev.B)
    return fail(PQP_ERR_INVALID_ARGUMENT, "QP index out of range");
  if (int rc = settle(h))
    return rc;
  *n_records = 0;
  if (h->trace_host.empty() || h->trace_slot.empty() || h->trace_slot[size_t(idx)] < 0)
    return PQP_OK; // the last launch did not trace this QP (settings.verbose was off)
  const double* slot = h->trace_host.data() + size_t(h->trace_slot[size_t(idx)]) * PQP_TRACE_RECORDS * 8;
  const int64_t n = int64_t(slot[0]);
  *n_records = n;
  if (records && capacity > 0)
    std::memcpy(records, slot + 8, size_t(std::min(n, capacity)) * 8 * sizeof(double));
  return PQP_OK;
}

double
pqp_batch_last_solve_ms(const pqp_batch* h)
{
  if (h && h->solve_in_flight) // the time of a solve in flight is known once it has finished
    (void)pqp_batch_wait(const_cast<pqp_batch*>(h));
  return h ? double(h->last_ms) : 0.0;
}

double
pqp_batch_last_prologue_ms(const pqp_batch* h)
{
  if (h && h->solve_in_flight)
    (void)pqp_batch_wait(const_cast<pqp_batch*>(h));
  return h ? double(h->last_prologue_ms) : 0.0;
}

int
pqp_batch_launch_config(const pqp_batch* h, int* threads, int64_t* lds_bytes)
{
  if (!h)
    return fail(PQP_ERR_INVALID_ARGUMENT, "null batch handle");
  // (of a launch of the whole batch; the diagonal-structure part of the rule is known once the set-up kernel has run:
  // pqp_batch_flush.  What a launch DID run on: pqp_batch_last_kernel)
  const LaunchPlan p = pqp_plan_solve(h, 0, long(h->dev.B), nullptr);
  if (threads)
    *threads = p.threads;
  if (lds_bytes)
    *lds_bytes = int64_t(p.lds);
  return PQP_OK;
}

const char*
pqp_batch_last_kernel(const pqp_batch* h)
{
  return h ? h->last_kernel : "";
}

} // extern "C"
