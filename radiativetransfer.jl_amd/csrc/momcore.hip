// momcore.hip -- the handle behind the C ABI (include/momcore.h) of libmomcore.so -- create / destroy, options, streams, error
// strings, timers -- and the operator-level API (mom_elemental ... mom_download, mom_postprocess, the batched products and
// inverses) with its kernels.  The other subsystems of the host driver are units of their own: mom_scene.hip (scene-level
// runs), mom_optics.hip (device-side layer optics), mom_rrs_api.hip (rotational Raman), mom_comm.hip (RCCL); what they share
// is mom_handle.hpp.  gfx950 (MI355X) only.  See DESIGN.md for the data layout and the kernel inventory.
#include "mom_handle.hpp"
#include "mom_ops.hpp"
#include "mom_rrs.hpp"

using namespace mom;

// =========================================================================================
// kernels
// =========================================================================================

// operator-level kernels, k_batch_inv and k_batched_mul among them: mom_ops.hpp (shared with the Float32 build)

// batched_mul / batch_inv! on ForwardDiff.Dual arrays (gpu_batched.jl:100-150): values [N,N,S] and P partials [N,N,S,P].
//   mul:  C = A B,      dC_i = A dB_i + dA_i B          inv:  X = A^-1,   dX_i = -X dA_i X
// One workgroup per batch item keeps the values in LDS (slab) while it walks the partials.
struct DualArgs {
  int N, S, P;
  const double *A, *dA, *B, *dB;
  double *C, *dC;
  double *scratch;
  int *info;
};

template <bool LDSM>
__global__ void __launch_bounds__(kThreads) k_batched_mul_dual(DualArgs a) {
  const int N = a.N;
  Ctx c;
  make_ctx<LDSM>(c, N, 1, mom_smem, LDSM ? nullptr : a.scratch + (size_t)blockIdx.x * kGenericBufs * mat_elems(N));
  zero_padding<LDSM>(c);
  __syncthreads();
  const size_t NN = (size_t)N * N;
  const int ld = c.ld;
  for (size_t pt = blockIdx.x; pt < (size_t)a.S; pt += gridDim.x) {
    wg_copy_mat(N, c.fd, a.A + NN * pt, N, c.P, ld);
    wg_copy_mat(N, c.fd, a.B + NN * pt, N, c.Q, ld);
    __syncthreads();
    double *C = a.C + NN * pt;
    wg_gemm<false, !LDSM>(N, ElP{c.P, ld}, ElP{c.Q, ld}, [=](int i, int j, double v) { C[i + (size_t)j * N] = v; });
    for (int ip = 0; ip < a.P; ++ip) {
      const size_t o = NN * (pt + (size_t)a.S * ip);
      __syncthreads();
      wg_copy_mat(N, c.fd, a.dB + o, N, c.r, ld);
      wg_copy_mat(N, c.fd, a.dA + o, N, c.t, ld);
      __syncthreads();
      double *dC = a.dC + o;
      wg_gemm<false, !LDSM>(N, ElP{c.P, ld}, ElP{c.r, ld}, [=](int i, int j, double v) { dC[i + (size_t)j * N] = v; });
      __syncthreads();
      wg_gemm<false, !LDSM>(N, ElP{c.t, ld}, ElP{c.Q, ld},
                            [=](int i, int j, double v) { dC[i + (size_t)j * N] = dC[i + (size_t)j * N] + v; });
    }
    __syncthreads();
  }
}

template <bool LDSM>
__global__ void __launch_bounds__(kThreads) k_batch_inv_dual(DualArgs a) {
  const int N = a.N;
  Ctx c;
  make_ctx<LDSM>(c, N, 1, mom_smem, LDSM ? nullptr : a.scratch + (size_t)blockIdx.x * kGenericBufs * mat_elems(N));
  zero_padding<LDSM>(c);
  if (threadIdx.x == 0) *c.bad = 0;
  __syncthreads();
  const size_t NN = (size_t)N * N;
  const int ld = c.ld;
  for (size_t pt = blockIdx.x; pt < (size_t)a.S; pt += gridDim.x) {
    wg_copy_mat(N, c.fd, a.A + NN * pt, N, c.P, ld);
    __syncthreads();
    if (N <= 64) wg_inverse_reg(N, c.P, ld, c.part, c.prow, c.ipiv, c.bad);
    else wg_inverse(N, c.fd, c.P, ld, c.prow, c.pcol, c.rowk, c.ipiv, c.sh, c.bad);
    wg_copy_mat(N, c.fd, c.P, ld, a.C + NN * pt, N);
    for (int ip = 0; ip < a.P; ++ip) {
      const size_t o = NN * (pt + (size_t)a.S * ip);
      __syncthreads();
      wg_copy_mat(N, c.fd, a.dA + o, N, c.Q, ld);
      __syncthreads();
      double *r = c.r;
      wg_gemm<false, !LDSM>(N, ElP{c.P, ld}, ElP{c.Q, ld}, [=](int i, int j, double v) { r[i + j * ld] = v; });
      __syncthreads();
      double *dX = a.dC + o;
      wg_gemm<false, !LDSM>(N, ElP{c.r, ld}, ElP{c.P, ld}, [=](int i, int j, double v) { dX[i + (size_t)j * N] = -v; });
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && *c.bad) atomicMax(a.info, *c.bad);
}

// =========================================================================================
// host side
// =========================================================================================

static thread_local std::string g_err;

int fail(mom_t *h, int code, const char *msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}

static size_t smem_bytes(const mom_t *h) { return lds_bytes(h->N, h->lds_mode); }

void mom_set_global_error(const char *msg) { g_err = msg ? msg : ""; }
extern "C" const char *mom_last_global_error(void) { return g_err.c_str(); }
extern "C" const char *mom_last_error(const mom_t *h) { return h ? h->err.c_str() : g_err.c_str(); }

// added layer + surface layer of the operator-level API (rt_run.jl:109-112), on first use
static int ensure_op_layers(mom_t *h) {
  if (h->op_layers) return MOM_OK;
  const size_t NN = (size_t)h->N * h->N;
  for (int k = 0; k < 6; ++k) {
    const size_t per = ((k < 4) ? NN : (size_t)h->N) * h->S;
    HIPCHK(h, h->added[k].renew(per));
    HIPCHK(h, h->surf[k].renew(per));
    HIPCHK(h, hipMemsetAsync(h->added[k], 0, per * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->surf[k], 0, per * sizeof(double), h->stream));
  }
  h->op_layers = true;
  return MOM_OK;
}
// the operator-level API keeps the composite matrices in the natural [N,N,S] layout; after a scene-level run the
// allocation holds row-pitched blocks, which the operator kernels must not be fed
static int op_composite_ready(mom_t *h, const char *who) {
  if (h->comp_pitched) {
    char buf[192];
    snprintf(buf, sizeof buf, "%s: the composite layer holds scene-level (mom_rt_run) state; start the operator-level "
             "sequence with mom_copy_added_to_composite or mom_upload", who);
    return fail(h, MOM_ESTATE, buf);
  }
  return MOM_OK;
}

extern "C" int mom_create(mom_t **out, int device, int N, int nStokes, int S, int max_m, int dtype) {
  if (!out || N <= 0 || S <= 0 || max_m <= 0 || nStokes <= 0 || nStokes > 4 || N % nStokes != 0)
    return fail(nullptr, MOM_EINVAL, "mom_create: bad argument");
  if (dtype != 0 && dtype != 1) return fail(nullptr, MOM_EINVAL, "mom_create: dtype must be 0 (Float64) or 1 (Float32)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(nullptr, MOM_EHIP, "mom_create: no HIP device available");
  if (device < 0 || device >= ndev) return fail(nullptr, MOM_EINVAL, "mom_create: device index out of range");
  mom_t *h = new mom_t();
  h->device = device; h->N = N; h->nS = nStokes; h->S = S; h->M = max_m; h->dtype = dtype;
  h->lds_mode = (N <= 64);
  *out = h;
  HIPCHK(h, hipSetDevice(device));
  HIPCHK(h, hipStreamCreate(&h->stream));
  {  // the second stream of MOM_OPT_OVERLAP: highest priority, so that its (shorter) launches are dispatched first
    int lo = 0, hi = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(h, hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, hi));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_go, hipEventDisableTiming));
  }
  const size_t NN = (size_t)N * N;
  const int Na = N + kMomPadMax;  // room for the dummy entries of strip_pad
  HIPCHK(h, h->d_mu.renew(Na));
  HIPCHK(h, h->d_wt.renew(Na));
  HIPCHK(h, h->d_sg.renew(Na));
  (void)NN;
  for (int k = 0; k < 6 && dtype == 0; ++k) {
    // composite blocks: room for the scene-level row pitch (comp_pitch); the operator-level API uses the natural one.
    // The added / surface layers of the operator-level API (12 N^2 S doubles) are allocated on its first use
    // (ensure_op_layers): the scene-level path keeps the added layer in LDS and never needs them.
    const size_t perc = (k < 4) ? (size_t)comp_pitch(Na) * Na : (size_t)Na;
    HIPCHK(h, h->comp[k].renew(perc * S * max_m));
    HIPCHK(h, hipMemsetAsync(h->comp[k], 0, perc * S * max_m * sizeof(double), h->stream));
  }
  for (int k = 0; k < 4; ++k) HIPCHK(h, h->d_vec[k].renew(S));
  HIPCHK(h, h->d_info.renew(1));
  HIPCHK(h, hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
  h->G = 1024;
  {
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, device));
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  if (dtype == 1) {  // Float32: the scene-level state lives in the f32 build's own object
    for (int k = 0; k < 4; ++k) HIPCHK(h, hipEventCreate(&h->ev[k]));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int rc = momf_create(&h->f32, device, h->stream, N, nStokes, S, max_m, h->d_info);
    if (rc) return fail(h, rc, momf_error(h->f32));
    return MOM_OK;
  }
  // + one padded matrix of slack: B-operand reads of the last column tile run past the stored columns
  HIPCHK(h, h->d_scratch.renew((size_t)h->G * kGenericBufs * mat_elems(N) + (size_t)ld_for(N) * np_for(N)));
  HIPCHK(h, hipMemsetAsync(h->d_scratch, 0, ((size_t)h->G * kGenericBufs * mat_elems(N) + (size_t)ld_for(N) * np_for(N)) * sizeof(double), h->stream));
  for (int k = 0; k < 4; ++k) HIPCHK(h, hipEventCreate(&h->ev[k]));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_destroy(mom_t *h) {
  if (!h) return MOM_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->f32) momf_destroy(h->f32);
  momr::destroy(h->rrs);
  if (h->comm && g_rccl_destroy) g_rccl_destroy(h->comm);
  for (int k = 0; k < 4; ++k) if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
  for (int k = 0; k < 2; ++k) if (h->ev_voigt[k]) (void)hipEventDestroy(h->ev_voigt[k]);
  for (auto e : h->ev_full) (void)hipEventDestroy(e);
  for (auto e : h->ev_red) (void)hipEventDestroy(e);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_go) (void)hipEventDestroy(h->ev_go);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // frees every device buffer of the handle (MomDevBuf members)
  return MOM_OK;
}

extern "C" int mom_sync(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_strip2_resumed(mom_t *h, int *units, int *left) {
  if (!h || !units || !left) return fail(h, MOM_EINVAL, "mom_strip2_resumed: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *units = (int)h->resume2_units; *left = 0;
  if (!h->d_resume2 || h->resume2_units == 0) { *units = 0; return MOM_OK; }
  std::vector<int> r(h->resume2_units);
  HIPCHK(h, hipMemcpy(r.data(), h->d_resume2, r.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int v : r) *left += (v < h->resume2_nz);
  return MOM_OK;
}

extern "C" int mom_check(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  HIPCHK(h, hipSetDevice(h->device));
  return check_info(h);
}

extern "C" int mom_set_option(mom_t *h, int option, int value) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (option == MOM_OPT_INVERSE) { h->opt_inverse = value; h->q.inv_mode = value; h->qk.inv_mode = value; h->q0.inv_mode = value; }
  else if (option == MOM_OPT_M0_REDUCTION) h->opt_m0 = value;
  else if (option == MOM_OPT_SMALL_WG) h->opt_w4 = value;
  else if (option == MOM_OPT_STAGGER) h->opt_stagger = value;
  else if (option == MOM_OPT_SMALL_N) { h->opt_small = value; h->scene_set = false; }  // the padded edge Nk depends on it
  else if (option == MOM_OPT_LAYER_SWEEP) h->opt_sweep = value;
  else if (option == MOM_OPT_STRIP_PAD) { h->opt_pad = value; h->scene_set = false; }
  else if (option == MOM_OPT_LEAN) { h->opt_lean = value; h->scene_set = false; }  // the padded edge of the m = 0 sub-problem depends on it
  else if (option == MOM_OPT_OVERLAP) h->opt_overlap = value;
  else if (option == MOM_OPT_STRIP2) h->opt_strip2 = value;
  else if (option == MOM_OPT_STRIP2_SCHED) {
    if (value < 0 || value > 3) return fail(h, MOM_EINVAL, "mom_set_option: MOM_OPT_STRIP2_SCHED takes a mask of bits 0 and 1");
    h->opt_strip2_sched = value;
  }
  else if (option == MOM_OPT_ZERO_SKIP) {
    if (value < 0 || value > 7) return fail(h, MOM_EINVAL, "mom_set_option: MOM_OPT_ZERO_SKIP takes a mask of bits 0, 1 and 2");
    h->opt_zero_skip = value;
  }
  else if (option == MOM_OPT_SOURCES_ONLY) h->opt_sources_only = value;
  else if (option == MOM_OPT_ELEMENTAL) h->opt_elemental = value;
  else if (option == MOM_OPT_LUT_BATCH) {
    if (value < 0) return fail(h, MOM_EINVAL, "mom_set_option: MOM_OPT_LUT_BATCH takes a number of (p, T) nodes >= 0 (0 = the default of 64)");
    h->opt_lut_batch = value;
  }
  else if (option == MOM_OPT_DUAL_WORKSPACE_MB) {
    if (value < 0) return fail(h, MOM_EINVAL, "mom_set_option: MOM_OPT_DUAL_WORKSPACE_MB takes megabytes >= 0 (0 = 60 % of the free HBM)");
    h->opt_dual_budget = (size_t)value << 20;
  }
  else if (option == MOM_OPT_RRS_KERNELS) {
    if (value < 0 || value > 63 || ((value & momr::KOPT_EL_FUSE_ON) && (value & momr::KOPT_EL_FUSE_OFF)))
      return fail(h, MOM_EINVAL, "mom_set_option: MOM_OPT_RRS_KERNELS takes a mask of bits 0..5 (bits 4 and 5 exclude each other)");
    h->opt_rrs_kernels = value;
    if (h->rrs) h->rrs->kopt = value;
  }
  else if (option == MOM_OPT_FORCE_GENERIC) {
    h->opt_force_generic = value;
    h->lds_mode = (h->N <= 64) && !value;
  } else return fail(h, MOM_EINVAL, "mom_set_option: unknown option");
  if (h->f32) momf_set_options(h->f32, h->opt_inverse, h->opt_force_generic, h->opt_sweep, h->opt_small, h->opt_m0, h->opt_pad, h->opt_w4);
  return MOM_OK;
}

extern "C" int mom_set_streams(mom_t *h, const double *qp_muN, const double *wt_muN, int N, int imu0_1based, double mu0,
                               const double *I0, const double *D, int strict) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (N != h->N || !qp_muN || !wt_muN || !I0 || !D || imu0_1based < 1 || imu0_1based * h->nS > N)
    return fail(h, MOM_EINVAL, "mom_set_streams: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  h->h_mu.assign(qp_muN, qp_muN + N);
  h->h_wt.assign(wt_muN, wt_muN + N);
  h->strict = strict;
  h->stage_z.drop(); h->stage_r.drop(); h->stage_d.drop();  // Greek sets staged for the previous nodes
  std::vector<double> sg(N);
  for (int i = 0; i < N; ++i) {
    const int comp = strict ? ((i + 1) % h->nS) : (i % h->nS) + 1;
    sg[i] = (comp > 2) ? -1.0 : 1.0;
  }
  {
    std::vector<double> mu(qp_muN, qp_muN + N), wt(wt_muN, wt_muN + N);
    mu.resize(N + kMomPadMax, 1.0); wt.resize(N + kMomPadMax, 0.0); sg.resize(N + kMomPadMax, 1.0);  // dummy entries (strip_pad)
    HIPCHK(h, hipMemcpyAsync(h->d_mu, mu.data(), mu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_wt, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_sg, sg.data(), sg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  DevStreams &q = h->q;
  q.mu = h->d_mu; q.wt = h->d_wt; q.sg = h->d_sg;
  for (int k = 0; k < 4; ++k) { q.I0[k] = (k < h->nS) ? I0[k] : 0.0; q.D[k] = (k < h->nS) ? D[k] : 1.0; }
  q.N = N; q.nS = h->nS; q.imu0 = imu0_1based; q.mu0 = mu0; q.inv_mode = h->opt_inverse;
  q.regular = 1;
  for (int i = 0; i < N; ++i)
    if (qp_muN[i] != qp_muN[(i / h->nS) * h->nS]) q.regular = 0;
  if (h->f32) {
    momf_set_options(h->f32, h->opt_inverse, h->opt_force_generic, h->opt_sweep, h->opt_small, h->opt_m0, h->opt_pad, h->opt_w4);
    const int rc = momf_set_streams(h->f32, qp_muN, wt_muN, sg.data(), imu0_1based, mu0, I0, D, q.regular);
    if (rc) return fail(h, rc, momf_error(h->f32));
  }
  h->streams_set = true;
  h->scene_set = false;  // the reduced (I,Q) stream set of a resident scene was derived from the old streams
  return MOM_OK;
}

static int grid_for(const mom_t *h, size_t total) {
  if (h->lds_mode) return (int)total;
  return (int)std::min<size_t>(total, (size_t)h->G);
}
int check_info(mom_t *h) {
  int info = 0;
  HIPCHK(h, hipMemcpyAsync(&info, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (info) {
    HIPCHK(h, hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
    char buf[128];
    snprintf(buf, sizeof buf, "zero pivot at elimination step %d while inverting (I - R r)", info);
    return fail(h, MOM_ESINGULAR, buf);
  }
  return MOM_OK;
}

// operator-level entry points: KERN<LDSM> (LAUNCH2: KERN<LDSM, TARG>) on the handle's stream with the handle's LDS image
#define LAUNCH(h, KERN, grid, args) \
  HIPCHK(h, mom_launch_ldsm(MOM_LDSM(KERN), (h)->lds_mode, grid, kThreads, smem_bytes(h), (h)->stream, args))
#define LAUNCH2(h, KERN, TARG, grid, args) \
  HIPCHK(h, mom_launch_ldsm(MOM_LDSM(KERN, TARG), (h)->lds_mode, grid, kThreads, smem_bytes(h), (h)->stream, args))

extern "C" int mom_elemental(mom_t *h, int m, int ndoubl, const double *tau_sum, const double *dtau, const double *varpi,
                             const double *Zpp, const double *Zmp, int z_batch) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_elemental: call mom_set_streams first");
  if (!tau_sum || !dtau || !varpi || !Zpp || !Zmp || (z_batch != 1 && z_batch != h->S) || m < 0 || ndoubl < 0)
    return fail(h, MOM_EINVAL, "mom_elemental: bad argument");
  if (h->f32) {
    const int rc = momf_op_elemental(h->f32, m, ndoubl, tau_sum, dtau, varpi, Zpp, Zmp, z_batch);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  const size_t NN = (size_t)h->N * h->N, zc = NN * z_batch;
  for (int k = 0; k < 2; ++k) HIPCHK(h, h->d_Zop[k].reserve(zc, h->stream));
  const size_t sb = (size_t)h->S * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(h->d_vec[0], tau_sum, sb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_vec[1], dtau, sb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_vec[2], varpi, sb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_Zop[0], Zpp, zc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_Zop[1], Zmp, zc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  OpArgs a{};
  a.q = h->q; a.S = h->S; a.m = m; a.nd = ndoubl; a.z_batch = z_batch;
  a.tau_sum = h->d_vec[0]; a.dtau = h->d_vec[1]; a.varpi = h->d_vec[2]; a.Zpp = h->d_Zop[0]; a.Zmp = h->d_Zop[1];
  for (int k = 0; k < 6; ++k) a.added[k] = h->added[k];
  a.scratch = h->d_scratch; a.info = h->d_info;
  LAUNCH(h, k_op_elemental, grid_for(h, h->S), a);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_doubling(mom_t *h, int ndoubl, double *expk) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_doubling: call mom_set_streams first");
  if (!expk || ndoubl < 0) return fail(h, MOM_EINVAL, "mom_doubling: bad argument");
  if (h->f32) {
    const int rc = momf_op_doubling(h->f32, ndoubl, expk);
    return rc ? fail(h, rc, momf_error(h->f32)) : check_info(h);
  }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  const size_t sb = (size_t)h->S * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(h->d_vec[3], expk, sb, hipMemcpyHostToDevice, h->stream));
  OpArgs a{};
  a.q = h->q; a.S = h->S; a.nd = ndoubl; a.expk = h->d_vec[3];
  for (int k = 0; k < 6; ++k) a.added[k] = h->added[k];
  a.scratch = h->d_scratch; a.info = h->d_info;
  if (ndoubl > 0) LAUNCH(h, k_op_doubling, grid_for(h, h->S), a);  // doubling.jl:28 returns early for 0
  HIPCHK(h, hipMemcpyAsync(expk, h->d_vec[3], sb, hipMemcpyDeviceToHost, h->stream));
  return check_info(h);
}

extern "C" int mom_interaction(mom_t *h, int iface, int with_surface_layer) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_interaction: call mom_set_streams first");
  if (iface < 0 || iface > 3) return fail(h, MOM_EINVAL, "mom_interaction: iface must be 0..3");
  if (h->f32) {
    const int rc = momf_op_interaction(h->f32, iface, with_surface_layer);
    return rc ? fail(h, rc, momf_error(h->f32)) : check_info(h);
  }
  HIPCHK(h, hipSetDevice(h->device));
  { int rc_ = ensure_op_layers(h); if (rc_) return rc_; if ((rc_ = op_composite_ready(h, "mom_interaction"))) return rc_; }
  OpArgs a{};
  a.q = h->q; a.S = h->S; a.iface = iface;
  for (int k = 0; k < 6; ++k) { a.added[k] = with_surface_layer ? h->surf[k] : h->added[k]; a.comp[k] = h->comp[k]; }
  a.scratch = h->d_scratch; a.info = h->d_info;
  LAUNCH(h, k_op_interaction, grid_for(h, h->S), a);
  return check_info(h);
}

// k_combine (mom_rt_run_multisensor, mom_scene.hip) is built and launched here, next to k_op_interaction: the two share
// interaction_core<LDSM, -1>, and in a unit where k_combine is its only caller the compiler folds k_combine's constant interface
// code into it -- other machine code than the library has had so far (profiles/r11_split_resources.txt)
hipError_t mom_launch_combine(const InterArgs &a, bool lds, int grid, size_t smem, hipStream_t st) {
  return mom_launch_ldsm(MOM_LDSM(k_combine), lds, grid, kThreads, smem, st, a);
}

extern "C" int mom_copy_added_to_composite(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (h->f32) {
    const int rc = momf_op_copy_added_to_composite(h->f32);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  h->comp_pitched = false;
  const size_t NN = (size_t)h->N * h->N;
  // composite order: R_mp, R_pm, T_pp, T_mm, J0p, J0m ; added order: r_pm, r_mp, t_mm, t_pp, j0p, j0m
  const int src[6] = {1, 0, 3, 2, 4, 5};
  for (int k = 0; k < 6; ++k) {
    const size_t bytes = ((k < 4) ? NN : (size_t)h->N) * h->S * sizeof(double);
    HIPCHK(h, hipMemcpyAsync(h->comp[k], h->added[src[k]], bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_surface_lambertian(mom_t *h, int m, double albedo, const double *tau_tot) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_surface_lambertian: call mom_set_streams first");
  if (!tau_tot || m < 0) return fail(h, MOM_EINVAL, "mom_surface_lambertian: bad argument");
  if (h->f32) {
    const int rc = momf_op_surface_lambertian(h->f32, m, albedo, tau_tot);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  HIPCHK(h, hipMemcpyAsync(h->d_vec[0], tau_tot, (size_t)h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_op_surface_fill, dim3(h->S), dim3(256), 0, h->stream, h->q, h->S, m, albedo, h->d_vec[0],
                     h->surf[0], h->surf[1], h->surf[2], h->surf[3], h->surf[4], h->surf[5]);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

static double *which_ptr(mom_t *h, int which, size_t *count) {
  const size_t NN = (size_t)h->N * h->N;
  if (which < 0 || which > 17) return nullptr;
  const int grp = which / 6, k = which % 6;
  *count = ((k < 4) ? NN : (size_t)h->N) * h->S;
  return grp == 0 ? h->added[k] : (grp == 1 ? h->comp[k] : h->surf[k]);
}

extern "C" int mom_upload(mom_t *h, int which, const double *src) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (which < 0 || which > 17 || !src) return fail(h, MOM_EINVAL, "mom_upload: bad argument");
  if (h->f32) {
    const int rc = momf_op_upload(h->f32, which, src);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (which / 6 != 1) { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  else h->comp_pitched = false;  // the caller (re)starts an operator-level sequence: natural [N,N,S] layout
  size_t count = 0;
  double *p = which_ptr(h, which, &count);
  HIPCHK(h, hipMemcpyAsync(p, src, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_download(mom_t *h, int which, double *dst) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (which < 0 || which > 17 || !dst) return fail(h, MOM_EINVAL, "mom_download: bad argument");
  if (h->f32) {
    const int rc = momf_op_download(h->f32, which, dst);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (which / 6 != 1) { const int rc_ = ensure_op_layers(h); if (rc_) return rc_; }
  size_t count = 0;
  double *p = which_ptr(h, which, &count);
  if (which / 6 == 1 && h->comp_pitched) {
    // after mom_rt_run: moment slot 0 of the scene-level state.  With the m = 0 reduction that moment lives in the
    // (I,Q) sub-problem's own arrays, which have no [N,N,S] image
    if (h->comp_on_chip)
      return fail(h, MOM_ESTATE, "mom_download: the run kept the composite layer in registers (operator edge <= 32); set "
                                 "MOM_OPT_SMALL_N = 0 before mom_rt_run to read it back");
    if (h->red0)
      return fail(h, MOM_ESTATE, "mom_download: Fourier moment 0 ran on the (I,Q) sub-problem; set "
                                 "MOM_OPT_M0_REDUCTION = 0 before mom_scene_set to read the composite layer back");
    if (h->Nk != h->N)
      return fail(h, MOM_ESTATE, "mom_download: the scene ran on an operator edge padded to a strip-chained kernel size; "
                                 "set MOM_OPT_STRIP_PAD = 0 before mom_scene_set to read the composite layer back");
    if (which % 6 < 4) {  // de-pitch: columns of N doubles at a pitch of comp_pitch(N)
      HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)h->N * sizeof(double), p, (size_t)comp_pitch(h->N) * sizeof(double),
                                 (size_t)h->N * sizeof(double), (size_t)h->N * h->S, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return MOM_OK;
    }
  }
  HIPCHK(h, hipMemcpyAsync(dst, p, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

static int blas_common(mom_t *h, int n, int batch, const double *A, const double *B, double *C, bool inv) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (n <= 0 || batch <= 0 || !A || !C || (!inv && !B)) return fail(h, MOM_EINVAL, "batched op: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->f32) {  // Float32 handle: the f32 build's kernels (gpu_batched.jl:45-58)
    const int rc = momf_blas(h->f32, n, batch, A, B, C, inv);
    if (rc) return fail(h, rc, momf_error(h->f32));
    return inv ? check_info(h) : MOM_OK;
  }
  HIPCHK(h, batched_run(h->stream, h->ws, h->d_info, h->opt_force_generic != 0, n, batch, A, B, C, inv));  // mom_ops.hpp
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return inv ? check_info(h) : MOM_OK;
}

extern "C" int mom_batch_inv(mom_t *h, int n, int batch, const double *A, double *X) {
  return blas_common(h, n, batch, A, nullptr, X, true);
}
extern "C" int mom_batched_mul(mom_t *h, int n, int batch, const double *A, const double *B, double *C) {
  return blas_common(h, n, batch, A, B, C, false);
}

static int dual_common(mom_t *h, int n, int batch, int P, const double *A, const double *dA, const double *B,
                       const double *dB, double *C, double *dC, bool inv) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_batch_inv_dual / mom_batched_mul_dual");
  if (n <= 0 || batch <= 0 || P < 0 || !A || !C || (P > 0 && (!dA || !dC)) || (!inv && (!B || (P > 0 && !dB))))
    return fail(h, MOM_EINVAL, "batched dual op: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)n * n * batch, cntP = cnt * P;
  double *buf = nullptr, *scr = nullptr;
  // one allocation: A, B, C [cnt] and dA, dB, dC [cntP]
  HIPCHK(h, h->ws[0].reserve((3 * cnt + 3 * cntP + 1) * sizeof(double), h->stream));
  buf = reinterpret_cast<double *>(h->ws[0].get());
  double *dA_ = buf + 3 * cnt, *dB_ = dA_ + cntP, *dC_ = dB_ + cntP;
  HIPCHK(h, hipMemcpyAsync(buf, A, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (P) HIPCHK(h, hipMemcpyAsync(dA_, dA, cntP * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (!inv) {
    HIPCHK(h, hipMemcpyAsync(buf + cnt, B, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (P) HIPCHK(h, hipMemcpyAsync(dB_, dB, cntP * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  const bool lds = n <= 64 && !h->opt_force_generic;
  const int grid = lds ? batch : std::min(batch, 1024);
  if (!lds) {
    const size_t scn = (size_t)grid * kGenericBufs * mat_elems(n) + (size_t)ld_for(n) * np_for(n);
    HIPCHK(h, h->ws[3].reserve(scn * sizeof(double), h->stream));
    scr = reinterpret_cast<double *>(h->ws[3].get());
    HIPCHK(h, hipMemsetAsync(scr, 0, scn * sizeof(double), h->stream));
  }
  DualArgs a{n, batch, P, buf, dA_, buf + cnt, dB_, buf + 2 * cnt, dC_, scr, h->d_info};
  const size_t sm = lds_bytes(n, lds);
  if (inv) {
    HIPCHK(h, mom_launch_ldsm(MOM_LDSM(k_batch_inv_dual), lds, grid, kThreads, sm, h->stream, a));
  } else {
    HIPCHK(h, mom_launch_ldsm(MOM_LDSM(k_batched_mul_dual), lds, grid, kThreads, sm, h->stream, a));
  }
  HIPCHK(h, hipMemcpyAsync(C, buf + 2 * cnt, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (P) HIPCHK(h, hipMemcpyAsync(dC, dC_, cntP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));

  return inv ? check_info(h) : MOM_OK;
}

extern "C" int mom_batch_inv_dual(mom_t *h, int n, int batch, int P, const double *A, const double *dA, double *X, double *dX) {
  return dual_common(h, n, batch, P, A, dA, nullptr, nullptr, X, dX, true);
}
extern "C" int mom_batched_mul_dual(mom_t *h, int n, int batch, int P, const double *A, const double *dA, const double *B,
                                    const double *dB, double *C, double *dC) {
  return dual_common(h, n, batch, P, A, dA, B, dB, C, dC, false);
}

// ---------------------------------------------------------------- operator-level post-processing

// cosd / sind as Julia evaluates them (base/special/trig.jl): reduction in degrees, double-double radians
// (deg2rad_ext), fdlibm kernels with the low word -- exact at the multiples of 30 and 90 degrees
#pragma clang fp contract(off)
static void mom_deg2rad_ext(double x, double &hi, double &lo) {
  const double m = 0.017453292519943295, m_hi = 0.01745329238474369, m_lo = 1.3519960527851425e-10;
  const volatile double u = 134217729.0 * x;
  const volatile double t = u - x;
  const double x_hi = u - t, x_lo = x - x_hi;
  hi = m * x;
  lo = x_hi * m_lo + (x_lo * m_hi + ((x_hi * m_hi - hi) + x_lo * m_lo));
}
static double mom_ksin(double deg) {
  double x, y;
  mom_deg2rad_ext(deg, x, y);
  const double z = x * x, v = z * x;
  const double r = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  return x - ((z * (0.5 * y - v * r) - y) - v * -1.66666666666666324348e-01);
}
static double mom_kcos(double deg) {
  double x, y;
  mom_deg2rad_ext(deg, x, y);
  const double z = x * x;
  double w = z * z;
  const double r = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                   w * w * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
  const double hz = 0.5 * z;
  w = 1.0 - hz;
  return w + (((1.0 - w) - hz) + (z * r - x * y));
}
static double mom_cosd(double x) {
  const double rx = std::fabs(std::fmod(x, 360.0));
  if (rx <= 45.0) return mom_kcos(rx);
  if (rx < 135.0) return mom_ksin(90.0 - rx);
  if (rx <= 225.0) return -mom_kcos(180.0 - rx);
  if (rx < 315.0) return mom_ksin(rx - 270.0);
  return mom_kcos(360.0 - rx);
}
static double mom_sind(double x) {
  const double rx = std::fmod(x, 360.0), arx = std::fabs(rx);
  if (rx == 0.0) return rx;
  if (arx < 45.0) return mom_ksin(rx);
  if (arx <= 135.0) return std::copysign(mom_kcos(90.0 - arx), rx);
  if (arx == 180.0) return std::copysign(0.0, rx);
  if (arx < 225.0) return mom_ksin((180.0 - arx) * std::copysign(1.0, rx));
  if (arx <= 315.0) return -std::copysign(mom_kcos(270.0 - arx), rx);
  return mom_ksin(rx - std::copysign(360.0, rx));
}

// postprocessing_vza!(RS_type::noRS, iμ₀, pol_type, composite_layer, vza, qp_μ, m, vaz, μ₀, weight, nSpec, SFI, R, R_SFI,
// T, T_SFI, ...) -- postprocessing_vza.jl:9-60 for ONE Fourier moment on the operator-level composite layer: gathers
// the nVza view rows of J0-/J0+ on the GPU (the reference copies the whole composite layer to the host, :17-20)
__global__ void k_op_postprocess(int N, int nS, int S, int nVza, const int *node, const double *cs_k, const double *J0p,
                                 const double *J0m, double *outR, double *outT) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nVza * nS * S;
  if (idx >= total) return;
  const int v = (int)(idx % nVza);
  const int k = (int)((idx / nVza) % nS);
  const size_t s = idx / ((size_t)nVza * nS);
  const size_t o = (size_t)(node[v] - 1) * nS + k + (size_t)N * s;
  const double cs = cs_k[v + (size_t)nVza * k];
  outR[idx] = cs * J0m[o];
  outT[idx] = cs * J0p[o];
}

extern "C" int mom_postprocess(mom_t *h, int m, int nVza, const int *node_1based, const double *vaz_deg, double weight,
                               double *R_SFI, double *T_SFI) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_postprocess");
  if (m < 0 || nVza <= 0 || !node_1based || !vaz_deg || !R_SFI || !T_SFI)
    return fail(h, MOM_EINVAL, "mom_postprocess: bad argument");
  for (int v = 0; v < nVza; ++v)
    if (node_1based[v] < 1 || node_1based[v] * h->nS > h->N) return fail(h, MOM_EINVAL, "mom_postprocess: bad view node");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc_ = op_composite_ready(h, "mom_postprocess"); if (rc_) return rc_; }
  const size_t total = (size_t)nVza * h->nS * h->S;
  HIPCHK(h, h->d_post.reserve(2 * total, h->stream));
  double *const d_post[2] = {h->d_post, h->d_post + total};
  // bigCS = weight * Diagonal([cos(m φ), cos(m φ), sin(m φ), sin(m φ)][1:n])   (postprocessing_vza.jl:32-33)
  auto cosd = [](double x) { return mom_cosd(x); };
  auto sind = [](double x) { return mom_sind(x); };
  std::vector<double> cs((size_t)nVza * h->nS);
  for (int k = 0; k < h->nS; ++k)
    for (int v = 0; v < nVza; ++v) cs[v + (size_t)nVza * k] = weight * ((k < 2) ? cosd(m * vaz_deg[v]) : sind(m * vaz_deg[v]));
  int *d_node = nullptr;
  double *d_cs = nullptr;
  HIPCHK(h, h->ws[2].reserve((size_t)nVza * sizeof(int), h->stream));   // grow-only workspace of the handle: no allocation per call, nothing to leak
  d_node = reinterpret_cast<int *>(h->ws[2].get());
  HIPCHK(h, h->ws[3].reserve(cs.size() * sizeof(double), h->stream));
  d_cs = reinterpret_cast<double *>(h->ws[3].get());
  HIPCHK(h, hipMemcpyAsync(d_node, node_1based, (size_t)nVza * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_op_postprocess, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->N, h->nS, h->S, nVza,
                     d_node, d_cs, h->comp[4].get(), h->comp[5].get(), d_post[0], d_post[1]);
  HIPCHK(h, hipGetLastError());
  std::vector<double> hr(total), ht(total);
  HIPCHK(h, hipMemcpyAsync(hr.data(), d_post[0], total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ht.data(), d_post[1], total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < total; ++i) { R_SFI[i] += hr[i]; T_SFI[i] += ht[i]; }  // `+=` like :48-49
  return MOM_OK;
}

#ifdef MOM_DIAG_STAMPS
extern "C" int mom_diag_read(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mom_diag_acc), 128 * sizeof(unsigned long long)) != hipSuccess) return MOM_EHIP;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mom_diag_acc), z, sizeof z) != hipSuccess) return MOM_EHIP;
  }
  return MOM_OK;
}
#endif

extern "C" int mom_timers(mom_t *h, double *ms, int n, int *kernel_launches) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!ms || n < 4) return fail(h, MOM_EINVAL, "mom_timers: need room for 4 values");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->f32) {
    for (int k = 0; k < n; ++k) ms[k] = 0.0;
    int nl = 0;
    const int rc = momf_timers(h->f32, ms, &nl);
    if (rc) return fail(h, rc, momf_error(h->f32));
    if (n >= 8) { ms[4] = ms[0]; ms[6] = nl; }
    if (kernel_launches) *kernel_launches = nl;
    return MOM_OK;
  }
  HIPCHK(h, mom_stage_times(h->ev, ms));
  if (n >= 8) {  // per-kernel sums: full-problem layer launches, reduced (m = 0) layer launches
    double full = 0.0, red = 0.0;
    float t;
    for (int z = 0; z < h->launches_full; ++z) { HIPCHK(h, hipEventElapsedTime(&t, h->ev_full[2 * z], h->ev_full[2 * z + 1])); full += t; }
    for (int z = 0; z < h->launches_red; ++z) { HIPCHK(h, hipEventElapsedTime(&t, h->ev_red[2 * z], h->ev_red[2 * z + 1])); red += t; }
    ms[4] = full; ms[5] = red; ms[6] = h->launches_full; ms[7] = h->launches_red;
  }
  if (kernel_launches) *kernel_launches = h->launches;
  return MOM_OK;
}
