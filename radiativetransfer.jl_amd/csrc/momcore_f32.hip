// momcore_f32.hip -- the Float32 build of the scene-level path (mom_create(..., dtype = 1)).
//
// The reference selects its float type with `float_type` (parameters_from_yaml.jl:160; batched ops for Float32 at
// gpu_batched.jl:45-58, the shapes of its own GPU tests: test/gpu_tests/gpu_batched_interaction.jl, n = 32, S = 20 000,
// Float32).  The same device templates as the Float64 library are compiled here with MOM_REAL = float in namespace
// momf: operators and sources in f32, products on v_mfma_f32_16x16x4_f32 (32 cycles per instruction per SIMD: twice
// the f64 rate), LDS images half the size.  What runs: the fused per-layer kernels of the general path (LDS-resident
// for N <= 64, generic mode above), layer-sweep mode, the surface layer (all three surface kinds) with HDRF/BHR, and
// post-processing; r4: the strip-chained images of the 8-wave build (N = 44, 52, 56, 60: momcore_strip.hip compiled for
// float, families F32_STRIP8 / F32_STRIP4 of mom_images.hpp), the (I,Q) reduction of moment 0 (a nested sub-scene: momf_scene::sub) and the padding of
// other edges to the strip sizes (strip_pad_f), and the operator-level API on dtype = 1 handles (mom_ops.hpp compiled for float:
// mom_elemental ... mom_download); r6: the device-side optics route (momf_scene_set_dev: the layer optics assembled in Float64 on the
// device, rounded there).  Not built for f32: multi-sensor, RRS, the Dual run.
//
// What this driver shares with the Float64 one, and what stays apart on purpose: DESIGN.md, section 3.
//
// The C ABI keeps Float64 host arrays for both dtypes (a Float32 Julia host passes Float64.(x) and converts back):
// inputs are rounded to f32 on upload, outputs widened on download.
#define MOM_REAL float
#define MOM_REAL_IS_FLOAT 1
#define MOM_NS momf
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "momcore.h"

#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_ops.hpp"
#include "mom_host.hpp"
#include "mom_images.hpp"
#include "mom_reduce.hpp"

using namespace momf;

namespace {

struct PostArgsF {
  int N, nS, S, M, nVza, hdr_all, zeroT_hi, m_first;  // M moments starting at Fourier index m_first
  const int *node;
  const double *cos_mphi, *sin_mphi;
  const float *J0p, *J0m, *hdrJ0, *hdrJm;
  float *R, *T, *hdr;
};
// postprocessing_vza! / postprocessing_vza_hdrf! (postprocessing_vza.jl:9-93); the azimuthal weights stay Float64
// like the reference's host-side `bigCS`, the sources are f32
__global__ void k_postprocess_f32(PostArgsF a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)a.nVza * a.nS * a.S;
  if (idx >= total) return;
  const int v = (int)(idx % a.nVza);
  const int k = (int)((idx / a.nVza) % a.nS);
  const size_t s = idx / ((size_t)a.nVza * a.nS);
  const int row = (a.node[v] - 1) * a.nS + k;
  float r = 0.f, t = 0.f, h = 0.f;
  for (int mr = 0; mr < a.M; ++mr) {
    const int m = a.m_first + mr;
    const double weight = (m == 0) ? 0.5 : 1.0;
    const float cs = (float)(weight * ((k < 2) ? a.cos_mphi[v + (size_t)a.nVza * m] : a.sin_mphi[v + (size_t)a.nVza * m]));
    const size_t o = row + (size_t)a.N * (s + (size_t)a.S * mr);
    r += cs * a.J0m[o];
    if (!(a.zeroT_hi && m > 0)) t += cs * a.J0p[o];
    if (m == 0) h += cs * a.hdrJ0[row + (size_t)a.N * s];
    else if (a.hdr_all) h += cs * a.hdrJm[row + (size_t)a.N * (s + (size_t)a.S * m)];
  }
  a.R[idx] = r;
  a.T[idx] = t;
  a.hdr[idx] = h;
}

// m = 0 reduction: the (I,Q) sub-scene's spectra [nVza,nS0,S] and BHR [nS0,S] are added to / become the first nS0 Stokes
// components of the full scene's (whose own moments start at m = 1); components >= nS0 get no m = 0 term (exactly 0)
struct CombineArgsF {
  int nVza, nS, nS0, S;
  float *R, *T, *hdr, *bhr_uw, *bhr_dw;
  const float *R0, *T0, *hdr0, *bhr0_uw, *bhr0_dw;
};
__global__ void k_combine_m0_f32(CombineArgsF a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)a.nVza * a.nS * a.S;
  if (idx < total) {
    const int v = (int)(idx % a.nVza), k = (int)((idx / a.nVza) % a.nS);
    const size_t s = idx / ((size_t)a.nVza * a.nS);
    if (k < a.nS0) {
      const size_t o = v + (size_t)a.nVza * (k + (size_t)a.nS0 * s);
      a.R[idx] += a.R0[o];
      a.T[idx] += a.T0[o];
      a.hdr[idx] += a.hdr0[o];
    }
  }
  if (idx < (size_t)a.nS * a.S) {
    const int k = (int)(idx % a.nS);
    const size_t s = idx / a.nS;
    a.bhr_uw[idx] = (k < a.nS0) ? a.bhr0_uw[k + (size_t)a.nS0 * s] : 0.f;
    a.bhr_dw[idx] = (k < a.nS0) ? a.bhr0_dw[k + (size_t)a.nS0 * s] : 0.f;
  }
}

}  // namespace

// Edges with a Float32 strip-chained image (the image table, mom_images.hpp); other edges are padded with dummy stream entries
// to reach one (the pad rule: mom_host.hpp)
static bool strip_size_f(int N) { return mom_find_image(MOM_IMG_F32_STRIP4, N) || mom_find_image(MOM_IMG_F32_STRIP8, N); }
static int strip_pad_f(int N) { return mom_strip_pad(strip_size_f, N); }

// (the resident scene's arrays and counts: MomSceneBufs, mom_host.hpp)
struct momf_scene : MomSceneBufs<float> {
  int device = 0, N = 0, nS = 0, S = 0, M = 0;  // M: moments allocated (the resident scene's: scene_M)
  int Nu = 0, Nmax = 0;  // Nu: the caller's operator edge; N: the kernels' (strip_pad_f, decided in momf_set_streams); Nmax: allocated
  // m = 0 reduction (include/momcore.h, MOM_OPT_M0_REDUCTION): moment 0 runs as its own scene `sub` on the (I,Q) streams,
  // this scene's launches start at Fourier index m_first = 1
  momf_scene *sub = nullptr;
  int m_first = 0;
  bool opt_m0 = true, opt_pad = true;
  // operator-level API (mom_ops.hpp): added / surface / composite layers in the reference's [N,N,S] layout, allocated on first use
  MomDevBuf<float> op_added[6], op_surf[6], op_comp[6], op_vec[4], op_Z[2];
  MomDevBuf<float> blas_buf[4];  // mom_batch_inv / mom_batched_mul: A, C, B, generic-mode scratch (grow-only: batched_run)
  bool op_ready = false, op_comp_set = false;
  std::vector<double> hd_mu, hd_wt, hd_sg;  // the caller's Float64 streams (the sub-scene is cut from them)
  double hd_I0[4] = {}, hd_D[4] = {}, hd_mu0 = 0;
  hipStream_t stream = nullptr;  // borrowed from the Float64 handle (the sub-scene shares it), like d_info: never destroyed here
  int *d_info = nullptr;
  DevStreams q{};
  MomDevBuf<float> comp[6];
  bool pack = true;                       // MOM_OPT_SMALL_N = 1 (2: one point per wavefront)
  bool small_n = true;                    // MOM_OPT_SMALL_N: 4 < N <= 32 on the wave-per-point kernels (mom_wave.hip, Float32 build)
  int G = 1024;
  std::vector<float> h_mu;
  bool lds = true, force_generic = false, sweep = true, strips = true, w4 = true;  // w4: MOM_OPT_SMALL_WG
  hipEvent_t ev[4] = {};
  int launches = 0;
  std::string err;
};

// (every call of it is inlined now; the out-of-line copy stays in the library's dynamic symbol table, which does not change)
template hipError_t MomDevBuf<float>::reserve(size_t, hipStream_t);

#define FCHK(s, call)                                                                                         \
  do {                                                                                                        \
    hipError_t e__ = (call);                                                                                  \
    if (e__ != hipSuccess) {                                                                                  \
      char b__[384];                                                                                          \
      snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__);  \
      (s)->err = b__;                                                                                         \
      return MOM_EHIP;                                                                                        \
    }                                                                                                         \
  } while (0)

const char *momf_error(const momf_scene *s) { return s->err.c_str(); }

int momf_create(momf_scene **out, int device, hipStream_t stream, int N, int nS, int S, int max_m, int *d_info) {
  momf_scene *s = new momf_scene();
  *out = s;
  s->device = device; s->N = s->Nu = N; s->nS = nS; s->S = S; s->M = max_m; s->stream = stream; s->d_info = d_info;
  const int Nm = s->Nmax = strip_pad_f(N);
  s->lds = N <= 64;
  FCHK(s, hipSetDevice(device));
  FCHK(s, s->d_mu.renew(Nm));
  FCHK(s, s->d_wt.renew(Nm));
  FCHK(s, s->d_sg.renew(Nm));
  for (int k = 0; k < 6; ++k) {
    const size_t per = (k < 4) ? (size_t)comp_pitch(Nm) * Nm : (size_t)Nm;
    FCHK(s, s->comp[k].renew(per * S * max_m));
    FCHK(s, hipMemsetAsync(s->comp[k], 0, per * S * max_m * sizeof(float), stream));
  }
  const size_t scr = (size_t)s->G * kGenericBufs * mat_elems(Nm) + (size_t)ld_for(Nm) * np_for(Nm);
  FCHK(s, s->d_scratch.renew(scr));
  FCHK(s, hipMemsetAsync(s->d_scratch, 0, scr * sizeof(float), stream));
  for (int k = 0; k < 4; ++k) FCHK(s, hipEventCreate(&s->ev[k]));
  FCHK(s, hipStreamSynchronize(stream));
  return MOM_OK;
}

void momf_destroy(momf_scene *s) {
  if (!s) return;
  momf_destroy(s->sub);
  for (int k = 0; k < 4; ++k) if (s->ev[k]) (void)hipEventDestroy(s->ev[k]);
  delete s;  // frees the scene's device buffers (MomDevBuf members)
}

void momf_set_options(momf_scene *s, int inv_mode, int force_generic, int sweep, int small_n, int m0, int pad, int w4) {
  s->w4 = w4 != 0;
  s->small_n = small_n != 0;
  s->pack = small_n == 1;
  s->q.inv_mode = inv_mode;
  s->force_generic = force_generic != 0;
  s->lds = (s->N <= 64) && !s->force_generic;
  s->sweep = sweep != 0;
  s->opt_m0 = m0 != 0;
  s->opt_pad = pad != 0;
  if (s->sub) momf_set_options(s->sub, inv_mode, force_generic, sweep, small_n, 0, 0, w4);
}

int momf_set_streams(momf_scene *s, const double *mu, const double *wt, const double *sg, int imu0, double mu0,
                     const double *I0, const double *D, int regular) {
  const int Nu = s->Nu;
  s->hd_mu.assign(mu, mu + Nu); s->hd_wt.assign(wt, wt + Nu); s->hd_sg.assign(sg, sg + Nu);
  for (int k = 0; k < 4; ++k) { s->hd_I0[k] = (k < s->nS) ? I0[k] : 0.0; s->hd_D[k] = (k < s->nS) ? D[k] : 1.0; }
  s->hd_mu0 = mu0;
  DevStreams &q = s->q;
  for (int k = 0; k < 4; ++k) { q.I0[k] = (float)s->hd_I0[k]; q.D[k] = (float)s->hd_D[k]; }
  q.nS = s->nS; q.imu0 = imu0; q.mu0 = (float)mu0; q.regular = regular;
  // `regular` was decided on the Float64 streams; two distinct f64 nodes may round to one f32 value, which only makes
  // more stream pairs take the equal-mu branch of get_elem_rt! -- exactly what a Float32 reference run does
  return MOM_OK;
}

// The kernel edge and the device copies of the streams, at scene time (the options that decide the edge may be set after
// momf_set_streams): padded to a strip-chained image where one is within reach; edges up to 32 belong to the wave-per-point
// kernel, which takes the operators as they are
static int apply_streams(momf_scene *s) {
  const int Nu = s->Nu;
  if ((int)s->hd_mu.size() != Nu) { s->err = "Float32 scene: streams not set"; return MOM_ESTATE; }
  const int N = s->N = (s->opt_pad && !s->force_generic && !(Nu <= 32 && s->small_n)) ? strip_pad_f(Nu) : Nu;
  s->lds = (N <= 64) && !s->force_generic;
  std::vector<float> fm(s->hd_mu.begin(), s->hd_mu.end()), fw(s->hd_wt.begin(), s->hd_wt.end()), fs(s->hd_sg.begin(), s->hd_sg.end());
  fm.resize(N, 1.f); fw.resize(N, 0.f); fs.resize(N, 1.f);  // dummy entries
  s->h_mu = fm;
  FCHK(s, hipMemcpyAsync(s->d_mu, fm.data(), N * sizeof(float), hipMemcpyHostToDevice, s->stream));
  FCHK(s, hipMemcpyAsync(s->d_wt, fw.data(), N * sizeof(float), hipMemcpyHostToDevice, s->stream));
  FCHK(s, hipMemcpyAsync(s->d_sg, fs.data(), N * sizeof(float), hipMemcpyHostToDevice, s->stream));
  FCHK(s, hipStreamSynchronize(s->stream));
  s->q.mu = s->d_mu; s->q.wt = s->d_wt; s->q.sg = s->d_sg; s->q.N = N;
  return MOM_OK;
}

// the layer optics assembled on the device in Float64 (mom_scene_set_optics): rounded to the scene's Float32 there
__global__ void k_cvt_d2f(const double *src, float *dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)src[i];
}
static int convert_f(momf_scene *s, MomDevBuf<float> &dst, const double *d_src, size_t n) {
  FCHK(s, dst.renew(n));
  hipLaunchKernelGGL(k_cvt_d2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, d_src, dst.get(), n);
  FCHK(s, hipGetLastError());
  return MOM_OK;
}

static bool wave_applies_f32(const momf_scene *s);

static int scene_set_impl(momf_scene *s, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                          const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *tau_sum,
                          double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi, bool dev_layers);

int momf_scene_set(momf_scene *s, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                   const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *tau_sum,
                   double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi) {
  return scene_set_impl(s, Nz, K, M, tau, varpi, zw, Zpp, Zmp, ndoubl, iface, tau_sum, albedo, nVza, node, cos_mphi, sin_mphi, false);
}
// the same with tau, varpi, zw, tau_sum as DEVICE Float64 arrays (the device-side layer optics of mom_scene_set_optics)
int momf_scene_set_dev(momf_scene *s, int Nz, int K, int M, const double *d_tau, const double *d_varpi, const double *d_zw,
                       const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *d_tau_sum,
                       double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi) {
  return scene_set_impl(s, Nz, K, M, d_tau, d_varpi, d_zw, Zpp, Zmp, ndoubl, iface, d_tau_sum, albedo, nVza, node, cos_mphi, sin_mphi, true);
}

static int scene_set_impl(momf_scene *s, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                          const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *tau_sum,
                          double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi, bool dev_layers) {
  FCHK(s, hipSetDevice(s->device));
  int rc;
  if ((rc = apply_streams(s))) return rc;
  const int N = s->N, Nu = s->Nu, nS = s->nS;
  const size_t S = s->S, NN = (size_t)N * N;
  if (dev_layers) {
    if ((rc = convert_f(s, s->d_tau, tau, S * Nz))) return rc;
    if ((rc = convert_f(s, s->d_varpi, varpi, S * Nz))) return rc;
    if ((rc = convert_f(s, s->d_zw, zw, (size_t)K * S * Nz))) return rc;
    if ((rc = convert_f(s, s->d_tau_sum, tau_sum, S * (Nz + 1)))) return rc;
  } else {
    FCHK(s, mom_upload_as(s->d_tau, tau, S * Nz, s->stream));
    FCHK(s, mom_upload_as(s->d_varpi, varpi, S * Nz, s->stream));
    FCHK(s, mom_upload_as(s->d_zw, zw, (size_t)K * S * Nz, s->stream));
    FCHK(s, mom_upload_as(s->d_tau_sum, tau_sum, S * (Nz + 1), s->stream));
  }
  if (N == Nu) {
    FCHK(s, mom_upload_as(s->d_Zpp, Zpp, NN * K * M, s->stream));
    FCHK(s, mom_upload_as(s->d_Zmp, Zmp, NN * K * M, s->stream));
  } else {
    const std::vector<double> zp = mom_pad_blocks(Zpp, Nu, N, (size_t)K * M), zm = mom_pad_blocks(Zmp, Nu, N, (size_t)K * M);
    FCHK(s, mom_upload_as(s->d_Zpp, zp.data(), zp.size(), s->stream));
    FCHK(s, mom_upload_as(s->d_Zmp, zm.data(), zm.size(), s->stream));
  }
  FCHK(s, mom_upload_as(s->d_node, node, (size_t)nVza, s->stream));
  FCHK(s, mom_upload_as(s->d_cos, cos_mphi, (size_t)nVza * M, s->stream));
  FCHK(s, mom_upload_as(s->d_sin, sin_mphi, (size_t)nVza * M, s->stream));
  const size_t nout = (size_t)nVza * nS * S;
  FCHK(s, s->d_R.renew(2 * nout));
  s->d_T = s->d_R + nout;
  FCHK(s, s->d_hdr.renew(nout));
  FCHK(s, s->d_hdrJ.renew((size_t)N * S));
  FCHK(s, s->d_bhr_uw.renew((size_t)nS * S));
  FCHK(s, s->d_bhr_dw.renew((size_t)nS * S));
  s->Nz = Nz; s->K = K; s->scene_M = M; s->nVza = nVza; s->albedo = (float)albedo; s->surf_kind = 0;
  s->nd.assign(ndoubl, ndoubl + Nz);
  s->iface.assign(iface, iface + Nz);
  // ---- m = 0 reduction (include/momcore.h): the data test and the cut are the Float64 driver's (mom_reduce.hpp).
  // Scenes that run on the lane- or wave-per-point kernels (all moments in one launch) keep moment 0 there.
  s->m_first = 0;
  const bool ok = s->opt_m0 && nS >= 3 && s->q.regular && !(Nu <= 4 && s->small_n) && !wave_applies_f32(s) &&
                  mom_m0_reducible(s->hd_I0, Nu, nS, K, Zpp, Zmp);
  if (!ok) {
    momf_destroy(s->sub);
    s->sub = nullptr;
    return MOM_OK;
  }
  // N0r real entries; the kernels run on N0 >= N0r (dummy entries at the end) unless the wave-per-point kernel takes the scene
  const int nS0 = kMomM0Stokes, N0r = mom_m0_edge(Nu, nS);
  const int N0 = (s->opt_pad && !s->force_generic && !(N0r <= 32 && s->small_n)) ? strip_pad_f(N0r) : N0r;
  if (s->sub && !(s->sub->Nu == N0 && s->sub->S == s->S)) { momf_destroy(s->sub); s->sub = nullptr; }
  if (!s->sub) {
    if ((rc = momf_create(&s->sub, s->device, s->stream, N0, nS0, s->S, 1, s->d_info))) {
      s->err = s->sub->err;
      momf_destroy(s->sub);
      s->sub = nullptr;
      return rc;
    }
  }
  momf_scene *u = s->sub;
  momf_set_options(u, s->q.inv_mode, s->force_generic, s->sweep, s->small_n, 0, 0, s->w4);
  u->strips = s->strips;
  const MomM0Cut cut = mom_m0_cut(s->hd_mu.data(), s->hd_wt.data(), Nu, nS, K, N0, Zpp, Zmp);
  const double one[4] = {1.0, 1.0, 1.0, 1.0};
  auto sub_fail = [&](int code) { s->err = u->err; return code; };
  if ((rc = momf_set_streams(u, cut.mu.data(), cut.wt.data(), cut.sg.data(), s->q.imu0, s->hd_mu0, s->hd_I0, one, s->q.regular)))
    return sub_fail(rc);
  if ((rc = scene_set_impl(u, Nz, K, 1, tau, varpi, zw, cut.Zpp.data(), cut.Zmp.data(), ndoubl, iface, tau_sum, albedo, nVza, node, cos_mphi,
                           sin_mphi, dev_layers)))
    return sub_fail(rc);
  s->m_first = 1;
  return MOM_OK;
}

int momf_scene_set_surface(momf_scene *s, int kind, int M, const double *Rsurf, const double *albedo_spec) {
  FCHK(s, hipSetDevice(s->device));
  const int N = s->N, Nu = s->Nu, nS = s->nS;
  int rc;
  if (kind == 1) {
    if (N == Nu) {
      FCHK(s, mom_upload_as(s->d_Rsurf, Rsurf, (size_t)N * N * M, s->stream));
    } else {
      const std::vector<double> rp = mom_pad_blocks(Rsurf, Nu, N, (size_t)M);
      FCHK(s, mom_upload_as(s->d_Rsurf, rp.data(), rp.size(), s->stream));
    }
    FCHK(s, s->d_hdrJm.renew((size_t)N * s->S * M));
    if (s->m_first) {
      // moment 0 runs on the (I,Q) sub-scene: its surface matrix must not couple (I,Q) with (U,V) either
      std::vector<double> r0;
      if (!mom_m0_cut_brdf(Rsurf, Nu, nS, s->sub->Nu, r0)) { s->err = kMomM0BrdfCouples; return MOM_EINVAL; }
      if ((rc = momf_scene_set_surface(s->sub, 1, 1, r0.data(), nullptr))) { s->err = s->sub->err; return rc; }
    }
  } else if (kind == 2) {
    FCHK(s, mom_upload_as(s->d_albedo_spec, albedo_spec, (size_t)s->S, s->stream));
    if (s->m_first && (rc = momf_scene_set_surface(s->sub, 2, 1, nullptr, albedo_spec))) { s->err = s->sub->err; return rc; }
  } else if (s->m_first) {
    s->sub->surf_kind = 0;
  }
  s->surf_kind = kind;
  return MOM_OK;
}

// momcore_strip.hip built for float (Makefile: momcore_fs<KS>.o, 8 waves; momcore_f4s<KS>.o, 4 waves): mom_images.hpp

// 4 < N <= 32: one spectral point per wavefront, operators in MFMA-layout registers, the whole run in ONE launch -- the
// Float32 build of momw::k_wsweep (the Float64 path: rt_run_wave in mom_scene.hip; what the two share: mom_host.hpp).  The
// "too many layers" refusals of the two runs: an artefact of d_ndif's fixed allocation here, kept as it is
static bool wave_applies_f32(const momf_scene *s) { return mom_wave_sweep_applies(*s, s->N, s->nS, s->small_n, s->force_generic); }
static int rt_run_wave_f32(momf_scene *s) {
  if (!s->d_ndif) FCHK(s, s->d_ndif.renew(kMaxSweepLayers * 4));
  if (s->Nz > kMaxSweepLayers * 4) { s->err = "Float32 wave sweep: too many layers"; return MOM_EINVAL; }
  FCHK(s, hipMemcpyAsync(s->d_ndif, s->nd.data(), sizeof(int) * s->Nz, hipMemcpyHostToDevice, s->stream));
  MomWaveSweepArgsF a{};
  mom_fill_wave_args(a, *s, s->q, s->S, s->d_info, s->pack);
  FCHK(s, hipEventRecord(s->ev[0], s->stream));
  FCHK(s, momwf_launch_sweep(&a, s->stream));
  for (int k = 1; k < 4; ++k) FCHK(s, hipEventRecord(s->ev[k], s->stream));
  FCHK(s, hipStreamSynchronize(s->stream));  // s->nd may be rewritten by the next scene_set
  s->launches = 1;
  return MOM_OK;
}

// N <= 4: one spectral point per lane, the whole run in ONE launch (the Float64 path: rt_run_small in mom_scene.hip)
static int rt_run_small_f32(momf_scene *s) {
  const int Nz = s->Nz;
  if (!s->d_smtab) FCHK(s, s->d_smtab.renew(48));
  if (!s->d_ndif) FCHK(s, s->d_ndif.renew(kMaxSweepLayers * 4));
  if (2 * Nz > kMaxSweepLayers * 4) { s->err = "Float32 lane sweep: too many layers"; return MOM_EINVAL; }
  float tab[48];
  mom_small_tables(s->h_mu.data(), s->N, tab);
  FCHK(s, hipMemcpyAsync(s->d_smtab, tab, sizeof tab, hipMemcpyHostToDevice, s->stream));
  std::vector<int> v(s->nd);
  v.insert(v.end(), s->iface.begin(), s->iface.end());
  FCHK(s, hipMemcpyAsync(s->d_ndif, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
  FCHK(s, hipStreamSynchronize(s->stream));
  MomSmallSweepArgsF a{};
  FCHK(s, mom_fill_small_args(a, *s, s->q, s->S, s->d_info, s->pack, s->stream));
  FCHK(s, hipEventRecord(s->ev[0], s->stream));
  FCHK(s, momsmf_launch_sweep(&a, s->N, s->stream));
  for (int k = 1; k < 4; ++k) FCHK(s, hipEventRecord(s->ev[k], s->stream));
  s->launches = 1;
  return MOM_OK;
}

int momf_rt_run(momf_scene *s) {
  FCHK(s, hipSetDevice(s->device));
  if (s->N <= 4 && s->small_n && !s->force_generic && s->nVza <= 4 && s->surf_kind == 0 && s->K <= 4) return rt_run_small_f32(s);
  if (wave_applies_f32(s)) return rt_run_wave_f32(s);
  const size_t S = s->S;
  const int N = s->N, Nz = s->Nz;
  const int m_first = s->m_first, M = s->scene_M - m_first;  // this scene's own moments: m_first ... s->scene_M - 1
  const bool lds = s->lds;
  const size_t sm = lds_bytes(N, lds);
  s->launches = 0;
  bool can_sweep = s->sweep && Nz <= kMaxSweepLayers && Nz > 1;
  for (int z = 2; z < Nz && can_sweep; ++z) can_sweep = (s->iface[z] == s->iface[1]);
  for (int z = 0; z < Nz && can_sweep; ++z) can_sweep = (s->nd[z] <= 127);
  FCHK(s, hipEventRecord(s->ev[0], s->stream));
  if (m_first) {  // moment 0 on the (I,Q) sub-scene (same stream: in order with what follows)
    const int rc = momf_rt_run(s->sub);
    if (rc) { s->err = s->sub->err; return rc; }
    s->launches += s->sub->launches;
    FCHK(s, hipSetDevice(s->device));
  }
  for (int z = (can_sweep ? -1 : 0); z < (can_sweep ? 0 : Nz) && M > 0; ++z) {
    LayerArgs a{};
    a.q = s->q; a.S = s->S; a.M = M; a.K = s->K; a.m_first = m_first;
    int zz = z;
    if (z < 0) {
      zz = 0;
      a.Nz_sweep = Nz;
      for (int k = 0; k < Nz; ++k) { a.nd_z[k] = (signed char)s->nd[k]; a.iface_z[k] = (signed char)s->iface[k]; }
      a.nd = s->nd[0]; a.iface = s->iface[1]; a.first = 1;
    } else {
      a.nd = s->nd[z]; a.iface = s->iface[z]; a.first = (z == 0);
    }
    a.tau = s->d_tau + S * zz; a.varpi = s->d_varpi + S * zz; a.zw = s->d_zw + (size_t)s->K * S * zz;
    a.tau_sum = s->d_tau_sum + S * zz;
    a.Zpp = s->d_Zpp + (size_t)N * N * s->K * m_first; a.Zmp = s->d_Zmp + (size_t)N * N * s->K * m_first;
    for (int k = 0; k < 6; ++k) a.comp[k] = s->comp[k];
    a.scratch = s->d_scratch; a.info = s->d_info;
    const int grid = lds ? (int)((S >= 2048) ? S : S * M) : (int)std::min<size_t>(S * M, (size_t)s->G);
    // strip-chained images (Float32 builds of mom_strip.hpp's chains) for the edges that have one; MOM_OPT_INVERSE != 0 keeps
    // the general path inside the same image, MOM_OPT_STRIPS_F32 = 0 (s->strips) the general image
    // 4-wave images (N = 36, 40 have no other): two workgroups per CU
    const MomLayerImage *im = (lds && s->strips && s->w4) ? mom_find_image(MOM_IMG_F32_STRIP4, N) : nullptr;
    if (!im && lds && s->strips) im = mom_find_image(MOM_IMG_F32_STRIP8, N);
    if (im) {
      FCHK(s, im->launch(&a, MomLaunchForm{}, grid, s->stream));
      s->launches++;
      continue;
    }
#define F32_LAUNCH(IF) FCHK(s, mom_launch_ldsm(MOM_LDSM(k_layer, IF), lds, grid, kThreads, sm, s->stream, a))
    MOM_IFACE_SWITCH(a.iface, F32_LAUNCH)
#undef F32_LAUNCH
    s->launches++;
  }
  FCHK(s, hipEventRecord(s->ev[1], s->stream));
  // surface: every moment of a BRDF surface, moment 0 only otherwise (m > 0: r = 0, t = I, j = 0 -- the interaction is the identity)
  for (int m = m_first; m < ((s->surf_kind == 1) ? s->scene_M : 1); ++m) {
    SurfArgs a{};
    a.q = s->q; a.S = s->S; a.iface = s->iface[Nz - 1];
    a.albedo = s->albedo; a.tau_tot = s->d_tau_sum + S * Nz;
    a.kind = s->surf_kind; a.m = m; a.albedo_spec = s->d_albedo_spec;
    a.Rsurf = (s->surf_kind == 1) ? s->d_Rsurf + (size_t)N * N * m : nullptr;
    for (int k = 0; k < 6; ++k)
      a.comp[k] = s->comp[k] + ((k < 4) ? (size_t)comp_pitch(N) * N : (size_t)N) * S * (m - m_first);
    a.hdrJ = (m == 0) ? s->d_hdrJ : s->d_hdrJm + (size_t)N * S * m;
    a.bhr_uw = s->d_bhr_uw; a.bhr_dw = s->d_bhr_dw; a.nS_out = s->nS;
    a.scratch = s->d_scratch; a.info = s->d_info;
    const int grid = lds ? (int)S : (int)std::min<size_t>(S, (size_t)s->G);
    FCHK(s, mom_launch_ldsm(MOM_LDSM(k_surface), lds, grid, kThreads, sm, s->stream, a));
  }
  FCHK(s, hipEventRecord(s->ev[2], s->stream));
  {
    const size_t total = (size_t)s->nVza * s->nS * S;
    PostArgsF pa{};
    pa.N = N; pa.nS = s->nS; pa.S = s->S; pa.M = M; pa.nVza = s->nVza; pa.m_first = m_first;
    pa.hdr_all = (s->surf_kind == 1); pa.zeroT_hi = (s->surf_kind == 2);
    pa.node = s->d_node; pa.cos_mphi = s->d_cos; pa.sin_mphi = s->d_sin;
    pa.J0p = s->comp[4]; pa.J0m = s->comp[5]; pa.hdrJ0 = s->d_hdrJ; pa.hdrJm = s->d_hdrJm;
    pa.R = s->d_R; pa.T = s->d_T; pa.hdr = s->d_hdr;
    hipLaunchKernelGGL(k_postprocess_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s->stream, pa);
    FCHK(s, hipGetLastError());
    if (m_first) {
      const momf_scene *u = s->sub;
      CombineArgsF ca{s->nVza, s->nS, u->nS, s->S, s->d_R, s->d_T, s->d_hdr, s->d_bhr_uw, s->d_bhr_dw,
                      u->d_R, u->d_T, u->d_hdr, u->d_bhr_uw, u->d_bhr_dw};
      const size_t tot2 = std::max(total, (size_t)s->nS * S);
      hipLaunchKernelGGL(k_combine_m0_f32, dim3((unsigned)((tot2 + 255) / 256)), dim3(256), 0, s->stream, ca);
      FCHK(s, hipGetLastError());
    }
  }
  FCHK(s, hipEventRecord(s->ev[3], s->stream));
  return MOM_OK;
}

int momf_get_RT(momf_scene *s, double *R, double *T) {
  FCHK(s, hipSetDevice(s->device));
  FCHK(s, mom_download_RT(*s, s->nS, s->S, R, T, s->stream));
  return MOM_OK;
}
int momf_get_hdr(momf_scene *s, double *hdr, double *up, double *dw) {
  FCHK(s, hipSetDevice(s->device));
  FCHK(s, mom_download_hdr(*s, s->nS, s->S, hdr, up, dw, s->stream));
  return MOM_OK;
}

int momf_timers(momf_scene *s, double *ms, int *launches) {
  FCHK(s, hipSetDevice(s->device));
  FCHK(s, mom_stage_times(s->ev, ms));
  *launches = s->launches;
  return MOM_OK;
}

// batch_inv!(X, A) / A ⊠ B on a Float32 handle: Float64 host arrays at the ABI, f32 on the device (batched_run, mom_ops.hpp)
int momf_blas(momf_scene *s, int n, int batch, const double *A, const double *B, double *C, bool inv) {
  FCHK(s, hipSetDevice(s->device));
  FCHK(s, batched_run(s->stream, s->blas_buf, s->d_info, s->force_generic, n, batch, A, B, C, inv));
  return MOM_OK;
}

// =========================================================================================
// operator-level API on a Float32 handle: Float64 host arrays at the ABI (rounded on upload, widened on download), the
// kernels of mom_ops.hpp in namespace momf.  The operators run on the caller's edge (no padding) and their own layer arrays.
// =========================================================================================
static int op_begin(momf_scene *s, DevStreams *q) {
  FCHK(s, hipSetDevice(s->device));
  const int N = s->Nu;
  if ((int)s->hd_mu.size() != N) { s->err = "operator-level call: streams not set"; return MOM_ESTATE; }
  if (!s->op_ready) {
    const size_t NN = (size_t)N * N;
    for (int k = 0; k < 6; ++k) {
      const size_t per = ((k < 4) ? NN : (size_t)N) * s->S;
      FCHK(s, s->op_added[k].renew(per));
      FCHK(s, s->op_surf[k].renew(per));
      FCHK(s, s->op_comp[k].renew(per));
      FCHK(s, hipMemsetAsync(s->op_added[k], 0, per * sizeof(float), s->stream));
      FCHK(s, hipMemsetAsync(s->op_surf[k], 0, per * sizeof(float), s->stream));
      FCHK(s, hipMemsetAsync(s->op_comp[k], 0, per * sizeof(float), s->stream));
    }
    for (int k = 0; k < 4; ++k) FCHK(s, s->op_vec[k].renew((size_t)s->S));
    s->op_ready = true;
  }
  // the caller's streams (a scene on this handle may have padded the device copies BEHIND entry Nu - 1; rewritten here anyway)
  FCHK(s, mom_to_device<float>(s->d_mu, s->hd_mu.data(), N, s->stream));
  FCHK(s, mom_to_device<float>(s->d_wt, s->hd_wt.data(), N, s->stream));
  FCHK(s, mom_to_device<float>(s->d_sg, s->hd_sg.data(), N, s->stream));
  *q = s->q;
  q->mu = s->d_mu; q->wt = s->d_wt; q->sg = s->d_sg; q->N = N;
  return MOM_OK;
}
#define OP_UP(s, dst, src, n) FCHK(s, mom_to_device<float>(dst, src, n, (s)->stream))
#define OP_DOWN(s, dst, src, n) FCHK(s, mom_to_host<float>(dst, src, n, (s)->stream))
#define OP_LAUNCH(s, KERN, grid, args)                                                                       \
  do {                                                                                                       \
    const bool l__ = (s)->Nu <= 64 && !(s)->force_generic;                                                   \
    FCHK(s, mom_launch_ldsm(MOM_LDSM(KERN), l__, grid, kThreads, lds_bytes((s)->Nu, l__), (s)->stream, args)); \
  } while (0)
static int op_grid(const momf_scene *s) {
  return (s->Nu <= 64 && !s->force_generic) ? s->S : (int)std::min<size_t>((size_t)s->S, (size_t)s->G);
}

int momf_op_elemental(momf_scene *s, int m, int nd, const double *tau_sum, const double *dtau, const double *varpi,
                      const double *Zpp, const double *Zmp, int z_batch) {
  OpArgs a{};
  int rc;
  if ((rc = op_begin(s, &a.q))) return rc;
  const size_t zc = (size_t)s->Nu * s->Nu * z_batch;
  for (int k = 0; k < 2; ++k) FCHK(s, s->op_Z[k].reserve(zc, s->stream));
  OP_UP(s, s->op_vec[0], tau_sum, s->S);
  OP_UP(s, s->op_vec[1], dtau, s->S);
  OP_UP(s, s->op_vec[2], varpi, s->S);
  OP_UP(s, s->op_Z[0], Zpp, zc);
  OP_UP(s, s->op_Z[1], Zmp, zc);
  a.S = s->S; a.m = m; a.nd = nd; a.z_batch = z_batch;
  a.tau_sum = s->op_vec[0]; a.dtau = s->op_vec[1]; a.varpi = s->op_vec[2]; a.Zpp = s->op_Z[0]; a.Zmp = s->op_Z[1];
  for (int k = 0; k < 6; ++k) a.added[k] = s->op_added[k];
  a.scratch = s->d_scratch; a.info = s->d_info;
  OP_LAUNCH(s, k_op_elemental, op_grid(s), a);
  FCHK(s, hipStreamSynchronize(s->stream));
  return MOM_OK;
}

int momf_op_doubling(momf_scene *s, int nd, double *expk) {
  OpArgs a{};
  int rc;
  if ((rc = op_begin(s, &a.q))) return rc;
  OP_UP(s, s->op_vec[3], expk, s->S);
  a.S = s->S; a.nd = nd; a.expk = s->op_vec[3];
  for (int k = 0; k < 6; ++k) a.added[k] = s->op_added[k];
  a.scratch = s->d_scratch; a.info = s->d_info;
  if (nd > 0) OP_LAUNCH(s, k_op_doubling, op_grid(s), a);  // doubling.jl:28 returns early for 0
  OP_DOWN(s, expk, s->op_vec[3], s->S);
  return MOM_OK;
}

int momf_op_interaction(momf_scene *s, int iface, int with_surface_layer) {
  OpArgs a{};
  int rc;
  if ((rc = op_begin(s, &a.q))) return rc;
  if (!s->op_comp_set) {
    s->err = "mom_interaction: start the operator-level sequence with mom_copy_added_to_composite or mom_upload";
    return MOM_ESTATE;
  }
  a.S = s->S; a.iface = iface;
  for (int k = 0; k < 6; ++k) { a.added[k] = with_surface_layer ? s->op_surf[k] : s->op_added[k]; a.comp[k] = s->op_comp[k]; }
  a.scratch = s->d_scratch; a.info = s->d_info;
  OP_LAUNCH(s, k_op_interaction, op_grid(s), a);
  FCHK(s, hipStreamSynchronize(s->stream));
  return MOM_OK;
}

int momf_op_copy_added_to_composite(momf_scene *s) {
  DevStreams q;
  int rc;
  if ((rc = op_begin(s, &q))) return rc;
  const size_t NN = (size_t)s->Nu * s->Nu;
  const int src[6] = {1, 0, 3, 2, 4, 5};  // composite order R_mp, R_pm, T_pp, T_mm, J0p, J0m ; added order r_pm, r_mp, t_mm, t_pp, j0p, j0m
  for (int k = 0; k < 6; ++k) {
    const size_t bytes = ((k < 4) ? NN : (size_t)s->Nu) * s->S * sizeof(float);
    FCHK(s, hipMemcpyAsync(s->op_comp[k], s->op_added[src[k]], bytes, hipMemcpyDeviceToDevice, s->stream));
  }
  FCHK(s, hipStreamSynchronize(s->stream));
  s->op_comp_set = true;
  return MOM_OK;
}

int momf_op_surface_lambertian(momf_scene *s, int m, double albedo, const double *tau_tot) {
  DevStreams q;
  int rc;
  if ((rc = op_begin(s, &q))) return rc;
  OP_UP(s, s->op_vec[0], tau_tot, s->S);
  hipLaunchKernelGGL(k_op_surface_fill, dim3(s->S), dim3(256), 0, s->stream, q, s->S, m, (float)albedo, s->op_vec[0], s->op_surf[0],
                     s->op_surf[1], s->op_surf[2], s->op_surf[3], s->op_surf[4], s->op_surf[5]);
  FCHK(s, hipGetLastError());
  FCHK(s, hipStreamSynchronize(s->stream));
  return MOM_OK;
}

static float *op_which(momf_scene *s, int which, size_t *count) {
  const int grp = which / 6, k = which % 6;
  *count = ((k < 4) ? (size_t)s->Nu * s->Nu : (size_t)s->Nu) * s->S;
  return grp == 0 ? s->op_added[k] : (grp == 1 ? s->op_comp[k] : s->op_surf[k]);
}
int momf_op_upload(momf_scene *s, int which, const double *src) {
  DevStreams q;
  int rc;
  if ((rc = op_begin(s, &q))) return rc;
  size_t count = 0;
  float *p = op_which(s, which, &count);
  if (which / 6 == 1) s->op_comp_set = true;
  OP_UP(s, p, src, count);
  return MOM_OK;
}
int momf_op_download(momf_scene *s, int which, double *dst) {
  DevStreams q;
  int rc;
  if ((rc = op_begin(s, &q))) return rc;
  if (which / 6 == 1 && !s->op_comp_set) {
    s->err = "mom_download: a Float32 handle keeps the operator-level composite layer apart from the scene-level state; start "
             "the operator-level sequence with mom_copy_added_to_composite or mom_upload";
    return MOM_ESTATE;
  }
  size_t count = 0;
  float *p = op_which(s, which, &count);
  OP_DOWN(s, dst, p, count);
  return MOM_OK;
}
