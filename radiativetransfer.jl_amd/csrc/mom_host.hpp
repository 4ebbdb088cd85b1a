// mom_host.hpp -- host-side helpers shared by the translation units of libmomcore.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "momcore.h"

// The one owner of a device allocation of the handles (mom_handle, momf_scene): pointer + capacity in elements of T, freed by
// the destructor.  A member that is not a MomDevBuf (an alias into one, a pointer borrowed from another handle) is never freed.
// After a failed call the buffer is empty, so an error return between two allocations leaves each buffer valid or empty.
template <class T>
class MomDevBuf {
 public:
  MomDevBuf() = default;
  MomDevBuf(const MomDevBuf &) = delete;
  MomDevBuf &operator=(const MomDevBuf &) = delete;
  MomDevBuf(MomDevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  MomDevBuf &operator=(MomDevBuf &&o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~MomDevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // exactly max(count, 1) elements, fresh: what is held is freed first (the caller knows no work in flight uses it)
  hipError_t renew(size_t count) {
    reset();
    count = std::max<size_t>(count, 1);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T));
    if (e == hipSuccess) cap_ = count;
    else p_ = nullptr;
    return e;
  }
  // grow-only, at least `count` elements: no call into the runtime in steady state; before a buffer that is too small is
  // freed, the stream it was last used on (`st`) is drained
  hipError_t reserve(size_t count, hipStream_t st) {
    if (count <= cap_) return hipSuccess;
    const hipError_t e = p_ ? hipStreamSynchronize(st) : hipSuccess;
    reset();
    return e != hipSuccess ? e : renew(count);
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

// host array -> a buffer of exactly `count` elements; the copy is asynchronous on `st` (src must outlive it)
template <class T>
inline hipError_t mom_upload(MomDevBuf<T> &dst, const T *src, size_t count, hipStream_t st) {
  const hipError_t e = dst.renew(count);
  return e != hipSuccess ? e : hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, st);
}
// the same through a staging vector of T (double -> float, int -> int); `st` is drained before the vector dies
template <class T, class U>
inline hipError_t mom_upload_as(MomDevBuf<T> &dst, const U *src, size_t count, hipStream_t st) {
  std::vector<T> v(count);
  for (size_t i = 0; i < count; ++i) v[i] = (T)src[i];
  const hipError_t e = mom_upload(dst, v.data(), count, st), e2 = hipStreamSynchronize(st);
  return e != hipSuccess ? e : e2;
}
#pragma GCC visibility push(hidden)  // what follows is internal to libmomcore.so: the exports of the library are the C ABI's
// The C ABI's Float64 host arrays <-> device memory of the handle's precision, into memory that exists.  double: the copy itself,
// asynchronous on `st`.  float: rounded / widened through a staging vector, `st` drained before it dies.
template <class Real>
inline hipError_t mom_to_device(Real *dst, const double *src, size_t n, hipStream_t st) {
  if constexpr (std::is_same<Real, double>::value) {
    return hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, st);
  } else {
    const std::vector<Real> v(src, src + n);
    const hipError_t e = hipMemcpyAsync(dst, v.data(), n * sizeof(Real), hipMemcpyHostToDevice, st), e2 = hipStreamSynchronize(st);
    return e != hipSuccess ? e : e2;
  }
}
template <class Real>
inline hipError_t mom_to_host(double *dst, const Real *src, size_t n, hipStream_t st) {
  if constexpr (std::is_same<Real, double>::value) {
    return hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, st);
  } else {
    std::vector<Real> v(n);
    const hipError_t e = hipMemcpyAsync(v.data(), src, n * sizeof(Real), hipMemcpyDeviceToHost, st), e2 = hipStreamSynchronize(st);
    std::copy(v.begin(), v.end(), dst);
    return e != hipSuccess ? e : e2;
  }
}

// The resident scene of a handle, ONE declaration for both precisions: mom_handle derives from MomSceneBufs<double>, momf_scene from
// MomSceneBufs<float>, and what both drivers do with a scene (the single-launch runs' argument blocks, the getters: below) reads
// these names.  The azimuthal weights stay Float64 in both (the reference's host-side `bigCS`).
template <class Real>
struct MomSceneBufs {
  int Nz = 0, K = 0, nVza = 0, scene_M = 0;  // scene_M: Fourier moments of the resident scene (<= the handle's M)
  int surf_kind = 0;                         // 0 Lambertian scalar, 1 BRDF matrices, 2 Lambertian Legendre (mom_scene_set_surface)
  Real albedo = 0;
  std::vector<int> nd, iface;
  MomDevBuf<Real> d_mu, d_wt, d_sg;
  MomDevBuf<Real> d_tau, d_varpi, d_zw, d_tau_sum, d_Zpp, d_Zmp;
  MomDevBuf<double> d_cos, d_sin;
  MomDevBuf<int> d_node;
  MomDevBuf<Real> d_R, d_hdr, d_hdrJ, d_hdrJm, d_bhr_uw, d_bhr_dw;
  Real *d_T = nullptr;  // d_R + nVza nS S: R_SFI || T_SFI are ONE buffer (the all-gather's send buffer as it stands)
  MomDevBuf<Real> d_Rsurf, d_albedo_spec;
  MomDevBuf<Real> d_smtab;   // N <= 4: F1 | F2 | SI tables [3][N,N] of the lane-per-point kernel
  MomDevBuf<Real> d_smpart;  // ... one (point, moment) per lane: the per-moment terms of R_SFI / T_SFI [M][2][nVza,nS,S]
  MomDevBuf<int> d_ndif;     // ndoubl | iface [2][Nz] of the single-launch runs
  MomDevBuf<Real> d_scratch;
};

// R / T and hdr / BHR of the resident scene into the caller's Float64 arrays (S spectral points, nS Stokes components)
template <class Real>
inline hipError_t mom_download_RT(const MomSceneBufs<Real> &b, int nS, int S, double *R, double *T, hipStream_t st) {
  const size_t nout = (size_t)b.nVza * nS * S;
  const hipError_t e = mom_to_host(R, b.d_R.get(), nout, st);
  return e != hipSuccess ? e : mom_to_host(T, b.d_T, nout, st);
}
template <class Real>
inline hipError_t mom_download_hdr(const MomSceneBufs<Real> &b, int nS, int S, double *hdr, double *up, double *dw, hipStream_t st) {
  hipError_t e = mom_to_host(hdr, b.d_hdr.get(), (size_t)b.nVza * nS * S, st);
  if (e == hipSuccess) e = mom_to_host(up, b.d_bhr_uw.get(), (size_t)nS * S, st);
  return e != hipSuccess ? e : mom_to_host(dw, b.d_bhr_dw.get(), (size_t)nS * S, st);
}

// the four stage times of a run from its events ev[0..3]: layers, surface, post-processing, total (ms)
inline hipError_t mom_stage_times(const hipEvent_t *ev, double *ms) {
  hipError_t e = hipEventSynchronize(ev[3]);
  const int from[4] = {0, 1, 2, 0}, to[4] = {1, 2, 3, 3};
  for (int k = 0; k < 4 && e == hipSuccess; ++k) {
    float t = 0.f;
    e = hipEventElapsedTime(&t, ev[from[k]], ev[to[k]]);
    ms[k] = t;
  }
  return e;
}
#pragma GCC visibility pop

// Scene-level path: an operator edge N for which no strip-chained kernel image exists is padded with up to 4 DUMMY
// STREAM ENTRIES (mu = 1, weight 0, zero rows and columns in every phase-matrix basis and BRDF matrix) when that
// reaches a size one exists for: most IQU stream counts (N = 3 k is a multiple of 4 only for every fourth k), and
// N = 32, 48 (measured: N = 48 as 52 runs 1.3x faster than the general path at 48).  A dummy entry is decoupled exactly:
// its column is zero in r and off-diagonal in t (zero weight, elemental.jl:198-205), its row is zero because its Z row
// is, so every product, series and pivoted inverse leaves the real rows and columns with the same terms plus exact zeros.
// `strip_size`: the edges that have a strip-chained finisher in the driver's precision (the image table, mom_images.hpp)
constexpr int kMomPadMax = 4;
inline int mom_strip_pad(bool (*strip_size)(int), int N) {
  if (strip_size(N)) return N;
  for (int p = N + 1; p <= N + kMomPadMax; ++p)
    if (strip_size(p)) return p;
  return N;
}
// Zero-weight streams come last in a stream set: the view angles and the Sun behind the Gauss nodes, the dummy entries behind
// them.  mom_weighted_edge: the entries in front of the trailing run of weights that are EXACTLY 0.0 (a zero between weighted
// entries ends the run); mom_q4_nbw: the blocks of four entries that hold one of them, at least 1 -- from block nbw on every entry is
// a zero-weight stream, whose column the elemental layer writes as r = 0, t = its diagonal entry (mom_kernels.hpp: weight <= 1e-8)
inline int mom_weighted_edge(const double *wt, int N) {
  int n = N;
  while (n > 0 && wt[n - 1] == 0.0) --n;
  return n;
}
inline int mom_q4_nbw(const double *wt, int N) { return std::max(1, (mom_weighted_edge(wt, N) + 3) / 4); }
// [N,N,B] -> [Nk,Nk,B], zero padded
inline std::vector<double> mom_pad_blocks(const double *src, int N, int Nk, size_t B) {
  std::vector<double> out((size_t)Nk * Nk * B, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < N; ++i) out[i + (size_t)Nk * (j + (size_t)Nk * b)] = src[i + (size_t)N * (j + (size_t)N * b)];
  return out;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is set once per (device, kernel image) and raised only when a
// larger LDS image is requested -- not on every launch.
inline hipError_t mom_allow_lds(const void *fn, size_t bytes) {
  static thread_local std::map<std::pair<int, const void *>, size_t> granted;
  int dev = 0;
  (void)hipGetDevice(&dev);
  size_t &g = granted[std::make_pair(dev, fn)];
  if (bytes <= g) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) g = bytes;
  return e;
}

// A run-time value as a template argument: `f` is a generic lambda and receives a std::integral_constant, which converts to its
// value in constant expressions; what `f` returns (a launch's hipError_t, a kernel's function pointer) comes back.  mom_with_int
// covers Lo ... Hi and refuses the rest (hipErrorInvalidValue, or a null pointer), so nothing outside that range is instantiated.
template <class F>
inline auto mom_with_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <int Lo, int Hi, class F>
inline auto mom_with_int(int v, F &&f) -> decltype(f(std::integral_constant<int, Lo>{})) {
  using R = decltype(f(std::integral_constant<int, Lo>{}));
  if (v == Lo) return f(std::integral_constant<int, Lo>{});
  if constexpr (Lo < Hi) return mom_with_int<Lo + 1, Hi>(v, f);
  else if constexpr (std::is_same<R, hipError_t>::value) return hipErrorInvalidValue;
  else return R{};
}

// One launch of a kernel with `smem` bytes of dynamic LDS
template <class Args>
inline hipError_t mom_launch_lds(void (*k)(Args), int grid, int threads, size_t smem, hipStream_t st, const Args &a) {
  const hipError_t e = mom_allow_lds(reinterpret_cast<const void *>(k), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(grid), dim3(threads), smem, st, a);
  return hipGetLastError();
}
// ... of a kernel templated on LDSM (operators in LDS / in per-workgroup global slabs): `k_lds` and `k_gen` are its two
// instantiations, MOM_LDSM(KERN, further template arguments...) names them
template <class Args>
inline hipError_t mom_launch_ldsm(void (*k_lds)(Args), void (*k_gen)(Args), bool lds, int grid, int threads, size_t smem,
                                  hipStream_t st, const Args &a) {
  return mom_launch_lds(lds ? k_lds : k_gen, grid, threads, smem, st, a);
}
#define MOM_LDSM(KERN, ...) KERN<true, ##__VA_ARGS__>, KERN<false, ##__VA_ARGS__>

// The interface code is a template argument of the layer kernels (see interaction_core): STMT(IF) for IF = iface, codes
// outside 0..2 taking the image of code 3
#define MOM_IFACE_SWITCH(iface, STMT) \
  switch (iface) {                    \
    case 0: STMT(0); break;           \
    case 1: STMT(1); break;           \
    case 2: STMT(2); break;           \
    default: STMT(3); break;          \
  }

// text for mom_last_global_error() (the thread's library-level error string, momcore.hip)
void mom_set_global_error(const char *msg);

// The absorption model as the line-shape kernels' shape (voigt.hip LineShape): 0 Voigt / HW32SD, 1 Voigt / HW32Voigt, 2 Doppler,
// 3 Lorentz -- the CEF is ignored by Doppler and Lorentz, as line_shape! ignores it (compute_absorption_cross_section.jl:167-177).
// An unknown code: -1 and, in *err, a text that starts with `fn` and holds the code
inline int mom_line_shape(const char *fn, int broadening, int cef, std::string *err) {
  const bool bad_b = broadening < MOM_BROADENING_VOIGT || broadening > MOM_BROADENING_LORENTZ;
  if (bad_b || cef < MOM_CEF_HW32SD || cef > MOM_CEF_HW32VOIGT) {
    *err = std::string(fn) + (bad_b ? ": unknown broadening code " + std::to_string(broadening) + " (0 Voigt, 1 Doppler, 2 Lorentz)"
                                    : ": unknown CEF code " + std::to_string(cef) + " (0 HW32SD, 1 HW32Voigt)");
    return -1;
  }
  return broadening == MOM_BROADENING_VOIGT ? cef : broadening + 1;
}
// does the shape read prefactor k of (nu, gamma_d, y, S, gamma_l)?  The others may be null at the C ABI
inline bool mom_shape_reads(int shape, int k) { return k == 0 || k == 3 || (k == 1 ? shape != 3 : k == 2 ? shape <= 1 : shape == 3); }

// ---- The line buffers of the absorption path.  THE FORMAT IS DECIDED HERE AND NOWHERE ELSE: kernels, launchers, entry points and
// getters take the views below and never index a buffer themselves.
// One layer's prefactors (device pointers, [cap] each): the five line_shape! takes (compute_absorption_cross_section.jl:118-124) and
// the line's 1-based grid window.  T = const double: what the line-shape kernels read; T = double: what k_line_prefactors* writes.
template <class T>
struct MomLineViewT {
  using Int = std::conditional_t<std::is_const<T>::value, const int, int>;
  T *nu, *gamma_d, *y, *S, *gamma_l;
  Int *i0, *i1;
  T *&prefactor(int k) { T **const m[5] = {&nu, &gamma_d, &y, &S, &gamma_l}; return *m[k]; }   // in the C ABI's order (mom_shape_reads)
  __host__ __device__ operator MomLineViewT<const T>() const { return {nu, gamma_d, y, S, gamma_l, i0, i1}; }
};
using MomLineView = MomLineViewT<const double>;
using MomLineOut = MomLineViewT<double>;
// One layer's partials of the five prefactors with respect to (k = 0) pressure and (k = 1) temperature: partial k of line j at
// p[j + ks k]; to a reader a null array counts as zeros
template <class T>
struct MomLinePartialsT {
  T *dnu, *dgamma_d, *dy, *dS, *dgamma_l;
  size_t ks;
  T *&partial(int q) { T **const m[5] = {&dnu, &dgamma_d, &dy, &dS, &dgamma_l}; return *m[q]; }   // the order of prefactor()
  __host__ __device__ operator MomLinePartialsT<const T>() const { return {dnu, dgamma_d, dy, dS, dgamma_l, ks}; }
};
using MomLinePartials = MomLinePartialsT<const double>;
using MomLinePartialsOut = MomLinePartialsT<double>;
// The resident partial block: [nu | gamma_d | y | S | gamma_l][2][nz][cap], (cap, nz) of the value block it belongs to
// (MomLineBlock::partials)
struct MomLinePartialBlock {
  double *base;
  size_t cap;
  int nz;
  size_t doubles() const { return 10 * cap * (size_t)nz; }
  __host__ __device__ MomLinePartialsOut layer(int z) const {
    const size_t ks = cap * (size_t)nz, lz = cap * (size_t)z;
    return {base + lz, base + 2 * ks + lz, base + 4 * ks + lz, base + 6 * ks + lz, base + 8 * ks + lz, ks};
  }
};
// The resident value block: [nu | gamma_d | y | S | the two window arrays as ints | gamma_l][nz][cap] in `doubles()` doubles at base
struct MomLineBlock {
  double *base;
  size_t cap;   // lines one layer has room for: the stride of the arrays, not the size of the allocation
  int nz;
  // the one capacity rule: room to grow to twice the lines before the next allocation, and no small allocations
  static size_t capacity_for(size_t nLines) { return std::max<size_t>(nLines, 1024) * 2; }
  size_t doubles() const { return 6 * cap * (size_t)nz; }
  __host__ __device__ MomLineOut layer(int z) const {
    const size_t ks = cap * (size_t)nz, lz = cap * (size_t)z;
    int *const win = reinterpret_cast<int *>(base + 4 * ks);
    return {base + lz, base + ks + lz, base + 2 * ks + lz, base + 3 * ks + lz, base + 5 * ks + lz, win + lz, win + ks + lz};
  }
  MomLinePartialBlock partials(double *at) const { return {at, cap, nz}; }   // the partial block to match, in memory of its own
};

// voigt.hip: one launch for all lines (device pointers, stream st); out[g] = acc  or  out[g] += factor * acc.  With `dln`, the Dual
// run: also dout[g + os k] = d_k acc  or  += factor * d_k acc
hipError_t mom_voigt_launch(hipStream_t st, int shape, int nLines, const MomLineView &ln, const MomLinePartials *dln, int nGrid,
                            const double *grid, double *out, double *dout, size_t os, double factor, int accumulate, int sorted);

// resident HITRAN table of one absorber + the TIPS spline tables of its isotopologues (device pointers)
struct MomLineTable {
  int nLines, nIso, nTmax;
  const double *nu0, *S0, *g_air, *g_self, *E, *n_air, *d_air, *sqw;  // [nLines]
  const int *iso;                                                     // [nLines] index into the spline tables
  const int *nT;                                                      // [nIso] knots per isotopologue
  const double *tT, *tQ, *tZ;                                         // [nIso, nTmax] knots, values, second derivatives
};
// the scalar part of gamma_d = (cSqrt2Ln2 / cc_) sqrt(cBolts_ / cMassMol) sqrt(T) nu_0 / sqrt(mol_weight)
// (compute_absorption_cross_section.jl:87-88), the `cgd` the prefactor kernels take per layer, and its temperature derivative
// (d sqrt(T) = 1 / (2 sqrt(T))) for the Dual run
inline double mom_doppler_cg() { return (1.1774100225 / 2.99792458e8) * std::sqrt(1.3806503e-23 / 1.66053873e-27); }
inline double mom_doppler_scale(double T) { return mom_doppler_cg() * std::sqrt(T); }
inline double mom_doppler_scale_dT(double T) { return mom_doppler_cg() * (1.0 / (2.0 * std::sqrt(T))); }
// voigt.hip: per-line prefactors of one (p, T) on the device; *unsorted is set when the windows are not monotone
hipError_t mom_line_prefactors_launch(hipStream_t st, const MomLineTable &tb, int nGrid, const double *grid, double p, double T,
                                      double vmr, double wing, double cgd, const MomLineOut &out, int *unsorted);
// every layer of a profile (pf.nz of them): prefactors of all (layer, line) pairs into pf, then the line shapes of all (layer, grid
// point) pairs; prm = [p | T | cgd | factor][nz], unsorted [nz].  With `dpf`, the Dual run: prm = [p | T | cgd | factor | d cgd / dT][nz],
// the prefactors' partials into dpf, dtau_abs [nGrid, nz, 2]
hipError_t mom_voigt_profile_launch(hipStream_t st, int shape, const MomLineTable &tb, const MomLineBlock &pf, const MomLinePartialBlock *dpf,
                                    int nGrid, const double *grid, const double *prm, double vmr, double wing, int *unsorted,
                                    double *tau_abs, double *dtau_abs, const double *factor);

// mom_dual.hip: rt_run on ForwardDiff.Dual numbers (values + P partials) for the resident scene.  Device pointers unless noted;
// partial arrays have the layout of their value arrays with the partial index as the slowest axis, nullptr = zero partials.
struct MomDualScene {
  int N, nS, S, Nz, K, M, P, nVza, imu0, strict, surf_kind;
  double mu0, albedo;
  double I0[4], D[4];
  const double *mu, *wt;                                   // [N]
  const double *tau, *varpi, *zw, *Zpp, *Zmp, *tau_sum;    // [S,Nz], [S,Nz], [K,S,Nz], [N,N,K,M] x2, [S,Nz+1]
  const double *dtau, *dvarpi, *dzw, *dZpp, *dZmp;         // (.., P)
  const double *dalbedo;                                   // [P]
  const double *Rsurf, *dRsurf, *albedo_spec, *dalbedo_spec;  // [N,N,M](,P), [S](,P)
  const int *nd, *iface;                                   // HOST [Nz]
  const int *node;                                         // [nVza]
  const double *cos_mphi, *sin_mphi;                       // [nVza,M]
  double *R, *T, *dR, *dT;                                 // [nVza,nS,S], [nVza,nS,S,P]
  double *hdr, *dhdr, *bhr_uw, *bhr_dw, *dbhr_uw, *dbhr_dw; // [nVza,nS,S](,P); [nS,S](,P)
  double *dtau_sum_buf;                                    // [S,Nz+1,P] scratch
  int *info;
  hipStream_t stream;
  MomDevBuf<char> *work;                                   // workspace owned by the handle (grown on demand)
  size_t work_budget;                                      // bytes the operator workspace may take (units are chunked to fit)
};
size_t momd_bytes_per_unit(int N, int P);
int momd_run(const MomDualScene &sc, std::string *err);   // 0 ok, 1 unsupported, 2 HIP error (text in *err)

// mom_zmom.hip: the phase-matrix Fourier moments as a plan and a launch.  The plan holds what does not depend on the destination:
// the host scalars of the recurrences and their uploads, the Greek rows [nG][6][l_pad], the (set, moment) -> block table
// slot [nG, M] and the planes of the generalised spherical functions.  The launch writes block slot[g + nG mi] of Zpp / Zmp, blocks of
// row pitch `pitch` >= N = n n_mu (the entries behind N are left as they are: zero them in front), and with Zpp0 the (I,Q) cut of
// the moment-0 block of set g into block g of [pitch0, pitch0, nG].  Everything is asynchronous on `st`, so the plan, the stage it
// was made from and the destinations outlive the stream's work.
struct MomZmomPlan {
  int n = 0, n_mu = 0, L = 0, l_pad = 0, nG = 0, m_first = 0, M = 0, ldSeed = 0;
  std::vector<double> mu, smu, coef, seed;  // the host side of the asynchronous uploads
  std::vector<int> slot;
  MomDevBuf<double> d_mu, d_smu, d_coef, d_seed, d_greek, d_tab;
  MomDevBuf<int> d_lmax, d_slot, d_flag;
};
#pragma GCC visibility push(hidden)
// the argument checks mom_z_moments makes before its first HIP call: the text of the first that fails, or null
const char *mom_zmom_check(int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek, int m_first,
                           int M);
hipError_t mom_zmom_plan(MomZmomPlan &pl, int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek,
                         int m_first, int M, const int *slot, hipStream_t st);
hipError_t mom_zmom_launch(const MomZmomPlan &pl, hipStream_t st, double *Zpp, double *Zmp, int pitch, double *Zpp0, double *Zmp0,
                           int pitch0);
// the data half of mom_m0_reducible on the device: *coupled = 1 when a moment-0 block (blocks 0 .. K - 1) of Zpp or Zmp has an
// (I,Q) <-> (U,V) entry != 0.0.  Drains `st`: the int is the only transfer
hipError_t mom_zmom_couples(MomZmomPlan &pl, hipStream_t st, int K, const double *Zpp, const double *Zmp, int pitch, int *coupled);
#pragma GCC visibility pop

// mom_mie.hip: the tables P, P2, R2, T2 [l_max, n_mu] (mu fastest) of compute_legendre_poly from device nodes mu, by the kernel of
// the spectral Mie call (k_mie_tables), bitwise the host's.  coef: mom_legendre_table_coef(l_max) on the device; pitau [2 n_mu]:
// room for the first row of the kernel's pi / tau tables; leg: the four destinations.  Asynchronous on `st`.
#pragma GCC visibility push(hidden)
std::vector<double> mom_legendre_table_coef(int l_max);
hipError_t mom_legendre_tables_launch(hipStream_t st, int n_mu, int l_max, const double *mu, const double *coef, double *pitau,
                                      double *const *leg);
#pragma GCC visibility pop

// mom_trunc.hip: the delta-BGE truncation of a batch of Greek sets as a plan and a launch.  The plan holds what does not depend on the
// destination: the nodes, the Greek rows [l_full, 6, 1 + nP, nG], the per-degree scalars, and the workspaces (tables, diagonal
// weights, Gram products of one sub-batch of sets).  The launch writes greek_t [l_tr, 6, 1 + nP, nG], c0 [1 + nP, nG] and
// status [nG] on the device; everything is asynchronous on `st`, so the plan and the destinations outlive the stream's work.
constexpr int kMomTruncMax = 128;  // the largest l_tr: the edge of the normal matrix the solve keeps in LDS
struct MomTruncPlan {
  int n_mu = 0, nG = 0, nP = 0, l_full = 0, l_tr = 0, chunk = 0;  // chunk: sets per pass over the Gram workspace
  std::vector<double> coef, fac;  // the host side of the asynchronous uploads
  MomDevBuf<double> d_mu, d_w, d_coef, d_fac, d_greek, d_tab, d_D, d_G;
};
#pragma GCC visibility push(hidden)
// the argument checks mom_truncate_phase makes before its first HIP call: the text of the first that fails, or null
const char *mom_trunc_check(int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr, const double *greek);
hipError_t mom_trunc_plan(MomTruncPlan &pl, int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr,
                          const double *greek, hipStream_t st);
hipError_t mom_trunc_launch(const MomTruncPlan &pl, hipStream_t st, double *greek_t, double *c0, int *status);
#pragma GCC visibility pop

// mom_scene.hip: what the two setters of the scene's partials share (mom_scene_set_partials there, mom_scene_set_optics_partials in
// mom_optics.hip).  _check: 0 <= P <= 64 and dZpp / dZmp both or neither, else MOM_EINVAL with `fn` in the text; _reset: the partials,
// outputs and workspaces of the previous call go and P becomes the scene's; _rest: everything but dtau / dvarpi / dzw (d_dual_in[0..2])
// -- the partials of the bases (padded like the scene's operators), of the surface of the scene's kind, d_dual_out, d_dual_ts
#pragma GCC visibility push(hidden)
int mom_partials_check(mom_t *h, const char *fn, int P, const double *dZpp, const double *dZmp);
void mom_partials_reset(mom_t *h, int P);
int mom_partials_rest(mom_t *h, const double *dZpp, const double *dZmp, const double *dalbedo, const double *dRsurf,
                      const double *dalbedo_spec);
#pragma GCC visibility pop

// argument blocks of the single-launch sweep kernels, shared by the launching translation unit (mom_scene.hip) and the
// kernels' own (mom_small.hip: momsm::k_sweep; mom_wave.hip: momw::k_wsweep)
template <class Real>
struct MomSmallSweepArgsT {
  int S, M, K, Nz, nVza, nS, imu0, pad;
  Real mu0, albedo;
  Real I0[4], D[4];
  // per-scene tables, the same for every spectral point (read through the scalar cache)
  const Real *mu, *wt, *sg;         // [N]
  const Real *F1, *F2, *SI;         // [N,N] i + N j: mu_j/(mu_i+mu_j), mu_j/(mu_i-mu_j), (1/mu_i)+(1/mu_j)
  const Real *Zpp, *Zmp;            // [N,N,K,M]
  const int *nd, *iface;              // [Nz]
  const int *node;                    // [nVza]
  const double *cos_mphi, *sin_mphi;  // [nVza,M]
  // per-point inputs
  const Real *tau, *varpi, *zw, *tau_sum;  // [S,Nz], [S,Nz], [K,S,Nz], [S,Nz+1]
  // outputs
  Real *R, *T, *hdr, *bhr_uw, *bhr_dw;  // [nVza,nS,S] x3, [nS,S] x2
  int *info;
  // r5: one (point, moment) per lane when `part` is given and M > 1: the terms of R_SFI / T_SFI go to part[m][R | T][nVza,nS,S]
  // and a second kernel adds them in ascending m (the order of the accumulator they replace); the lanes of m = 0 write hdr / bhr
  Real *part;
};
using MomSmallSweepArgs = MomSmallSweepArgsT<double>;
using MomSmallSweepArgsF = MomSmallSweepArgsT<float>;  // mom_small.hip with -DMOMS_FLOAT
template <class Real>
struct MomWaveSweepArgsT {
  int N, S, M, K, Nz, nVza, nS, imu0, inv_mode, pad;
  Real mu0, albedo;
  Real I0[4], D[4];
  const Real *mu, *wt, *sg;           // [N]
  const Real *Zpp, *Zmp;              // [N,N,K,M]
  const int *nd;                        // [Nz]
  const int *node;                      // [nVza]
  const double *cos_mphi, *sin_mphi;    // [nVza,M]
  const Real *tau, *varpi, *zw, *tau_sum;  // [S,Nz], [S,Nz], [K,S,Nz], [S,Nz+1]
  Real *R, *T, *hdr, *bhr_uw, *bhr_dw;
  int *info;
  // surface (mom_scene_set_surface): 0 LambertianSurfaceScalar(albedo), 1 BRDF matrices Rsurf [N,N,M] (every moment),
  // 2 LambertianSurfaceLegendre (albedo_spec [S]; j0+ = 0, T_SFI from m = 0 only: lambertian_surface.jl:112,131-132)
  int surf_kind, pad2;
  const Real *Rsurf, *albedo_spec;
};
using MomWaveSweepArgs = MomWaveSweepArgsT<double>;   // Float64 wave-per-point sweep (mom_wave.hip)
using MomWaveSweepArgsF = MomWaveSweepArgsT<float>;   // Float32 build of the same kernels (mom_wave.hip with -DMOMW_FLOAT)

#pragma GCC visibility push(hidden)
// ---- The single-launch runs up to their launch, written once for both drivers over MomSceneBufs<Real>.  `Streams` is the driver's
// DevStreams (mom:: or momf::, mom_kernels.hpp), with N the edge the scene runs on.  The nd | iface upload, the launch (momsm_ /
// momsmf_, momw_ / momwf_launch_sweep) and the timing events around it stay with each driver.
// What the two argument blocks have in common
template <class Args, class Real, class Streams>
inline void mom_fill_sweep_scene(Args &a, const MomSceneBufs<Real> &b, const Streams &q, int S, int *info) {
  a.S = S; a.M = b.scene_M; a.K = b.K; a.Nz = b.Nz; a.nVza = b.nVza; a.nS = q.nS; a.imu0 = q.imu0;
  a.mu0 = q.mu0; a.albedo = b.albedo;
  for (int k = 0; k < 4; ++k) { a.I0[k] = q.I0[k]; a.D[k] = q.D[k]; }
  a.mu = b.d_mu; a.wt = b.d_wt; a.sg = b.d_sg;
  a.Zpp = b.d_Zpp; a.Zmp = b.d_Zmp;
  a.nd = b.d_ndif; a.node = b.d_node; a.cos_mphi = b.d_cos; a.sin_mphi = b.d_sin;
  a.tau = b.d_tau; a.varpi = b.d_varpi; a.zw = b.d_zw; a.tau_sum = b.d_tau_sum;
  a.R = b.d_R; a.T = b.d_T; a.hdr = b.d_hdr; a.bhr_uw = b.d_bhr_uw; a.bhr_dw = b.d_bhr_dw;
  a.info = info;
}
// N <= 4, one spectral point per lane.  F1 | F2 | SI [3][16] from the host copy of the streams: mu_j/(mu_i + mu_j),
// mu_j/(mu_i - mu_j), (1/mu_i) + (1/mu_j) -- the expressions of elemental.jl:176-186 in Real, evaluated once
template <class Real>
inline void mom_small_tables(const Real *mu, int N, Real *tab /* [48] */) {
  std::fill(tab, tab + 48, Real(0));
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      const Real mui = mu[i], muj = mu[j];
      tab[i + N * j] = muj / (mui + muj);
      tab[16 + i + N * j] = muj / (mui - muj);
      tab[32 + i + N * j] = (1 / mui) + (1 / muj);
    }
}
// its argument block: tables in d_smtab, nd | iface in d_ndif.  `split` (MOM_OPT_SMALL_N = 1) and more than one moment: one
// (point, moment) per lane (mom_small.hip SPLIT), which needs the grow-only part buffer
template <class Real, class Streams>
inline hipError_t mom_fill_small_args(MomSmallSweepArgsT<Real> &a, MomSceneBufs<Real> &b, const Streams &q, int S, int *info, bool split,
                                      hipStream_t st) {
  mom_fill_sweep_scene(a, b, q, S, info);
  a.F1 = b.d_smtab; a.F2 = b.d_smtab + 16; a.SI = b.d_smtab + 32;
  a.iface = b.d_ndif + b.Nz;
  if (!(a.M > 1 && split)) return hipSuccess;
  const hipError_t e = b.d_smpart.reserve((size_t)a.M * 2 * a.nVza * a.nS * a.S, st);
  a.part = b.d_smpart;
  return e;
}
// 4 < N <= 32, one spectral point per wavefront.  The kernel covers ScatteringInterface_11 (code 3) on every layer after the first
// and at the surface; `small_n` / `force_generic`: MOM_OPT_SMALL_N, MOM_OPT_FORCE_GENERIC
template <class Real>
inline bool mom_wave_sweep_applies(const MomSceneBufs<Real> &b, int N, int nS, bool small_n, bool force_generic) {
  if (!(N > 4 && N <= 32 && small_n && !force_generic && b.nVza * nS <= 256)) return false;
  for (int z = 1; z < b.Nz; ++z)
    if (b.iface[z] != 3) return false;
  return b.iface[b.Nz - 1] == 3;
}
// points per wavefront (mom_wave.hip, block-diagonal packing; k_wsweep's PK); `pack`: MOM_OPT_SMALL_N = 1 (2 keeps one point per wave)
inline int mom_wave_points(int N, bool pack) { return pack ? (N == 5 ? 3 : (N >= 6 && N <= 8 ? 2 : 1)) : 1; }
template <class Real, class Streams>
inline void mom_fill_wave_args(MomWaveSweepArgsT<Real> &a, const MomSceneBufs<Real> &b, const Streams &q, int S, int *info, bool pack) {
  mom_fill_sweep_scene(a, b, q, S, info);
  a.N = q.N; a.inv_mode = q.inv_mode; a.pad = mom_wave_points(q.N, pack);
  a.surf_kind = b.surf_kind; a.Rsurf = b.d_Rsurf; a.albedo_spec = b.d_albedo_spec;
}
#pragma GCC visibility pop

// ---- entry points between the translation units: declarations only (no device code, nothing that depends on MOM_NS / MOM_REAL).
// Every unit that defines one of them includes this header, so a definition is checked against what its callers see.
// momcore_w4.hip: the same kernels built for 4-wave workgroups (2 workgroups per CU when the operators are
// small enough for two LDS images: the m = 0 (I,Q) sub-problem of N = 60 is N0 = 40 -> 77 KB).
size_t mom4_lds_bytes(int N, bool lds_mats);
hipError_t mom4_launch_layer(const void *layer_args, int iface, bool lds, int grid, size_t smem, hipStream_t st);
// momcore_gen.hip: the general layer kernels k_layer<LDSM, IFACE> of the 8-wave build
hipError_t mom_gen_launch_layer(const void *layer_args, int iface, bool lds, int grid, size_t smem, hipStream_t st);
// the per-size images (strip-chained, lean, two-buffer, quad-block): mom_images.hpp
hipError_t mom4_launch_surface(const void *surf_args, bool lds, int grid, size_t smem, hipStream_t st);
int mom4_generic_bufs_elems(int N);
// momcore_f32.hip: the Float32 build of the scene-level path (dtype = 1)
struct momf_scene;
int momf_create(momf_scene **out, int device, hipStream_t stream, int N, int nS, int S, int max_m, int *d_info);
void momf_destroy(momf_scene *s);
const char *momf_error(const momf_scene *s);
void momf_set_options(momf_scene *s, int inv_mode, int force_generic, int sweep, int small_n, int m0, int pad, int w4);
int momf_set_streams(momf_scene *s, const double *mu, const double *wt, const double *sg, int imu0, double mu0, const double *I0,
                     const double *D, int regular);
int momf_scene_set(momf_scene *s, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                   const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *tau_sum,
                   double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi);
int momf_scene_set_dev(momf_scene *s, int Nz, int K, int M, const double *d_tau, const double *d_varpi, const double *d_zw,
                       const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *d_tau_sum,
                       double albedo, int nVza, const int *node, const double *cos_mphi, const double *sin_mphi);
int momf_scene_set_surface(momf_scene *s, int kind, int M, const double *Rsurf, const double *albedo_spec);
int momf_rt_run(momf_scene *s);
int momf_get_RT(momf_scene *s, double *R, double *T);
int momf_get_hdr(momf_scene *s, double *hdr, double *up, double *dw);
int momf_timers(momf_scene *s, double *ms, int *launches);
int momf_blas(momf_scene *s, int n, int batch, const double *A, const double *B, double *C, bool inv);
int momf_op_elemental(momf_scene *s, int m, int nd, const double *tau_sum, const double *dtau, const double *varpi,
                      const double *Zpp, const double *Zmp, int z_batch);
int momf_op_doubling(momf_scene *s, int nd, double *expk);
int momf_op_interaction(momf_scene *s, int iface, int with_surface_layer);
int momf_op_copy_added_to_composite(momf_scene *s);
int momf_op_surface_lambertian(momf_scene *s, int m, double albedo, const double *tau_tot);
int momf_op_upload(momf_scene *s, int which, const double *src);
int momf_op_download(momf_scene *s, int which, double *dst);
// mom_small.hip: N <= 4, one spectral point per lane, the whole sweep in one launch
hipError_t momsm_launch_sweep(const void *args, int N, hipStream_t st);
hipError_t momsmf_launch_sweep(const void *args, int N, hipStream_t st);  // mom_small.hip built with -DMOMS_FLOAT
// mom_wave.hip: 4 < N <= 32, one spectral point per wavefront; k_wsweep<2, 8> is an object of its own (mom_wave8.o, -DMOMW_ONLY_KS8)
hipError_t momw_launch_sweep(const void *args, hipStream_t st);
hipError_t momw_launch_sweep8(const void *args, hipStream_t st);
hipError_t momwf_launch_sweep(const void *args, hipStream_t st);  // mom_wave.hip built with -DMOMW_FLOAT
hipError_t momwf_launch_sweep8(const void *args, hipStream_t st);
