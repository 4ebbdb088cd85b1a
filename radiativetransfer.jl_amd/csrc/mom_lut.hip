// mom_lut.hip -- the InterpolationModel of the C ABI (include/momcore.h, mom_lut_*): cross sections on a (nu, p, T) grid kept on
// the device as the coefficients of Interpolations.jl's `interpolate(A, BSpline(Cubic(Line(OnGrid()))))`, scaled to the model's
// ranges (make_model_helpers.jl:55-99, compute_absorption_cross_section.jl:139-159).  Three kernels: the prefilter along nu (chunks
// with a halo), the prefilter along p or T (one short Thomas solve per thread) and the evaluation (value and Dual).
#include <cstring>

#include "mom_handle.hpp"

// plain IEEE products and sums in every kernel of this file: the value of a Dual run is bitwise the value run's, and the staged
// and the 64-tap form of the evaluation add the same terms in the same order
#pragma clang fp contract(off)

namespace {
// ---- prefilter.  Per axis of n nodes the padded coefficients c_0 .. c_{n+1} solve (c_{i-1} + 4 c_i + c_{i+1}) / 6 = f_i (i = 1..n)
// with c_0 - 2 c_1 + c_2 = 0 and c_{n-1} - 2 c_n + c_{n+1} = 0.  The first interior row minus the first boundary row is c_1 = f_1
// (likewise c_n = f_n), which leaves the constant system  u_{k-1} + 4 u_k + u_{k+1} = r_k  for u_k = c_{k+2}, k = 0 .. m-1, m = n-2,
// r_k = 6 f_{k+2} (- f_1 for k = 0, - f_n for k = m-1); then c_0 = 2 c_1 - c_2, c_{n+1} = 2 c_n - c_{n-1}.
// Thomas: cp_0 = 1/4, cp_j = 1 / (4 - cp_{j-1}) (a table: it depends on the position only), d_j = (r_j - d_{j-1}) cp_j,
// u_j = d_j - cp_j u_{j+1}.
//
// Along nu the axis is long and the columns are few: a thread owns kNuChunk unknowns and solves them together with kNuHalo unknowns
// on either side, the system cut off there (u = 0 beyond the halo; at the ends of the axis the cut is the true boundary).  The
// error of the cut solves the homogeneous system, which decays by 2 - sqrt(3) = 0.268 per node: at the owned unknowns it is at
// most 0.268^32 = 5e-19 of max |c| per side.  A workgroup of one wavefront takes kNuSuper consecutive unknowns of one column
// through LDS, so that the loads and the stores are coalesced.
constexpr int kNuChunk = 32, kNuHalo = 32, kNuThreads = 64;
constexpr int kNuSuper = kNuChunk * kNuThreads;     // unknowns per workgroup
constexpr int kNuTile = kNuSuper + 2 * kNuHalo;     // right-hand sides it stages
constexpr int kNuDp = kNuChunk + kNuHalo + 1;       // a thread's row of d_j (owned unknowns + right halo), padded: odd stride
__device__ inline int nu_pad(int p) { return p + (p >> 5); }   // a thread's stride of 32 doubles becomes 33: two banks apart per lane

__global__ void __launch_bounds__(kNuThreads) k_lut_prefilter_nu(const double *__restrict__ table, double *__restrict__ coef,
                                                                 const double *__restrict__ cp, int nNu, int nP) {
  __shared__ double tile[kNuTile + kNuTile / 32 + 1];
  __shared__ double dp[kNuDp * kNuThreads];
  const int tid = threadIdx.x, col = blockIdx.y, ip = col % nP, iT = col / nP;
  const double *f = table + (size_t)nNu * col;
  double *c = coef + (size_t)(nNu + 2) * ((size_t)(ip + 1) + (size_t)(nP + 2) * (iT + 1));
  const int m = nNu - 2, base = blockIdx.x * kNuSuper;
  const double f1 = f[0], fn = f[nNu - 1];
  for (int idx = tid; idx < kNuTile; idx += kNuThreads) {
    const int k = base - kNuHalo + idx;
    double r = 0.0;
    if (k >= 0 && k < m) {
      r = 6.0 * f[k + 1];
      if (k == 0) r -= f1;
      if (k == m - 1) r -= fn;
    }
    tile[nu_pad(idx)] = r;
  }
  __syncthreads();
  const int a0 = base + tid * kNuChunk;
  if (a0 < m) {
    const int b0 = min(a0 + kNuChunk, m), lo = max(a0 - kNuHalo, 0), hi = min(b0 + kNuHalo, m);
    double *row = dp + tid * kNuDp;
    double d = 0.0;
    for (int k = lo; k < hi; ++k) {
      d = (tile[nu_pad(k - base + kNuHalo)] - d) * cp[k - lo];
      if (k >= a0) row[k - a0] = d;
    }
    double u = d;   // u_{hi-1}
    for (int k = hi - 2; k >= a0; --k) {
      u = row[k - a0] - cp[k - lo] * u;
      row[k - a0] = u;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < kNuSuper; idx += kNuThreads) {
    const int k = base + idx;
    if (k >= m) break;
    const double u = dp[(idx / kNuChunk) * kNuDp + idx % kNuChunk];
    c[k + 2] = u;
    if (k == 0) { c[1] = f1; c[0] = 2.0 * f1 - u; }
    if (k == m - 1) { c[nNu] = fn; c[nNu + 1] = 2.0 * fn - u; }
  }
}

// Along p or T: one thread per line of n nodes (node i at c[i * stride], f_i in place), consecutive threads on consecutive nu.
// Line t: nu index t % nu2, the other axis' index t / nu2 + other_off at other_stride.
__global__ void __launch_bounds__(256) k_lut_prefilter_axis(double *__restrict__ coef, const double *__restrict__ cp, int n, size_t stride,
                                                            int nu2, int n_other, size_t other_stride, int other_off) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nu2 * n_other) return;
  double *c = coef + t % nu2 + other_stride * (t / nu2 + other_off);
  const int m = n - 2;
  const double f1 = c[stride], fn = c[(size_t)n * stride];
  double d = 0.0;
  for (int k = 0; k < m; ++k) {
    double r = 6.0 * c[(size_t)(k + 2) * stride];
    if (k == 0) r -= f1;
    if (k == m - 1) r -= fn;
    d = (r - d) * cp[k];
    c[(size_t)(k + 2) * stride] = d;
  }
  double u = d;
  for (int k = m - 2; k >= 0; --k) {
    u = c[(size_t)(k + 2) * stride] - cp[k] * u;
    c[(size_t)(k + 2) * stride] = u;
  }
  c[0] = 2.0 * f1 - c[2 * stride];
  c[(size_t)(n + 1) * stride] = 2.0 * fn - c[(size_t)(n - 1) * stride];
}

// ---- evaluation.  Per axis x = (value - first) / step + 1, i = clamp(floor(x), 1, n - 1), delta = x - i, and the cubic B-spline
// weights of c_{i-1} .. c_{i+2}; the host forms the 4 x 4 (p, T) weight products of a layer (and their partials) once, the kernel
// contracts the 16 coefficient rows along nu with them and applies the nu weights.
struct LutLayer {
  double W[3][16];   // [0] wp[b] wT[c] at b + 4 c; [1] its partial with respect to p: (dwp[b] / p_step) wT[c]; [2] to T
  double factor;
  long long base;    // offset of coefficient (0, ip - 1, iT - 1)
};
static_assert(sizeof(LutLayer) % sizeof(double) == 0, "LutLayer is uploaded as doubles");
struct LutEvalArgs {
  const double *coef;
  const LutLayer *layers;
  const double *nu;   // [n] query points
  int n, nNu;
  double nu_first, nu_step;
  size_t s1, s2;      // strides of the p and the T axis of coef
  double *out;        // [n, Nz]
  double *dout;       // [n, Nz, 2] (Dual run)
  size_t dout_k;      // stride of the partial index
  int accumulate;     // out += value * factor (a profile call)  or  out = value
};
__host__ __device__ inline void lut_weights(double d, double *w) {
  const double e = 1.0 - d;
  w[0] = e * e * e / 6.0;
  w[1] = 2.0 / 3.0 - d * d + d * d * d / 2.0;
  w[2] = 2.0 / 3.0 - e * e + e * e * e / 2.0;
  w[3] = d * d * d / 6.0;
}
__host__ __device__ inline int lut_cell(double v, double first, double step, int n, double *delta) {
  const double x = (v - first) / step + 1.0, f = floor(x);
  const int i = f >= (double)(n - 1) ? n - 1 : (f >= 1.0 ? (int)f : 1);   // a NaN lands in cell 1: every index stays inside the table
  *delta = x - (double)i;
  return i;
}

constexpr int kEvalBlock = 256;
constexpr int kEvalTile = 768;   // contracted-row entries a workgroup stages: 256 outputs at up to 3 table nodes per output
// the (p, T) contraction at padded nu index k: r[q] = sum_c sum_b W[q][b + 4 c] C[k, b, c]
template <bool DUAL>
__device__ inline void lut_contract(const double *__restrict__ c, size_t s1, size_t s2, const LutLayer &L, double *r) {
  r[0] = 0.0;
  if constexpr (DUAL) { r[1] = 0.0; r[2] = 0.0; }
#pragma unroll
  for (int cc = 0; cc < 4; ++cc)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double v = c[s1 * b + s2 * cc];
      r[0] += L.W[0][b + 4 * cc] * v;
      if constexpr (DUAL) {
        r[1] += L.W[1][b + 4 * cc] * v;
        r[2] += L.W[2][b + 4 * cc] * v;
      }
    }
}
// blockIdx.y = layer.  staged: the workgroup's outputs span the contracted-row entries [lo, hi] between the cells of its first and
// its last query point when nu is monotone; if they fit the tile, each entry is contracted once into LDS and an output reads its
// four neighbours there.  An output whose cell lies outside the staged span (nu not monotone after all), a span that does not
// fit, and staged = 0 take the 64-tap form: the same sums in the same order.
template <bool DUAL>
__global__ void __launch_bounds__(kEvalBlock) k_lut_eval(LutEvalArgs a, int staged) {
  constexpr int NQ = DUAL ? 3 : 1;
  __shared__ double sR[NQ][kEvalTile];
  const int z = blockIdx.y;
  const LutLayer &L = a.layers[z];
  const double *C = a.coef + L.base;
  const int g0 = blockIdx.x * kEvalBlock, g = g0 + threadIdx.x, gl = min(g0 + kEvalBlock, a.n) - 1;
  const bool live = g < a.n;
  double delta = 0.0;
  const int i = live ? lut_cell(a.nu[g], a.nu_first, a.nu_step, a.nNu, &delta) : 1;
  int lo = 0, span = 0;
  if (staged) {
    double t;
    const int ia = lut_cell(a.nu[g0], a.nu_first, a.nu_step, a.nNu, &t), ib = lut_cell(a.nu[gl], a.nu_first, a.nu_step, a.nNu, &t);
    lo = min(ia, ib) - 1;
    span = max(ia, ib) + 2 - lo + 1;
    if (span <= kEvalTile) {
      for (int k = threadIdx.x; k < span; k += kEvalBlock) {
        double r[NQ];
        lut_contract<DUAL>(C + lo + k, a.s1, a.s2, L, r);
#pragma unroll
        for (int q = 0; q < NQ; ++q) sR[q][k] = r[q];
      }
    } else {
      span = 0;
    }
    __syncthreads();
  }
  if (!live) return;
  double w[4], val[NQ];
  lut_weights(delta, w);
#pragma unroll
  for (int q = 0; q < NQ; ++q) val[q] = 0.0;
  const int k0 = i - 1 - lo;
  if (k0 >= 0 && k0 + 3 < span) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < NQ; ++q) val[q] += w[t] * sR[q][k0 + t];
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double r[NQ];
      lut_contract<DUAL>(C + i - 1 + t, a.s1, a.s2, L, r);
#pragma unroll
      for (int q = 0; q < NQ; ++q) val[q] += w[t] * r[q];
    }
  }
  const size_t o = (size_t)a.n * z + g;
  if (a.accumulate) {
    a.out[o] = a.out[o] + val[0] * L.factor;
    if constexpr (DUAL)
      for (int k = 0; k < 2; ++k) a.dout[o + a.dout_k * k] = a.dout[o + a.dout_k * k] + val[1 + k] * L.factor;
  } else {
    a.out[o] = val[0];
    if constexpr (DUAL)
      for (int k = 0; k < 2; ++k) a.dout[o + a.dout_k * k] = val[1 + k];
  }
}

// ---- host side
const char *const kAxisName[3] = {"nu", "p", "T"};

MomLut *lut_of(mom_t *h, int id) { return id >= 0 && (size_t)id < h->luts.size() && h->luts[id].live ? &h->luts[id] : nullptr; }
int bad_id(mom_t *h, const char *fn, int id) {
  char buf[160];
  snprintf(buf, sizeof buf, "%s: %d is not a live table id (mom_lut_create)", fn, id);
  return fail(h, MOM_EINVAL, buf);
}
int no_coef(mom_t *h, const char *fn) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: the table has no coefficients yet: call mom_lut_set_table or mom_lut_build first", fn);
  return fail(h, MOM_ESTATE, buf);
}
// the scaled interpolant does not extrapolate: a value outside [first, last] of its axis raises (end points inside)
bool lut_outside(const MomLut &t, int axis, double v) {
  const double last = t.first[axis] + t.step[axis] * (t.n[axis] - 1);
  return !(v >= t.first[axis] && v <= last);
}
int out_of_range(mom_t *h, const char *fn, const MomLut &t, int axis, double v) {
  char buf[240];
  snprintf(buf, sizeof buf, "%s: %s = %.17g is outside the table's %s axis [%.17g, %.17g] (an InterpolationModel does not extrapolate)", fn,
           kAxisName[axis], v, kAxisName[axis], t.first[axis], t.first[axis] + t.step[axis] * (t.n[axis] - 1));
  return fail(h, MOM_EINVAL, buf);
}
// 1 non-decreasing, -1 non-increasing, 0 neither: the evaluation stages the contracted row for the first two
int lut_order(const double *v, size_t n) {
  bool up = true, down = true;
  for (size_t k = 1; k < n; ++k) {
    up = up && v[k] >= v[k - 1];
    down = down && v[k] <= v[k - 1];
  }
  return up ? 1 : (down ? -1 : 0);
}
// one layer's (p, T) cell, weight products and their partials (floor and clamp on the values; d/dp = dw / p_step)
void lut_layer(const MomLut &t, double p, double T, double factor, LutLayer *L) {
  double dp, dT, wp[4], wT[4];
  const int ip = lut_cell(p, t.first[1], t.step[1], t.n[1], &dp), iT = lut_cell(T, t.first[2], t.step[2], t.n[2], &dT);
  lut_weights(dp, wp);
  lut_weights(dT, wT);
  const double ep = 1.0 - dp, eT = 1.0 - dT;
  const double gp[4] = {-(ep * ep) / 2.0, -2.0 * dp + 3.0 * dp * dp / 2.0, 2.0 * ep - 3.0 * ep * ep / 2.0, dp * dp / 2.0};
  const double gT[4] = {-(eT * eT) / 2.0, -2.0 * dT + 3.0 * dT * dT / 2.0, 2.0 * eT - 3.0 * eT * eT / 2.0, dT * dT / 2.0};
  for (int c = 0; c < 4; ++c)
    for (int b = 0; b < 4; ++b) {
      L->W[0][b + 4 * c] = wp[b] * wT[c];
      L->W[1][b + 4 * c] = (gp[b] / t.step[1]) * wT[c];
      L->W[2][b + 4 * c] = wp[b] * (gT[c] / t.step[2]);
    }
  L->factor = factor;
  const size_t nu2 = (size_t)t.n[0] + 2, p2 = (size_t)t.n[1] + 2;
  L->base = (long long)(nu2 * ((size_t)(ip - 1) + p2 * (size_t)(iT - 1)));
}
// the layers' blocks on the device, then one launch; `nu` [n] and the outputs are device pointers
int lut_eval_launch(mom_t *h, const MomLut &t, const std::vector<LutLayer> &layers, const double *nu, int n, int staged, double *out,
                    double *dout, size_t dout_k, int accumulate) {
  const size_t per = sizeof(LutLayer) / sizeof(double);
  HIPCHK(h, h->d_lut_prm.reserve(per * layers.size(), h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_lut_prm, layers.data(), layers.size() * sizeof(LutLayer), hipMemcpyHostToDevice, h->stream));
  LutEvalArgs a{};
  a.coef = t.d_coef; a.layers = reinterpret_cast<const LutLayer *>(h->d_lut_prm.get()); a.nu = nu; a.n = n; a.nNu = t.n[0];
  a.nu_first = t.first[0]; a.nu_step = t.step[0];
  a.s1 = (size_t)t.n[0] + 2; a.s2 = a.s1 * ((size_t)t.n[1] + 2);
  a.out = out; a.dout = dout; a.dout_k = dout_k; a.accumulate = accumulate;
  const dim3 blocks((n + kEvalBlock - 1) / kEvalBlock, (unsigned)layers.size());
  if (dout) hipLaunchKernelGGL(k_lut_eval<true>, blocks, dim3(kEvalBlock), 0, h->stream, a, staged);
  else hipLaunchKernelGGL(k_lut_eval<false>, blocks, dim3(kEvalBlock), 0, h->stream, a, staged);
  HIPCHK(h, hipGetLastError());
  return MOM_OK;
}
// d_table -> d_coef, three passes on the handle's stream
int lut_prefilter(mom_t *h, MomLut &t) {
  const int nNu = t.n[0], nP = t.n[1], nT = t.n[2];
  const size_t nu2 = (size_t)nNu + 2, p2 = (size_t)nP + 2, t2 = (size_t)nT + 2;
  std::vector<double> cp((size_t)std::max(std::max(nP, nT), kNuChunk + 2 * kNuHalo));
  cp[0] = 0.25;
  for (size_t j = 1; j < cp.size(); ++j) cp[j] = 1.0 / (4.0 - cp[j - 1]);
  HIPCHK(h, h->d_lut_cp.reserve(cp.size(), h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_lut_cp, cp.data(), cp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (!t.d_coef) HIPCHK(h, t.d_coef.renew(nu2 * p2 * t2));
  t.has_coef = false;
  hipLaunchKernelGGL(k_lut_prefilter_nu, dim3((nNu - 2 + kNuSuper - 1) / kNuSuper, nP * nT), dim3(kNuThreads), 0, h->stream,
                     t.d_table.get(), t.d_coef.get(), h->d_lut_cp.get(), nNu, nP);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_lut_prefilter_axis, dim3((unsigned)((nu2 * nT + 255) / 256)), dim3(256), 0, h->stream, t.d_coef.get(),
                     h->d_lut_cp.get(), nP, nu2, (int)nu2, nT, nu2 * p2, 1);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_lut_prefilter_axis, dim3((unsigned)((nu2 * p2 + 255) / 256)), dim3(256), 0, h->stream, t.d_coef.get(),
                     h->d_lut_cp.get(), nT, nu2 * p2, (int)nu2, (int)p2, nu2, 0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));   // cp is a host temporary
  t.has_coef = true;
  return MOM_OK;
}
}  // namespace

extern "C" int mom_lut_create(mom_t *h, int nNu, double nu_first, double nu_step, int nP, double p_first, double p_step, int nT,
                              double t_first, double t_step, int *lut) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!lut) return fail(h, MOM_EINVAL, "mom_lut_create: null output");
  const int n[3] = {nNu, nP, nT};
  const double first[3] = {nu_first, p_first, t_first}, step[3] = {nu_step, p_step, t_step};
  char buf[200];
  for (int k = 0; k < 3; ++k) {
    if (n[k] < 3) {
      snprintf(buf, sizeof buf, "mom_lut_create: the %s axis has %d nodes; a cubic B-spline axis needs at least 3", kAxisName[k], n[k]);
      return fail(h, MOM_EINVAL, buf);
    }
    if (!(step[k] > 0.0) || !std::isfinite(step[k]) || !std::isfinite(first[k])) {
      snprintf(buf, sizeof buf, "mom_lut_create: the %s axis needs a finite first node and a step > 0 (got %g, %g)", kAxisName[k], first[k],
               step[k]);
      return fail(h, MOM_EINVAL, buf);
    }
  }
  if ((long long)nP * nT > 65535 || ((size_t)nNu + 2) * ((size_t)nP + 2) * ((size_t)nT + 2) > ((size_t)1 << 40))
    return fail(h, MOM_EINVAL, "mom_lut_create: more than 65535 (p, T) nodes or more than 2^40 coefficients");
  size_t id = 0;
  while (id < h->luts.size() && h->luts[id].live) ++id;
  if (id == h->luts.size()) h->luts.emplace_back();
  MomLut &t = h->luts[id];
  t = MomLut{};
  t.live = true;
  for (int k = 0; k < 3; ++k) { t.n[k] = n[k]; t.first[k] = first[k]; t.step[k] = step[k]; }
  *lut = (int)id;
  return MOM_OK;
}

extern "C" int mom_lut_destroy(mom_t *h, int lut) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_destroy", lut);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *t = MomLut{};
  return MOM_OK;
}

extern "C" int mom_lut_set_table(mom_t *h, int lut, const double *sigma) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_set_table", lut);
  if (!sigma) return fail(h, MOM_EINVAL, "mom_lut_set_table: null table");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t count = (size_t)t->n[0] * t->n[1] * t->n[2];
  t->has_table = t->has_coef = false;
  if (!t->d_table) HIPCHK(h, t->d_table.renew(count));
  HIPCHK(h, hipMemcpyAsync(t->d_table, sigma, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  t->has_table = true;
  return lut_prefilter(h, *t);   // synchronises: the host table is free again
}

// make_interpolation_model's loop over the (p, T) nodes (make_model_helpers.jl:82-88) as batches of "layers" of the profile kernels:
// node z = i + nP j is layer z of a profile with p = p_i, T = T_j, factor 1, accumulated into a zeroed table.
extern "C" int mom_lut_build(mom_t *h, int lut, double vmr, double wing_cutoff, double *gpu_ms) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_build", lut);
  int rc = mom_absorption_state(h, "mom_lut_build", false, true);
  if (rc) return rc;
  const int nNu = t->n[0], nP = t->n[1], nT = t->n[2], nodes = nP * nT;
  for (int j = 0; j < nT; ++j) {
    const double T = t->first[2] + t->step[2] * j;
    if (!(T > 0.0)) return fail(h, MOM_EINVAL, "mom_lut_build: the T axis reaches T <= 0");
    if ((rc = mom_tips_range(h, T))) return rc;
  }
  if (gpu_ms) gpu_ms[0] = gpu_ms[1] = 0.0;
  HIPCHK(h, hipSetDevice(h->device));
  std::string err;
  const int shape = mom_line_shape("", h->abs_broadening, h->abs_cef, &err);
  const size_t count = (size_t)nNu * nodes;
  t->has_table = t->has_coef = false;
  if (!t->d_table) HIPCHK(h, t->d_table.renew(count));
  if (!t->d_nu) {
    std::vector<double> nu((size_t)nNu);
    for (int k = 0; k < nNu; ++k) nu[k] = t->first[0] + t->step[0] * k;
    HIPCHK(h, mom_upload(t->d_nu, nu.data(), nu.size(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  hipEvent_t ev[3] = {};
  if (gpu_ms)
    for (int k = 0; k < 3; ++k) HIPCHK(h, hipEventCreate(&ev[k]));
  struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 3; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ev};
  if (gpu_ms) HIPCHK(h, hipEventRecord(ev[0], h->stream));
  HIPCHK(h, hipMemsetAsync(t->d_table, 0, count * sizeof(double), h->stream));
  const int nLines = h->lt.nLines;
  // the prefactor block of a batch grows with nodes x lines: kLutBatch nodes at a time (MOM_OPT_LUT_BATCH); nodes are independent,
  // so the batch size does not change a bit
  const int batch = std::min(nodes, h->opt_lut_batch > 0 ? h->opt_lut_batch : 64);
  MomDevBuf<double> d_pf, prm;
  std::vector<double> hp(4 * (size_t)nodes);
  if (nLines > 0) {
    MomLineBlock pf = {nullptr, MomLineBlock::capacity_for((size_t)nLines), batch};
    HIPCHK(h, d_pf.renew(pf.doubles()));
    pf.base = d_pf;
    HIPCHK(h, prm.renew(4 * (size_t)nodes + ((size_t)nodes + 1) / 2));
    for (int z0 = 0; z0 < nodes; z0 += batch) {   // [p | T | cgd | factor][nb] per batch
      const int nb = std::min(batch, nodes - z0);
      double *b = hp.data() + 4 * (size_t)z0;
      for (int z = 0; z < nb; ++z) {
        const double T = t->first[2] + t->step[2] * ((z0 + z) / nP);
        b[z] = t->first[1] + t->step[1] * ((z0 + z) % nP);
        b[nb + z] = T;
        b[2 * (size_t)nb + z] = mom_doppler_scale(T);
        b[3 * (size_t)nb + z] = 1.0;
      }
    }
    HIPCHK(h, hipMemcpyAsync(prm, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int *flags = reinterpret_cast<int *>(prm + 4 * (size_t)nodes);
    HIPCHK(h, hipMemsetAsync(flags, 0, sizeof(int) * (size_t)nodes, h->stream));
    for (int z0 = 0; z0 < nodes; z0 += batch) {
      const int nb = std::min(batch, nodes - z0);
      const double *b = prm + 4 * (size_t)z0;
      pf.nz = nb;   // the last batch may be shorter: a block of fewer layers in the same memory
      HIPCHK(h, mom_voigt_profile_launch(h->stream, shape, h->lt, pf, nullptr, nNu, t->d_nu, b, vmr, wing_cutoff, flags + z0,
                                         t->d_table + (size_t)nNu * z0, nullptr, b + 3 * (size_t)nb));
    }
  }
  if (gpu_ms) HIPCHK(h, hipEventRecord(ev[1], h->stream));
  t->has_table = true;
  if ((rc = lut_prefilter(h, *t))) return rc;   // synchronises: hp, d_pf and prm may go
  if (gpu_ms) {
    HIPCHK(h, hipEventRecord(ev[2], h->stream));
    HIPCHK(h, hipEventSynchronize(ev[2]));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) gpu_ms[0] = ms;
    if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) gpu_ms[1] = ms;
  }
  return MOM_OK;
}

extern "C" int mom_lut_get_table(mom_t *h, int lut, double *sigma) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_get_table", lut);
  if (!sigma) return fail(h, MOM_EINVAL, "mom_lut_get_table: null output");
  if (!t->has_table) return fail(h, MOM_ESTATE, "mom_lut_get_table: the table is empty: call mom_lut_set_table or mom_lut_build first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(sigma, t->d_table, (size_t)t->n[0] * t->n[1] * t->n[2] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_lut_get_coefficients(mom_t *h, int lut, double *c) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_get_coefficients", lut);
  if (!c) return fail(h, MOM_EINVAL, "mom_lut_get_coefficients: null output");
  if (!t->has_coef) return no_coef(h, "mom_lut_get_coefficients");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t count = ((size_t)t->n[0] + 2) * ((size_t)t->n[1] + 2) * ((size_t)t->n[2] + 2);
  HIPCHK(h, hipMemcpyAsync(c, t->d_coef, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// compute_absorption_cross_section(model::InterpolationModel, grid, p, T) (compute_absorption_cross_section.jl:139-159) and, with J,
// absorption_cross_section(...; autodiff = true) (autodiff_helper.jl:17-51)
extern "C" int mom_lut_xsec(mom_t *h, int lut, int n, const double *nu, double p, double T, double *sigma, double *J) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, "mom_lut_xsec", lut);
  if (n < 1 || !nu || !sigma) return fail(h, MOM_EINVAL, "mom_lut_xsec: bad argument");
  if (!t->has_coef) return no_coef(h, "mom_lut_xsec");
  if (lut_outside(*t, 1, p)) return out_of_range(h, "mom_lut_xsec", *t, 1, p);
  if (lut_outside(*t, 2, T)) return out_of_range(h, "mom_lut_xsec", *t, 2, T);
  for (int k = 0; k < n; ++k)
    if (lut_outside(*t, 0, nu[k])) return out_of_range(h, "mom_lut_xsec", *t, 0, nu[k]);
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)n;
  HIPCHK(h, h->d_lut_io.reserve(4 * N, h->stream));   // nu | sigma | J
  double *d = h->d_lut_io;
  HIPCHK(h, hipMemcpyAsync(d, nu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  std::vector<LutLayer> layer(1);
  lut_layer(*t, p, T, 1.0, &layer[0]);
  const int rc = lut_eval_launch(h, *t, layer, d, n, lut_order(nu, N) != 0, d + N, J ? d + 2 * N : nullptr, N, 0);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(sigma, d + N, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (J) HIPCHK(h, hipMemcpyAsync(J, d + 2 * N, 2 * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

namespace {
// mom_lut_tau_abs_profile and its Dual run
int lut_profile_run(mom_t *h, const char *fn, bool dual, int lut, int Nz, const double *pressure, const double *temperature,
                    const double *factor, double *gpu_ms) {
  char buf[200];
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  MomLut *t = lut_of(h, lut);
  if (!t) return bad_id(h, fn, lut);
  if (!t->has_coef) return no_coef(h, fn);
  int rc = mom_absorption_state(h, fn, true, false);
  if (rc) return rc;
  snprintf(buf, sizeof buf, "%s: bad argument", fn);
  if (Nz < 1 || Nz > h->abs_Nz || Nz > 65535 || !pressure || !temperature || !factor) return fail(h, MOM_EINVAL, buf);
  for (int z = 0; z < Nz; ++z) {
    if (lut_outside(*t, 1, pressure[z])) return out_of_range(h, fn, *t, 1, pressure[z]);
    if (lut_outside(*t, 2, temperature[z])) return out_of_range(h, fn, *t, 2, temperature[z]);
  }
  // the handle's grid, as mom_absorption_begin saw it
  if (lut_outside(*t, 0, h->grid_min)) return out_of_range(h, fn, *t, 0, h->grid_min);
  if (lut_outside(*t, 0, h->grid_max)) return out_of_range(h, fn, *t, 0, h->grid_max);
  if (gpu_ms) *gpu_ms = 0.0;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = (size_t)h->S;
  if (dual && !h->d_dtau_abs) {   // allocated and zeroed by the first Dual call after mom_absorption_begin
    const size_t n = 2 * S * h->abs_Nz;
    HIPCHK(h, h->d_dtau_abs.renew(n));
    HIPCHK(h, hipMemsetAsync(h->d_dtau_abs, 0, n * sizeof(double), h->stream));
  }
  std::vector<LutLayer> layers((size_t)Nz);
  for (int z = 0; z < Nz; ++z) lut_layer(*t, pressure[z], temperature[z], factor[z], &layers[z]);
  if (gpu_ms) {
    for (int k = 0; k < 2; ++k)
      if (!h->ev_voigt[k]) HIPCHK(h, hipEventCreate(&h->ev_voigt[k]));
    HIPCHK(h, hipEventRecord(h->ev_voigt[0], h->stream));
  }
  if ((rc = lut_eval_launch(h, *t, layers, h->d_grid, h->S, h->grid_order != 0, h->d_tau_abs, dual ? h->d_dtau_abs.get() : nullptr,
                            S * h->abs_Nz, 1)))
    return rc;
  if (gpu_ms) HIPCHK(h, hipEventRecord(h->ev_voigt[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // layers is a host temporary
  if (gpu_ms) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev_voigt[0], h->ev_voigt[1]) == hipSuccess) *gpu_ms = ms;
  }
  return MOM_OK;
}
}  // namespace

extern "C" int mom_lut_tau_abs_profile(mom_t *h, int lut, int Nz, const double *pressure, const double *temperature, const double *factor,
                                       double *gpu_ms) {
  return lut_profile_run(h, "mom_lut_tau_abs_profile", false, lut, Nz, pressure, temperature, factor, gpu_ms);
}
extern "C" int mom_lut_tau_abs_profile_dual(mom_t *h, int lut, int Nz, const double *pressure, const double *temperature,
                                            const double *factor, double *gpu_ms) {
  return lut_profile_run(h, "mom_lut_tau_abs_profile_dual", true, lut, Nz, pressure, temperature, factor, gpu_ms);
}
