// mom_zmom.hip -- phase-matrix Fourier moments Z++ / Z-+ from Greek coefficients on gfx950 (Float64).
//
// Restates Scattering.compute_Z_moments(mod, mu, greek_coefs, m) (src/Scattering/compute_Z_matrices.jl:5-84) with
// compute_associated_legendre_PRT (legendre_functions.jl:17-178) and construct_Pi_matrix / construct_B_matrix
// (mie_helper_functions.jl:287-348) for a batch of nG Greek sets and the moments m_first .. m_first + M - 1.  Two launches:
//   (a) k_zmom_prt   one lane per (m, +-mu_i) walks l = m .. L - 1 (L = the largest l_max of the batch) and keeps the two previous
//                    orders of P, R, T in registers; writes the functions of the requested m only, as planes [L, n_mu] with mu
//                    fastest.  The reference's [n_mu, L, L] cube does not exist.
//   (b) k_zmom_gemm  A++[(i,a),(j,c)] = sum_(l,b) (Pi_l(mu_i) B_l)[a,b] Pi_l(mu_j)[b,c] and A-+ with Pi_l(-mu_j), as one GEMM of
//                    N x N x n (l_max - m), N = n n_mu, on v_mfma_f64_16x16x4 per (set, m, sign): both factors are formed from the
//                    planes of (a) and the Greek rows while they are staged in LDS, a k-step of 16 inner indices at a time, and
//                    2 fact and the sign pattern of Z-+ go in the epilogue.
// The statements of (a) are the reference's in the reference's association, without contraction, and the per-l scalars (square
// roots, integer quotients) come from the host, formed as the host text forms them: the planes are bitwise those of
// corert._prt_for_moment.  The products of (b) are summed in another order than the reference's loop over l (k-steps of the
// MFMA, fused multiply-adds); DESIGN section 4 states what that is allowed to cost.
// The host part is a plan and a launch (MomZmomPlan, mom_host.hpp): mom_z_moments launches into a buffer of its own and downloads it,
// the handle's scene setters launch into the buffers their kernels read (staged Greek sets, mom_scene.hip) -- the same kernels and
// the same arithmetic per entry, so the two leave the same bits.  (c) k_zmom_couples is the data half of the m = 0 reducibility
// test for bases that never reach the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "momcore.h"
#include "mom_host.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;     // output tile of a workgroup: 64 x 64, four wavefronts of 32 x 32 (2 x 2 MFMA tiles each)
constexpr int kKStep = 16;    // inner indices (l, b) staged per step: four MFMA k-steps
constexpr int kLd = 80;       // LDS row pitch in doubles: the four k rows a wavefront reads at once start 32 banks apart
constexpr int kThreads = 256;
constexpr int kCoef = 8;      // per-(m, l) scalars of the recurrence: m1, m2, 2l - 1, Y_P, X_P, Y_R, X_R, Z

// ---- (a) generalised spherical functions ----------------------------------------------------------------------------------
// coef [M, L, 8] as above (m = 0: m1, m2, Z unused; Y_P = l - 1, X_P = l, Y_R = sqrt((l + 1)(l - 3)), X_R = sqrt(l^2 - 4));
// seed [M, ldSeed, 2]: sqrt(i (i + m)) and sqrt((m + i) / (i - 2)) of the m >= 2 seed's product over i = 1 .. m;
// smu [n_mu] = sqrt(1 - mu^2) (the same at -mu); s15 = sqrt(1.5), s05 = sqrt(0.5), s16 = sqrt(1/6), hs15 = 0.5 sqrt(1.5).
// tab: planes [M, 2, 3, L, n_mu] (sign of mu, then P, R, T with T as the reference returns it, -T of the recurrence); rows
// l < m are never written and never read.
__global__ void __launch_bounds__(64) k_zmom_prt(int n_mu, int L, int m_first, int M, int ldSeed, const double *__restrict__ mu,
                                                 const double *__restrict__ smu, const double *__restrict__ coef,
                                                 const double *__restrict__ seed, double s15, double s05, double s16, double hs15,
                                                 double *__restrict__ tab) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= M * 2 * n_mu) return;
  const int i = t % n_mu, sg = (t / n_mu) & 1, mi = t / (2 * n_mu), m = m_first + mi;
  const double c = sg ? -mu[i] : mu[i], s = smu[i];
  const size_t plane = (size_t)L * n_mu;
  double *o = tab + (size_t)(mi * 2 + sg) * 3 * plane + i;
  double P1 = 0.0, R1 = 0.0, T1 = 0.0, P2 = 0.0, R2 = 0.0, T2 = 0.0;  // orders l - 1 and l - 2
  for (int l = m; l < L; ++l) {
    const double *cf = coef + ((size_t)mi * L + l) * kCoef;
    const double m1 = cf[0], m2 = cf[1], c2l1 = cf[2], Yp = cf[3], Xp = cf[4], Yr = cf[5], Xr = cf[6], Zc = cf[7];
    double P, R = 0.0, T = 0.0;
    if (m == 0) {
      if (l == 0) {
        P = 1.0;
      } else if (l == 1) {
        P = c;
      } else if (l == 2) {
        P = 0.5 * (3.0 * c * c - 1.0);
        R = hs15 * s * s;
      } else {
        P = (P1 * c2l1 * c - P2 * Yp) / Xp;
        R = (R1 * c2l1 * c - R2 * Yr) / Xr;
      }
    } else if (m == 1 && l == 1) {
      P = s05 * s;
    } else if (m == 1 && l == 2) {
      const double cB = s15 * s;
      P = s16 * (3.0 * c * s);
      R = -s16 * c * cB;
      T = s16 * cB;
    } else if (l == m) {  // m >= 2 seed
      double f1 = 1.0, f2 = 1.0;
      const double sh = s / 2.0;
      const double *sd = seed + (size_t)mi * ldSeed * 2;
      for (int q = 1; q <= m; ++q) {
        f1 = f1 * ((double)(2 * q - 1) * s) / sd[2 * q];
        if (q > 2) f2 = f2 * sh * sd[2 * q + 1];
        else f2 = f2 * sh;
      }
      const double edge = m == 2 ? 0.5 : 0.0;
      P = f1;
      if (s > 1e-8) {
        R = f2 * (1.0 + c * c) / (s * s);
        T = -(f2 * (2.0 * c) / (s * s));
      } else {
        R = edge;
        T = -edge;
      }
    } else if (l == m + 1 && m >= 2) {  // no order l - 2 yet: the step without the m2 term
      P = (m1 * P1 * c2l1 * c) / Xp;
      R = (m1 * R1 * c2l1 * c + m1 * T1 * Zc) / Xr;
      T = (m1 * T1 * c2l1 * c + m1 * R1 * Zc) / Xr;
    } else {
      P = (m1 * P1 * c2l1 * c - m2 * P2 * Yp) / Xp;
      R = (m1 * R1 * c2l1 * c - m2 * R2 * Yr + m1 * T1 * Zc) / Xr;
      T = (m1 * T1 * c2l1 * c - m2 * T2 * Yr + m1 * R1 * Zc) / Xr;
    }
    o[(size_t)l * n_mu] = P;
    o[plane + (size_t)l * n_mu] = R;
    o[2 * plane + (size_t)l * n_mu] = -T;  // the reference returns P, R, -T
    P2 = P1, R2 = R1, T2 = T1;
    P1 = P, R1 = R, T1 = T;
  }
}

// ---- (b) the contraction over (l, b) ----------------------------------------------------------------------------------------
// Pi_l[b][c] (construct_Pi_matrix): which plane (0 P, 1 R, 2 T, -1: zero) and its sign
__device__ __forceinline__ int pi_sel(int b, int c, double &sgn) {
  sgn = 1.0;
  if (b == c) return (b == 0 || b == 3) ? 0 : 1;
  if (b + c == 3 && b >= 1 && b <= 2) {
    sgn = -1.0;
    return 2;
  }
  return -1;
}

// (Pi_l B_l)[a][b] (construct_B_matrix: [beta gamma 0 0; gamma alpha 0 0; 0 0 zeta epsilon; 0 0 -epsilon delta]) has one term
// per entry: plane f with sign sgn times Greek row q (alpha, beta, gamma, delta, epsilon, zeta = 0 .. 5); -1: zero
__device__ __forceinline__ int left_sel(int a, int b, int &q, double &sgn) {
  sgn = 1.0;
  switch (a * 4 + b) {
    case 0: q = 1; return 0;               // P beta
    case 1: q = 2; return 0;               // P gamma
    case 4: q = 2; return 1;               // R gamma
    case 5: q = 0; return 1;               // R alpha
    case 6: q = 5; sgn = -1.0; return 2;   // -T zeta
    case 7: q = 4; sgn = -1.0; return 2;   // -T epsilon
    case 8: q = 2; sgn = -1.0; return 2;   // -T gamma
    case 9: q = 0; sgn = -1.0; return 2;   // -T alpha
    case 10: q = 5; return 1;              // R zeta
    case 11: q = 4; return 1;              // R epsilon
    case 14: q = 4; sgn = -1.0; return 0;  // P (-epsilon)
    case 15: q = 3; return 0;              // P delta
    default: q = 0; return -1;
  }
}

// grid: (output tiles, (set, m), {++, -+}).  The MFMA's row index runs over the columns (j, c) of Z and its column index, the one
// on the lanes, over the rows (i, a): Z is stored with i fastest, so a wavefront's stores are runs of 16 doubles.
// The block of (set g, moment mi) is slot[g + nG mi] of the destination, whose blocks have the row pitch `pitch` >= N (strip_pad's
// edge: the entries behind N are not written).  With Zpp0 the moment-0 block of set g also goes, cut to its (I,Q) entries at the
// mom_m0_full mapping (mom_reduce.hpp), to block g of the (I,Q) sub-problem's [pitch0, pitch0, nG] arrays.
template <int n>
__global__ void __launch_bounds__(kThreads) k_zmom_gemm(int n_mu, int L, int l_pad, int nG, int m_first, int M, int pitch,
                                                        const int *__restrict__ slot, const int *__restrict__ l_max,
                                                        const double *__restrict__ greek, const double *__restrict__ tab,
                                                        double *__restrict__ Zpp, double *__restrict__ Zmp, int pitch0,
                                                        double *__restrict__ Zpp0, double *__restrict__ Zmp0) {
  __shared__ double Xs[kKStep][kLd];  // Pi_l(+-mu_j)[b][c] at [k][(j, c) of the tile]
  __shared__ double Ys[kKStep][kLd];  // (Pi_l(mu_i) B_l)[a][b] at [k][(i, a) of the tile]
  const int N = n * n_mu, tiles = (N + kTile - 1) / kTile;
  const int tj = blockIdx.x / tiles, ti = blockIdx.x - tj * tiles;
  const int g = blockIdx.y % nG, mi = blockIdx.y / nG, sg = blockIdx.z, m = m_first + mi;
  const int inner = n * (l_max[g] - m);  // <= 0: the set has no order l >= m, the matrix is zero
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4, wj = w >> 1, wi = w & 1;
  // staging: this thread's (j, c) of X and (i, a) of Y, k = w + 4 q of the step
  const int cx = tj * kTile + lane, jx = cx / n, cc = cx - jx * n;
  const int ry = ti * kTile + lane, iy = ry / n, aa = ry - iy * n;
  const size_t plane = (size_t)L * n_mu;
  const double *tx = tab + (size_t)(mi * 2 + sg) * 3 * plane + jx;
  const double *ty = tab + (size_t)(mi * 2) * 3 * plane + iy;
  const double *gk = greek + (size_t)g * 6 * l_pad;
  d4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int r = 0; r < 2; ++r) acc[p][r] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < inner; k0 += kKStep) {
#pragma unroll
    for (int q = 0; q < kKStep / 4; ++q) {
      const int k = w + 4 * q, kk = k0 + k, lo = kk / n, b = kk - lo * n, l = m + lo;
      double x = 0.0, y = 0.0;
      if (kk < inner) {  // l < l_max[g] <= L
        double sgn;
        int qg;
        const int fx = pi_sel(b, cc, sgn);
        if (cx < N && fx >= 0) x = sgn * tx[(size_t)fx * plane + (size_t)l * n_mu];
        const int fy = left_sel(aa, b, qg, sgn);
        if (ry < N && fy >= 0) y = (sgn * ty[(size_t)fy * plane + (size_t)l * n_mu]) * gk[(size_t)qg * l_pad + l];
      }
      Xs[k][lane] = x;
      Ys[k][lane] = y;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kKStep / 4; ++s) {
      const int kr = 4 * s + lq;
      const double xa[2] = {Xs[kr][wj * 32 + lr], Xs[kr][wj * 32 + 16 + lr]};
      const double yb[2] = {Ys[kr][wi * 32 + lr], Ys[kr][wi * 32 + 16 + lr]};
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[p][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[p], yb[r], acc[p][r], 0, 0, 0);
    }
    __syncthreads();
  }
  // epilogue: Z = 2 fact A, fact = 1/2 at m = 0; Z-+ flips the blocks (a <= 1, c >= 2) and (a >= 2, c <= 1)
  const double scale = m == 0 ? 1.0 : 2.0;
  double *out = (sg ? Zmp : Zpp) + (size_t)slot[g + nG * mi] * pitch * pitch;
  double *out0 = (n >= 3 && m == 0 && Zpp0) ? (sg ? Zmp0 : Zpp0) + (size_t)g * pitch0 * pitch0 : nullptr;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int cj = tj * kTile + wj * 32 + p * 16 + lq + 4 * v, ri = ti * kTile + wi * 32 + r * 16 + lr;
        if (cj >= N || ri >= N) continue;
        double z = scale * acc[p][r][v];
        if (sg && ((ri % n <= 1) != (cj % n <= 1))) z = -z;
        out[(size_t)cj * pitch + ri] = z;
        if (out0 && ri % n <= 1 && cj % n <= 1) out0[(size_t)((cj / n) * 2 + cj % n) * pitch0 + (ri / n) * 2 + ri % n] = z;
      }
}

// The device half of mom_m0_reducible (mom_reduce.hpp): *flag becomes 1 when an (I,Q) <-> (U,V) entry of a moment-0 block (blocks
// 0 .. K - 1 of [pitch, pitch, K, M]) of either array is != 0.0 (a NaN counts).  *flag is zeroed on the stream in front.
__global__ void __launch_bounds__(256) k_zmom_couples(int N, int n, int pitch, int K, const double *__restrict__ Zpp,
                                                      const double *__restrict__ Zmp, int *flag) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, NN = (size_t)N * N;
  if (e >= NN * K) return;
  const int k = (int)(e / NN), j = (int)((e - k * NN) / N), i = (int)(e - k * NN - (size_t)j * N);
  if (((i % n) < 2) == ((j % n) < 2)) return;
  const size_t o = i + (size_t)pitch * (j + (size_t)pitch * k);
  if (Zpp[o] != 0.0 || Zmp[o] != 0.0) atomicOr(flag, 1);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int zmom_fail(const char *fn, const char *what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  mom_set_global_error(buf);
  return MOM_EINVAL;
}

int zmom_device(const char *fn, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    char buf[128];
    snprintf(buf, sizeof buf, "%s: no HIP device available", fn);
    mom_set_global_error(buf);
    return MOM_EHIP;
  }
  if (device < 0 || device >= ndev) return zmom_fail(fn, "device index out of range");
  return MOM_OK;
}

#define ZCHK(call)                                                                                     \
  do {                                                                                                 \
    hipError_t e__ = (call);                                                                           \
    if (e__ != hipSuccess) {                                                                           \
      char buf__[384];                                                                                 \
      snprintf(buf__, sizeof buf__, "%s: %s failed: %s", fn, #call, hipGetErrorString(e__));           \
      mom_set_global_error(buf__);                                                                     \
      rc = MOM_EHIP;                                                                                   \
      goto done;                                                                                       \
    }                                                                                                  \
  } while (0)

// the per-(m, l) scalars of the recurrences, as legendre_functions.jl forms them (integer products and quotients in Float64)
void zmom_scalars(int L, int m_first, int M, int ldSeed, std::vector<double> &coef, std::vector<double> &seed) {
  coef.assign((size_t)M * L * kCoef, 0.0);
  seed.assign((size_t)M * ldSeed * 2, 1.0);
  for (int mi = 0; mi < M; ++mi) {
    const long long m = m_first + mi;
    for (long long l = std::max<long long>(m + 1, 3); l < L; ++l) {
      double *cf = &coef[((size_t)mi * L + l) * kCoef];
      cf[2] = (double)(2 * l - 1);
      if (m == 0) {
        cf[3] = (double)(l - 1);
        cf[4] = (double)l;
        cf[5] = std::sqrt((double)((l + 1) * (l - 3)));
        cf[6] = std::sqrt((double)(l * l - 4));
        continue;
      }
      const double m1 = std::sqrt((double)(l - m) / (double)(l + m));
      cf[0] = m1;
      cf[1] = m1 * std::sqrt((double)(l - m - 1) / (double)(l + m - 1));
      cf[3] = (double)(l - 1 + m);
      cf[4] = (double)(l - m);
      cf[5] = ((double)(l + m - 1) / (double)(l - 1)) * std::sqrt((double)((l - 3) * (l + 1)));
      cf[6] = ((double)(l - m) / (double)l) * std::sqrt((double)(l * l - 4));
      cf[7] = (double)(2 * m * (2 * l - 1)) / (double)(l * (l - 1));
    }
    for (long long q = 1; q <= m; ++q) {
      seed[((size_t)mi * ldSeed + q) * 2] = std::sqrt((double)(q * (q + m)));
      if (q > 2) seed[((size_t)mi * ldSeed + q) * 2 + 1] = std::sqrt((double)(m + q) / (double)(q - 2));
    }
  }
}

// argument checks of a plan, before any HIP call: the text of the first one that fails, or null
const char *zmom_check(int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek, int m_first, int M) {
  if (n != 1 && n != 3 && n != 4) return "nStokes must be 1, 3 or 4";
  if (n_mu < 1) return "n_mu must be at least 1";
  if (nG < 1) return "nG must be at least 1";
  if (M < 1) return "M must be at least 1";
  if (m_first < 0) return "m_first must not be negative";
  if (l_pad < 1) return "l_pad must be at least 1";
  if (!mu || !l_max || !greek) return "null pointer";
  for (int g = 0; g < nG; ++g)
    if (l_max[g] < 1 || l_max[g] > l_pad) return "every l_max must be within 1..l_pad";
  for (int i = 0; i < n_mu; ++i)
    if (!(mu[i] > 0.0 && mu[i] <= 1.0)) return "all mu within compute_Z_moments have to be in ]0,1]";
  if ((long long)n * n_mu > 46340 || (long long)nG * M > 65535 || (long long)m_first + M > 46340)
    return "size out of range (N <= 46340, nG M <= 65535, m_first + M <= 46340)";
  return nullptr;
}

int zmom_run(const char *fn, int device, int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek,
             int m_first, int M, int set_inner, double *Zpp, double *Zmp, double *gpu_ms) {
  if (const char *bad = zmom_check(n, n_mu, mu, nG, l_pad, l_max, greek, m_first, M)) return zmom_fail(fn, bad);
  if (!Zpp || !Zmp) return zmom_fail(fn, "null pointer");
  if (set_inner < 0 || (set_inner > 0 && nG % set_inner != 0)) return zmom_fail(fn, "set_inner must be 0 or a divisor of nG");
  if (set_inner == 0) set_inner = nG;
  int rc = zmom_device(fn, device);
  if (rc != MOM_OK) return rc;

  const int N = n * n_mu;
  const size_t nZ = (size_t)N * N * nG * M;
  // [N, N, nG, M] for set_inner = nG; [N, N, K, M, P] for nG = K P sets ordered k fastest and set_inner = K
  std::vector<int> slot((size_t)nG * M);
  for (int mi = 0; mi < M; ++mi)
    for (int g = 0; g < nG; ++g) slot[g + (size_t)nG * mi] = (g % set_inner) + set_inner * (mi + M * (g / set_inner));
  MomZmomPlan pl;
  MomDevBuf<double> d_Z;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ZCHK(hipSetDevice(device));
  ZCHK(hipStreamCreate(&st));
  ZCHK(hipEventCreate(&ev[0]));
  ZCHK(hipEventCreate(&ev[1]));
  ZCHK(mom_zmom_plan(pl, n, n_mu, mu, nG, l_pad, l_max, greek, m_first, M, slot.data(), st));
  ZCHK(d_Z.renew(2 * nZ));
  ZCHK(hipEventRecord(ev[0], st));
  ZCHK(mom_zmom_launch(pl, st, d_Z.get(), d_Z.get() + nZ, N, nullptr, nullptr, 0));
  ZCHK(hipEventRecord(ev[1], st));
  ZCHK(hipMemcpyAsync(Zpp, d_Z.get(), nZ * sizeof(double), hipMemcpyDeviceToHost, st));
  ZCHK(hipMemcpyAsync(Zmp, d_Z.get() + nZ, nZ * sizeof(double), hipMemcpyDeviceToHost, st));
  ZCHK(hipStreamSynchronize(st));
  if (gpu_ms) {
    float t = 0.f;
    ZCHK(hipEventElapsedTime(&t, ev[0], ev[1]));
    *gpu_ms = t;
  }
done:
  if (st) (void)hipStreamSynchronize(st);  // the buffers and the host vectors end with this call
  for (int q = 0; q < 2; ++q)
    if (ev[q]) (void)hipEventDestroy(ev[q]);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

}  // namespace

extern "C" int mom_z_moments(int device, int nStokes, int n_mu, const double *mu, int nG, int l_pad, const int *l_max,
                             const double *greek, int m_first, int M, int set_inner, double *Zpp, double *Zmp, double *gpu_ms) {
  return zmom_run("mom_z_moments", device, nStokes, n_mu, mu, nG, l_pad, l_max, greek, m_first, M, set_inner, Zpp, Zmp, gpu_ms);
}

// ---- plan and launch (mom_host.hpp): what mom_z_moments and the handle's staged scene setters (mom_scene.hip) share ---------
const char *mom_zmom_check(int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek, int m_first,
                           int M) {
  return zmom_check(n, n_mu, mu, nG, l_pad, l_max, greek, m_first, M);
}

#define PCHK(call)                          \
  do {                                      \
    const hipError_t e__ = (call);          \
    if (e__ != hipSuccess) return e__;      \
  } while (0)

hipError_t mom_zmom_plan(MomZmomPlan &pl, int n, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek,
                         int m_first, int M, const int *slot, hipStream_t st) {
  int L = 0;
  for (int g = 0; g < nG; ++g) L = std::max(L, l_max[g]);
  pl.n = n; pl.n_mu = n_mu; pl.L = L; pl.l_pad = l_pad; pl.nG = nG; pl.m_first = m_first; pl.M = M; pl.ldSeed = m_first + M;
  zmom_scalars(L, m_first, M, pl.ldSeed, pl.coef, pl.seed);
  pl.mu.assign(mu, mu + n_mu);
  pl.smu.resize((size_t)n_mu);
  for (int i = 0; i < n_mu; ++i) pl.smu[i] = std::sqrt(1.0 - mu[i] * mu[i]);
  pl.slot.assign(slot, slot + (size_t)nG * M);
  PCHK(mom_upload(pl.d_mu, pl.mu.data(), pl.mu.size(), st));
  PCHK(mom_upload(pl.d_smu, pl.smu.data(), pl.smu.size(), st));
  PCHK(mom_upload(pl.d_coef, pl.coef.data(), pl.coef.size(), st));
  PCHK(mom_upload(pl.d_seed, pl.seed.data(), pl.seed.size(), st));
  PCHK(mom_upload(pl.d_greek, greek, (size_t)l_pad * 6 * nG, st));
  PCHK(mom_upload(pl.d_lmax, l_max, (size_t)nG, st));
  PCHK(mom_upload(pl.d_slot, pl.slot.data(), pl.slot.size(), st));
  return pl.d_tab.renew((size_t)M * 2 * 3 * L * n_mu);
}

hipError_t mom_zmom_launch(const MomZmomPlan &pl, hipStream_t st, double *Zpp, double *Zmp, int pitch, double *Zpp0, double *Zmp0,
                           int pitch0) {
  const int N = pl.n * pl.n_mu, tiles = (N + kTile - 1) / kTile;
  if (pitch < N || (Zpp0 && (!Zmp0 || pitch0 < 2 * pl.n_mu))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_zmom_prt, dim3((unsigned)((pl.M * 2 * pl.n_mu + 63) / 64)), dim3(64), 0, st, pl.n_mu, pl.L, pl.m_first, pl.M,
                     pl.ldSeed, pl.d_mu.get(), pl.d_smu.get(), pl.d_coef.get(), pl.d_seed.get(), std::sqrt(1.5), std::sqrt(0.5),
                     std::sqrt(1.0 / 6.0), 0.5 * std::sqrt(1.5), pl.d_tab.get());
  PCHK(hipGetLastError());
  const dim3 grid((unsigned)(tiles * tiles), (unsigned)(pl.nG * pl.M), 2);
#define ZMOM_GEMM(NS)                                                                                                              \
  hipLaunchKernelGGL(k_zmom_gemm<NS>, grid, dim3(kThreads), 0, st, pl.n_mu, pl.L, pl.l_pad, pl.nG, pl.m_first, pl.M, pitch,        \
                     pl.d_slot.get(), pl.d_lmax.get(), pl.d_greek.get(), pl.d_tab.get(), Zpp, Zmp, pitch0, Zpp0, Zmp0)
  if (pl.n == 1) ZMOM_GEMM(1);
  else if (pl.n == 3) ZMOM_GEMM(3);
  else ZMOM_GEMM(4);
#undef ZMOM_GEMM
  return hipGetLastError();
}

hipError_t mom_zmom_couples(MomZmomPlan &pl, hipStream_t st, int K, const double *Zpp, const double *Zmp, int pitch, int *coupled) {
  const int N = pl.n * pl.n_mu;
  const size_t total = (size_t)N * N * K;
  if (!pl.d_flag) PCHK(pl.d_flag.renew(1));
  PCHK(hipMemsetAsync(pl.d_flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_zmom_couples, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, N, pl.n, pitch, K, Zpp, Zmp, pl.d_flag.get());
  PCHK(hipGetLastError());
  PCHK(hipMemcpyAsync(coupled, pl.d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);
}
