// mom_pcw.hip -- Mie aerosol optics by the Domke-PCW method on gfx950 (Float64): the Greek coefficients expanded directly in the
// Mie coefficients (Sanghavi 2014, eq. 22-24), no scattering-angle quadrature.
//
// Restates compute_aerosol_optical_properties(::MieModel{PCW}) (src/Scattering/compute_PCW.jl:16-193) with compute_avg_anbns! and
// compute_avg_C_scatt_ext (mie_helper_functions.jl:120-144, 258-263) and the Wigner 3j recursions of compute_wigner_values.jl.  The
// reference reads the symbols from two tables [2 N + 1, N + 1, 2 N + 1]; here no table exists: every symbol is produced and used in
// registers.  A call is five launches:
//   (a) k_mie_ab       of mom_mie.hip (through mom_mie_ab.hpp): a_n, b_n of all radii as four planes [Np, ld], radius fastest
//   (b) k_pcw_diag     per order n: sum_i w_i |a_n + b_n|^2, |a_n - b_n|^2, |a_n|^2 + |b_n|^2, Re(a_n + b_n); one wavefront per n
//   (c) k_pcw_gram     X~ diag(w) X~^T for X = [Re a; Im a; Re b; Im b] (4 Np x nR) on v_mfma_f64_16x16x4, K the radius axis: the
//                      lower triangle of 32 x 32 macro tiles, one wavefront each, the radii in G interleaved chunks.  X~ is X without
//                      order n = n_max,i of radius i: the reference takes a radius into a pair average only where both orders are
//                      < n_max,i (strict), which is exactly the product of the masked rows.
//   (d) k_pcw_combine  adds the G partial products in chunk order and forms what (e) reads, per pair (n, m >= n), from the four
//                      complex averages conj(a_n) a_m, conj(a_n) b_m, conj(b_n) a_m, conj(b_n) b_m: six real planes stored BY DIAGONAL,
//                      [m - n][n], so that lanes over n at one step of the walk read consecutive addresses
//   (e) k_pcw_sums     one workgroup per degree l, lanes over n: each lane walks its (n, l) column of symbols downward in m from
//                      m = n + l and accumulates the five sums of compute_Sl; fixed-order reduction; writes the six Greek rows
// Nothing is added with floating-point atomics: two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "momcore.h"
#include "mom_host.hpp"
#include "mom_mie_ab.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kRowPad = 16;      // the planes' row count Np: a 16-row tile never straddles two planes
constexpr int kMacro = 32;       // a wavefront of (c) owns 2 x 2 tiles
constexpr int kChunk = 16;       // radii per K chunk of (c): four MFMA steps, each lane brings four consecutive radii
constexpr int kSumThreads = 256;
// The recursion multiplies three integers below (n + l + 1)^2 as the reference does, in 64 bits: their product stays below 2^63 for
// n + l + 1 < 1990.  A call walks n <= N_max, l <= 2 N_max - 2.
constexpr int kMaxOrder = 640;           // N_max of mom_mie_pcw (MOM_PCW_MAX_ORDER)
constexpr int kMaxTableColumn = 1900;    // n_max + l_max of mom_wigner_tables
constexpr size_t kMaxTableBytes = (size_t)1 << 30;  // mom_wigner_tables: per table

// ---- the symbols of one (n, l) column ------------------------------------------------------------------------------------
// The reference's recursions (compute_wigner_values.jl:24-147) unfolded: wigner3j_m110! recurses upward in m until it meets
// m = n + l (eq. 27, 28: a chain over n) and m = n + l + 1 (zero), so a column is a walk downward from m = n + l with the two
// symbols above in registers; wigner3j_000! is the same in steps of two, and only the parity of n + l survives (the other runs into
// m = n + l + 1).  The operations and their order are the reference's; nothing may be contracted into an FMA.  D_{k+1} of one step
// is D_k of the step before and is carried, not recomputed (the same value).  l is the degree (the tables' third index minus one).
struct WigCol {
  long long n, l, m, d2, s2;
  double a, aup, dup, w;  // (-1, 1, 0) at m and m + 1; D_{m+2}; (0, 0, 0) at the last m of the parity of n + l

  __device__ double D(long long k) const {
#pragma clang fp contract(off)
    return (1.0 / (double)k) * sqrt((double)((k * k - 1) * (k * k - d2) * (s2 - k * k)));
  }
  __device__ void start(int n_, int l_) {
#pragma clang fp contract(off)
    n = n_, l = l_, m = n + l, d2 = (l - n) * (l - n), s2 = (n + l + 1) * (n + l + 1);
    double s = ((l & 1) ? -1.0 : 1.0) * sqrt((double)((l + 1) * (l + 2)) / (double)((2 * l + 1) * (2 * l + 2) * (2 * l + 3)));  // eq. 28
    for (long long j = 2; j <= n; ++j)  // eq. 27
      s = -s * sqrt((double)(j * (2 * j - 1) * ((j + l) * (j + l) - 1)) / (double)((j + l) * (2 * (j + l) + 1) * (j * j - 1)));
    a = s, aup = 0.0, dup = 0.0;
    w = a * 2.0 * sqrt((double)((n + l) * (n + l + 1) * n * (n + 1))) / (double)(l * (l + 1) - (l + n) * (l + n + 1) - n * (n + 1));  // eq. 30
  }
  __device__ void step() {  // m -> m - 1
#pragma clang fp contract(off)
    m -= 1;
    const long long k = m + 1;
    const double dk = D(k), Mk = 1.0 - (double)(n * (n + 1) - l * (l + 1)) / (double)(k * (k + 1));
    const double an = (1.0 / dk) * (Mk * (double)(2 * m + 3) * a - dup * aup);  // eq. 25
    aup = a, a = an, dup = dk;
    if (((n + l - m) & 1) == 0)  // eq. 29
      w = -w * sqrt((double)((m + 2) * (m + 2) - d2) / (double)((m + 1) * (m + 1) - d2)) *
          sqrt((1.0 - (1.0 / (double)(n + l - m))) * (1.0 + (1.0 / (double)(m + n + l + 2))));
  }
  __device__ double w000() const { return ((n + l - m) & 1) ? 0.0 : w; }
  // (-1, -1, 2), eq. 31; fac = ((l - 1) l (l + 1) (l + 2))^(-1/2), l >= 2
  __device__ double b(double fac) const {
#pragma clang fp contract(off)
    const long long sg = ((m + n + l) & 1) ? -1 : 1;
    return ((double)sg * fac) * ((double)(m * (m + 1) + sg * n * (n + 1)) * a + 2.0 * sqrt((double)(m * (m + 1) * n * (n + 1))) * w000());
  }
};

// compute_wigner_values: one lane per (n, l) column; tables [l_max, n_max, m_max] with m fastest, zeroed before
__global__ void __launch_bounds__(64) k_wigner_tables(int m_max, int n_max, int l_max, const double *__restrict__ fac, double *__restrict__ A,
                                                      double *__restrict__ B) {
  const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long long)n_max * l_max) return;
  const int n = (int)(idx % n_max) + 1, l = (int)(idx / n_max);
  const int lo = max(abs(n - l), 1);
  WigCol c;
  c.start(n, l);
  const size_t col = ((size_t)l * n_max + (n - 1)) * m_max;
  for (;;) {
    if (c.m <= m_max) {
      A[col + c.m - 1] = c.a;
      if (l >= 2) B[col + c.m - 1] = c.b(fac[l]);
    }
    if (c.m == lo) break;
    c.step();
  }
}

// ---- (b) the sums over the radii that keep order n = n_max,i ---------------------------------------------------------------
// planes: Re a, Im a, Re b, Im b at stride ps; diag [4, Np]: |a + b|^2, |a - b|^2, |a|^2 + |b|^2, Re(a + b), each weighted
__global__ void __launch_bounds__(64) k_pcw_diag(int nR, int ld, int Np, size_t ps, const double *__restrict__ pl, const double *__restrict__ w,
                                                 double *__restrict__ diag) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const double *aR = pl + (size_t)p * ld, *aI = aR + ps, *bR = aI + ps, *bI = bR + ps;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < nR; i += 64) {
    const double ar = aR[i], ai = aI[i], br = bR[i], bi = bI[i], wi = w[i];
    s[0] += wi * ((ar + br) * (ar + br) + (ai + bi) * (ai + bi));
    s[1] += wi * ((ar - br) * (ar - br) + (ai - bi) * (ai - bi));
    s[2] += wi * ((ar * ar + ai * ai) + (br * br + bi * bi));
    s[3] += wi * (ar + br);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s[q] += __shfl_xor(s[q], off);
    if (lane == 0) diag[(size_t)q * Np + p] = s[q];
  }
}

// ---- (c) the Gram product ------------------------------------------------------------------------------------------------
// One wavefront per block: macro tile blockIdx.x of the lower triangle (rows 32 R .., columns 32 C .., R >= C) and the radius
// chunks blockIdx.y, blockIdx.y + G, ...  X is the four planes back to back (ps = Np ld), row = q Np + n - 1.  Operand layouts
// of v_mfma_f64_16x16x4: A lane = A[row lane & 15][k lane >> 4], B lane = B[k lane >> 4][column lane & 15].  K is the contiguous axis,
// so a lane loads FOUR consecutive radii of its row (16 c + 4 (lane >> 4) ..) and step j of the chunk multiplies the j-th of them:
// the four k of a step are 16 c + 4 q + j, q = 0..3, the same in A and B, which permutes the sum over k and nothing else.
// part [G, 4 Np, 4 Np]; the upper macro tiles are never written and never read.
__global__ void __launch_bounds__(64) k_pcw_gram(int Np, int ld, int nChunks, int G, const double *__restrict__ X, const double *__restrict__ w,
                                                 const int *__restrict__ nmax, double *__restrict__ part) {
  const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
  int R = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((R + 1) * (R + 2) / 2 <= (int)blockIdx.x) ++R;
  while (R * (R + 1) / 2 > (int)blockIdx.x) --R;
  const int C = (int)blockIdx.x - R * (R + 1) / 2;
  const int M = 4 * Np;
  int row[2], col[2], prow[2], pcol[2];  // X rows of the lane in the two row tiles and the two column tiles; their order index
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    row[t] = kMacro * R + 16 * t + lr, col[t] = kMacro * C + 16 * t + lr;
    prow[t] = row[t] % Np, pcol[t] = col[t] % Np;
  }
  d4 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[s][t] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int c = blockIdx.y; c < nChunks; c += G) {
    const int i0 = kChunk * c + 4 * lq;
    double wk[4];
    int keep[4];  // order index p stays where p + 1 < n_max,i
#pragma unroll
    for (int j = 0; j < 4; ++j) wk[j] = w[i0 + j], keep[j] = nmax[i0 + j] - 1;
    double a[2][4], b[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double va = X[(size_t)row[t] * ld + i0 + j], vb = X[(size_t)col[t] * ld + i0 + j];
        a[t][j] = prow[t] < keep[j] ? va : 0.0;
        b[t][j] = pcol[t] < keep[j] ? wk[j] * vb : 0.0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][j], b[t][j], acc[s][t], 0, 0, 0);
  }
  double *out = part + (size_t)blockIdx.y * M * M;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C lane, register r = C[row (lane >> 4) + 4 r][column lane & 15]
        out[(size_t)(kMacro * R + 16 * s + lq + 4 * r) * M + kMacro * C + 16 * t + lr] = acc[s][t][r];
}

// ---- (d) chunk sum and the planes of (e) -----------------------------------------------------------------------------------
// One lane per pair (n, d = m - n), n fastest.  Q: six planes [Np, Np] by diagonal, [d][n - 1]:
//   0: Re(anam + anbm + bnam + bnbm)   1: Re(anam - anbm - bnam + bnbm)              (compute_PCW.jl:174)
//   2, 3: anam + bnam - anbm - bnbm    4, 5: anam' - bnam' + anbm' - bnbm'           (:151; ' the conjugate)
// each added in the order written there.  diag2 [2, Np]: anan - anbn + bnan - bnbn (:159).  pairs, when given: the four complex
// averages themselves as eight arrays [N, N], entry [m - 1][n - 1] (test access).
struct PcwPairsOut {
  double *p[8];
};

__global__ void __launch_bounds__(256) k_pcw_combine(int N, int Np, int G, const double *__restrict__ part, double *__restrict__ Q,
                                                     double *__restrict__ diag2, PcwPairsOut po) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int pn = (int)(idx % Np), d = (int)(idx / Np), pm = pn + d;
  if (d >= Np || pn >= N || pm >= N) return;
  const int M = 4 * Np;
  const size_t MM = (size_t)M * M;
  // sum_i w_i X~[qa Np + pn, i] X~[qb Np + pm, i]: the product is symmetric, stored where the row's macro tile is not above the column's
  auto g = [&](int qa, int qb) {
    int r1 = qa * Np + pn, r2 = qb * Np + pm;
    if (r1 / kMacro < r2 / kMacro) {
      const int t = r1;
      r1 = r2, r2 = t;
    }
    const double *p = part + (size_t)r1 * M + r2;
    double v = 0.0;
    for (int c = 0; c < G; ++c) v += p[c * MM];
    return v;
  };
  // conj(u_n) v_m = (ur_n vr_m + ui_n vi_m) + i (ur_n vi_m - ui_n vr_m); planes: 0 Re a, 1 Im a, 2 Re b, 3 Im b
  double re[4], im[4];  // anam, anbm, bnam, bnbm
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      re[2 * u + v] = g(2 * u, 2 * v) + g(2 * u + 1, 2 * v + 1);
      im[2 * u + v] = g(2 * u, 2 * v + 1) - g(2 * u + 1, 2 * v);
    }
  const size_t o = (size_t)d * Np + pn, QQ = (size_t)Np * Np;
  Q[o] = ((re[0] + re[1]) + re[2]) + re[3];
  Q[QQ + o] = ((re[0] - re[1]) - re[2]) + re[3];
  Q[2 * QQ + o] = ((re[0] + re[2]) - re[1]) - re[3];
  Q[3 * QQ + o] = ((im[0] + im[2]) - im[1]) - im[3];
  Q[4 * QQ + o] = ((re[0] - re[2]) + re[1]) - re[3];
  Q[5 * QQ + o] = ((-im[0] + im[2]) - im[1]) + im[3];
  if (d == 0) {
    diag2[pn] = ((re[0] - re[1]) + re[2]) - re[3];
    diag2[Np + pn] = ((im[0] - im[1]) + im[2]) - im[3];
  }
  if (po.p[0]) {
    const size_t e = (size_t)pm * N + pn;
#pragma unroll
    for (int q = 0; q < 4; ++q) po.p[2 * q][e] = re[q], po.p[2 * q + 1][e] = im[q];
  }
}

// ---- (e) the symbols and the sums S_l, fused --------------------------------------------------------------------------------
// Workgroup blockIdx.x is the degree l = 0 .. 2 N - 2 (the reference's l - 1), thread t takes n = t + 1, t + 1 + 256, ...  A lane
// walks its column from m = n + l down to max(l - n, n): steps with m > N only advance the recursion and read nothing; the terms
// with max(l - n, n + 1) <= m <= min(l + n, N) go into the first sums of compute_Sl, m = n into the second.  diag as k_pcw_diag
// writes it, Q and diag2 as k_pcw_combine.  greek [6, 2 N - 1] in the order alpha, beta, gamma, delta, epsilon, zeta, not divided by
// C_sca.  The 12 sums (first and second of S00, S0-0, S22, S2-2, Re S02, Im S02) are reduced over the workgroup by a fixed tree.
__global__ void __launch_bounds__(kSumThreads) k_pcw_sums(int N, int Np, const double *__restrict__ Q, const double *__restrict__ diag,
                                                          const double *__restrict__ diag2, const double *__restrict__ fac, double pi,
                                                          double k2, double *__restrict__ greek) {
#pragma clang fp contract(off)
  __shared__ double red[12][kSumThreads];
  const int l = blockIdx.x, tid = threadIdx.x;
  const size_t QQ = (size_t)Np * Np;
  const double fl = fac[l];
  double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int n = tid + 1; n <= N; n += kSumThreads) {
    const int lo = max(l - n, n), m_star = max(l - n, n + 1);
    if (lo > N) continue;
    const long long c1 = 2 * n + 1;
    WigCol c;
    c.start(n, l);
    for (;;) {
      const int m = (int)c.m;
      if (m <= N) {
        const double A = c.a, B = l >= 2 ? c.b(fl) : 0.0;
        if (m >= m_star) {
          const size_t o = (size_t)(m - n) * Np + (n - 1);
          const long long sg = ((l + n + m) & 1) ? -1 : 1, c2 = 2 * (2 * (long long)m + 1) * c1;
          const double p1 = Q[o], p2 = Q[QQ + o];
          f[0] += (p1 * (A * A)) * (double)c2;
          f[1] += (p2 * (A * A)) * (double)(c2 * sg);
          f[2] += (p1 * (B * B)) * (double)c2;
          f[3] += (p2 * (B * B)) * (double)(c2 * sg);
          const double ar = (double)sg * Q[2 * QQ + o] + Q[4 * QQ + o], ai = (double)sg * Q[3 * QQ + o] + Q[5 * QQ + o];
          f[4] += ar * 2.0 * (double)c1 * (double)(2 * m + 1) * A * B;
          f[5] += ai * 2.0 * (double)c1 * (double)(2 * m + 1) * A * B;
        }
        if (m == n) {
          const long long sgl = (l & 1) ? -1 : 1;
          s[0] += (diag[n - 1] * (A * A)) * (double)(c1 * c1);
          s[1] += (diag[Np + n - 1] * (A * A)) * (double)(c1 * c1 * sgl);
          s[2] += (diag[n - 1] * (B * B)) * (double)(c1 * c1);
          s[3] += (diag[Np + n - 1] * (B * B)) * (double)(c1 * c1 * sgl);
          s[4] += diag2[n - 1] * 2.0 * (double)c1 * (double)c1 * A * B;
          s[5] += diag2[Np + n - 1] * 2.0 * (double)c1 * (double)c1 * A * B;
        }
      }
      if (m == lo) break;
      c.step();
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) red[q][tid] = f[q], red[6 + q][tid] = s[q];
  __syncthreads();
  for (int h = kSumThreads / 2; h > 0; h >>= 1) {
    if (tid < h)
#pragma unroll
      for (int q = 0; q < 12; ++q) red[q][tid] += red[q][tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double coef = (double)(2 * l + 1) * pi / k2;
    double S[6];  // S00, S0-0, S22, S2-2, Re S02, Im S02
#pragma unroll
    for (int q = 0; q < 6; ++q) S[q] = coef * (red[q][0] + red[6 + q][0]);
    const size_t L = (size_t)2 * N - 1;
    greek[l] = S[2] + S[3];
    greek[L + l] = S[0] + S[1];
    greek[2 * L + l] = S[4];
    greek[3 * L + l] = S[0] - S[1];
    greek[4 * L + l] = S[5];
    greek[5 * L + l] = S[2] - S[3];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int pcw_fail(const char *fn, const char *what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  mom_set_global_error(buf);
  return MOM_EINVAL;
}

int pcw_device(const char *fn, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    char buf[128];
    snprintf(buf, sizeof buf, "%s: no HIP device available", fn);
    mom_set_global_error(buf);
    return MOM_EHIP;
  }
  if (device < 0 || device >= ndev) return pcw_fail(fn, "device index out of range");
  return MOM_OK;
}

#define PCHK(call)                                                                                     \
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

inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// ((l - 1) l (l + 1) (l + 2))^(-0.5) for l = 0 .. n - 1 (eq. 31), by the host library's pow; 0 below l = 2, where the reference
// answers 0 for the symbol before it reaches the power
std::vector<double> pcw_fac(int n) {
  std::vector<double> f((size_t)n, 0.0);
  for (long long l = 2; l < n; ++l) f[(size_t)l] = std::pow((double)((l - 1) * l * (l + 1) * (l + 2)), -0.5);
  return f;
}

// mom_mie_pcw (pairs null) and mom_pcw_pair_averages (pairs given: stops after (d))
int pcw_run(const char *fn, int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N, int flags,
            double *const *pairs, double *greek, double *C, double *gpu_ms) {
  if (nR < 1) return pcw_fail(fn, "nR must be at least 1");
  if (!(lambda > 0.0)) return pcw_fail(fn, "lambda must be positive");
  if (!(n_i >= 0.0) || !std::isfinite(n_r) || !std::isfinite(n_i)) return pcw_fail(fn, "n_i must be >= 0 (m = n_r + i n_i)");
  if (N < 1 || N > kMaxOrder) return pcw_fail(fn, "N_max must be 1..640 (MOM_PCW_MAX_ORDER)");
  if (flags != 0) return pcw_fail(fn, "unknown flag");
  if (!r || !w || (!pairs && (!greek || !C))) return pcw_fail(fn, "null pointer");
  if (pairs)
    for (int q = 0; q < 8; ++q)
      if (!pairs[q]) return pcw_fail(fn, "null pointer");
  if (!(r[0] > 0.0) || !std::isfinite(r[nR - 1])) return pcw_fail(fn, "r[0] must be positive and r finite");
  for (int i = 1; i < nR; ++i)
    if (!(r[i] > r[i - 1])) return pcw_fail(fn, "r must be ascending");
  const double kw = 2.0 * M_PI / lambda;  // wavenumber
  std::vector<double> hx((size_t)nR);
  for (int i = 0; i < nR; ++i) {
    hx[i] = kw * r[i];
    if (mom_mie_ab::n_max_of(hx[i]) > N) return pcw_fail(fn, "N_max is smaller than the largest per-radius n_max");
  }
  int rc = pcw_device(fn, device);
  if (rc != MOM_OK) return rc;

  const size_t ld = round_up(nR, kChunk), Np = round_up(N, kRowPad), M = 4 * Np, ps = Np * ld, L = 2 * (size_t)N - 1;
  const int nChunks = (int)(ld / kChunk), nRows = (int)(M / kMacro), nMacro = nRows * (nRows + 1) / 2;
  int G = 4096 / nMacro;  // about four wavefronts per SIMD of the device
  G = G < 1 ? 1 : (G > nChunks ? nChunks : G);
  // one allocation, carved in doubles: planes | w | diag [4, Np] | diag2 [2, Np] | fac [L] | Q [6, Np, Np] | greek [6, L] |
  // part [G, M, M] | pairs [8, N, N] | the workspace of the coefficient kernel
  const size_t nQ = 6 * Np * Np, nPart = (size_t)G * M * M, nPairs = pairs ? 8 * (size_t)N * N : 0;
  const size_t nDbl = 4 * ps + ld + 6 * Np + L + nQ + 6 * L + nPart + nPairs;
  const size_t bytes = nDbl * sizeof(double) + mom_mie_ab::workspace_bytes(N, ld);
  const std::vector<double> hfac = pcw_fac((int)L);
  std::vector<double> hdiag(4 * Np);
  char *base = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  PCHK(hipSetDevice(device));
  PCHK(hipStreamCreate(&st));
  PCHK(hipMalloc((void **)&base, bytes));
  {
    double *p = (double *)base;
    double *d_pl = p; p += 4 * ps;
    double *d_w = p; p += ld;
    double *d_diag = p; p += 4 * Np;
    double *d_diag2 = p; p += 2 * Np;
    double *d_fac = p; p += L;
    double *d_Q = p; p += nQ;
    double *d_greek = p; p += 6 * L;
    double *d_part = p; p += nPart;
    double *d_pairs = p; p += nPairs;
    const size_t nZero = (size_t)((char *)d_part - base);  // planes (rows above n_max,i, padding), w padding, Q; part is written where read
    const int *d_nmax = nullptr;
    PCHK(hipMemsetAsync(base, 0, nZero, st));
    if (nPairs) PCHK(hipMemsetAsync(d_pairs, 0, nPairs * sizeof(double), st));
    PCHK(hipMemcpyAsync(d_w, w, (size_t)nR * sizeof(double), hipMemcpyHostToDevice, st));
    PCHK(hipMemcpyAsync(d_fac, hfac.data(), L * sizeof(double), hipMemcpyHostToDevice, st));
    for (int q = 0; q < 4; ++q) PCHK(hipEventCreate(&ev[q]));
    rc = mom_mie_ab::launch(fn, st, nR, ld, hx.data(), n_r, n_i, N, ps, d_pl, (char *)p, nullptr, &d_nmax, ev[0], ev[1]);
    if (rc != MOM_OK) goto done;
    hipLaunchKernelGGL(k_pcw_diag, dim3(N), dim3(64), 0, st, nR, (int)ld, (int)Np, ps, d_pl, d_w, d_diag);
    PCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pcw_gram, dim3(nMacro, G), dim3(64), 0, st, (int)Np, (int)ld, nChunks, G, d_pl, d_w, d_nmax, d_part);
    PCHK(hipGetLastError());
    {
      PcwPairsOut po;
      for (int q = 0; q < 8; ++q) po.p[q] = pairs ? d_pairs + (size_t)q * N * N : nullptr;
      hipLaunchKernelGGL(k_pcw_combine, dim3((unsigned)((Np * Np + 255) / 256)), dim3(256), 0, st, N, (int)Np, G, d_part, d_Q, d_diag2, po);
      PCHK(hipGetLastError());
    }
    PCHK(hipEventRecord(ev[2], st));
    if (!pairs) {
      hipLaunchKernelGGL(k_pcw_sums, dim3((unsigned)L), dim3(kSumThreads), 0, st, N, (int)Np, d_Q, d_diag, d_diag2, d_fac, M_PI, kw * kw, d_greek);
      PCHK(hipGetLastError());
    }
    PCHK(hipEventRecord(ev[3], st));
    if (pairs) {
      for (int q = 0; q < 8; ++q)
        PCHK(hipMemcpyAsync(pairs[q], d_pairs + (size_t)q * N * N, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
      PCHK(hipMemcpyAsync(greek, d_greek, 6 * L * sizeof(double), hipMemcpyDeviceToHost, st));
      PCHK(hipMemcpyAsync(hdiag.data(), d_diag, 4 * Np * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PCHK(hipStreamSynchronize(st));
    if (!pairs) {
      // compute_avg_C_scatt_ext: 2 pi / k^2 (2 n + 1) times the weighted sums of k_pcw_diag, added in the order of n
      double cs = 0.0, ce = 0.0;
      for (int n = 1; n <= N; ++n) {
        const double coef = 2.0 * M_PI / (kw * kw) * (double)(2 * n + 1);
        cs += coef * hdiag[2 * Np + n - 1];
        ce += coef * hdiag[3 * Np + n - 1];
      }
      C[0] = cs, C[1] = ce;
    }
    if (gpu_ms)
      for (int q = 0; q < 3; ++q) {
        float t = 0.f;
        PCHK(hipEventElapsedTime(&t, ev[q], ev[q + 1]));
        gpu_ms[q] = t;
      }
  }
done:
  for (int q = 0; q < 4; ++q)
    if (ev[q]) (void)hipEventDestroy(ev[q]);
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

int wigner_tables_run(const char *fn, int device, int m_max, int n_max, int l_max, double *A, double *B) {
  if (m_max < 1 || n_max < 1 || l_max < 1) return pcw_fail(fn, "m_max, n_max and l_max must be at least 1");
  if (!A || !B) return pcw_fail(fn, "null pointer");
  // the walk of a column starts at m = n + l - 1 whatever m_max is
  if ((long long)n_max + l_max > kMaxTableColumn) return pcw_fail(fn, "n_max + l_max must be at most 1900");
  const size_t n = (size_t)m_max * n_max * l_max;
  if ((size_t)m_max > kMaxTableBytes / sizeof(double) / n_max / l_max)
    return pcw_fail(fn, "a table would be larger than MOM_WIGNER_MAX_TABLE_BYTES (1 GiB)");
  int rc = pcw_device(fn, device);
  if (rc != MOM_OK) return rc;
  const std::vector<double> hfac = pcw_fac(l_max);
  char *base = nullptr;
  hipStream_t st = nullptr;
  PCHK(hipSetDevice(device));
  PCHK(hipStreamCreate(&st));
  PCHK(hipMalloc((void **)&base, (2 * n + l_max) * sizeof(double)));
  {
    double *d_A = (double *)base, *d_B = d_A + n, *d_fac = d_B + n;
    PCHK(hipMemsetAsync(base, 0, 2 * n * sizeof(double), st));
    PCHK(hipMemcpyAsync(d_fac, hfac.data(), (size_t)l_max * sizeof(double), hipMemcpyHostToDevice, st));
    const long long cols = (long long)n_max * l_max;
    hipLaunchKernelGGL(k_wigner_tables, dim3((unsigned)((cols + 63) / 64)), dim3(64), 0, st, m_max, n_max, l_max, d_fac, d_A, d_B);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(A, d_A, n * sizeof(double), hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(B, d_B, n * sizeof(double), hipMemcpyDeviceToHost, st));
    PCHK(hipStreamSynchronize(st));
  }
done:
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

}  // namespace

extern "C" int mom_mie_pcw(int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N_max, int flags,
                           double *greek, double *C, double *gpu_ms) {
  return pcw_run("mom_mie_pcw", device, nR, r, w, lambda, n_r, n_i, N_max, flags, nullptr, greek, C, gpu_ms);
}

extern "C" int mom_pcw_pair_averages(int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N_max,
                                     double *anam_re, double *anam_im, double *anbm_re, double *anbm_im, double *bnam_re, double *bnam_im,
                                     double *bnbm_re, double *bnbm_im) {
  double *const pairs[8] = {anam_re, anam_im, anbm_re, anbm_im, bnam_re, bnam_im, bnbm_re, bnbm_im};
  return pcw_run("mom_pcw_pair_averages", device, nR, r, w, lambda, n_r, n_i, N_max, 0, pairs, nullptr, nullptr, nullptr);
}

extern "C" int mom_wigner_tables(int device, int m_max, int n_max, int l_max, double *A, double *B) {
  return wigner_tables_run("mom_wigner_tables", device, m_max, n_max, l_max, A, B);
}
