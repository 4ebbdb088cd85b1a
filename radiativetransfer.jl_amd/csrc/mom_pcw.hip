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
// mom_mie_pcw_dual runs the same five kernels with Jacobian rows: up to three weight rows (w_x and its partials in a size
// parameter: every sum is linear in w) and, with MOM_PCW_INDEX_ROWS, d / dn_r and d / dn_i of row 0 from the Dual form of (a).  The
// kernels are templates over the row counts; a row's statements do not depend on them, so a weight row is bitwise the value call's.
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
// planes: Re a, Im a, Re b, Im b at stride ps; diag [nO, 4, Np]: |a + b|^2, |a - b|^2, |a|^2 + |b|^2, Re(a + b), weighted, one row
// per weight row w [NW, ld]: a row's statements do not depend on NW.  IDX: planes 4 .. 7 hold a' = da / dm, b' = db / dm, and two
// more rows follow, d / dn_r and d / dn_i of row 0.  Each quantity takes ONE complex sum, z = sum w_0 conj(u) u' for |u|^2 and
// sum w_0 u' for Re u: d / dn_r u = u' and d / dn_i u = i u' (Cauchy-Riemann), so the rows are (2 Re z, -2 Im z) and (Re z, -Im z).
template <int NW, bool IDX>
__global__ void __launch_bounds__(64) k_pcw_diag(int nR, int ld, int Np, size_t ps, const double *__restrict__ pl, const double *__restrict__ w,
                                                 double *__restrict__ diag) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const double *aR = pl + (size_t)p * ld, *aI = aR + ps, *bR = aI + ps, *bI = bR + ps;
  double s[NW][4], zr[4] = {0.0, 0.0, 0.0, 0.0}, zi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < NW; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[k][q] = 0.0;
  for (int i = lane; i < nR; i += 64) {
    const double ar = aR[i], ai = aI[i], br = bR[i], bi = bI[i];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const double wi = w[(size_t)k * ld + i];
      s[k][0] += wi * ((ar + br) * (ar + br) + (ai + bi) * (ai + bi));
      s[k][1] += wi * ((ar - br) * (ar - br) + (ai - bi) * (ai - bi));
      s[k][2] += wi * ((ar * ar + ai * ai) + (br * br + bi * bi));
      s[k][3] += wi * (ar + br);
    }
    if constexpr (IDX) {
      const double dar = aR[4 * ps + i], dai = aI[4 * ps + i], dbr = bR[4 * ps + i], dbi = bI[4 * ps + i], wi = w[i];
      const double pr = ar + br, pi = ai + bi, mr = ar - br, mi = ai - bi, dpr = dar + dbr, dpi = dai + dbi, dmr = dar - dbr, dmi = dai - dbi;
      zr[0] += wi * (pr * dpr + pi * dpi), zi[0] += wi * (pr * dpi - pi * dpr);
      zr[1] += wi * (mr * dmr + mi * dmi), zi[1] += wi * (mr * dmi - mi * dmr);
      zr[2] += wi * ((ar * dar + ai * dai) + (br * dbr + bi * dbi)), zi[2] += wi * ((ar * dai - ai * dar) + (br * dbi - bi * dbr));
      zr[3] += wi * dpr, zi[3] += wi * dpi;
    }
  }
#pragma unroll
  for (int k = 0; k < NW; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) s[k][q] += __shfl_xor(s[k][q], off);
      if (lane == 0) diag[((size_t)k * 4 + q) * Np + p] = s[k][q];
    }
  if constexpr (IDX) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) zr[q] += __shfl_xor(zr[q], off), zi[q] += __shfl_xor(zi[q], off);
      const double two = q < 3 ? 2.0 : 1.0;
      if (lane == 0) diag[((size_t)NW * 4 + q) * Np + p] = two * zr[q], diag[((size_t)(NW + 1) * 4 + q) * Np + p] = -two * zi[q];
    }
  }
}

// ---- (c) the Gram product ------------------------------------------------------------------------------------------------
// One wavefront per block: macro tile blockIdx.x of the lower triangle (rows 32 R .., columns 32 C .., R >= C) and the radius
// chunks blockIdx.y, blockIdx.y + G, ...  X is the four planes back to back (ps = Np ld), row = q Np + n - 1.  Operand layouts
// of v_mfma_f64_16x16x4: A lane = A[row lane & 15][k lane >> 4], B lane = B[k lane >> 4][column lane & 15].  K is the contiguous axis,
// so a lane loads FOUR consecutive radii of its row (16 c + 4 (lane >> 4) ..) and step j of the chunk multiplies the j-th of them:
// the four k of a step are 16 c + 4 q + j, q = 0..3, the same in A and B, which permutes the sum over k and nothing else.
// part [NW, G, 4 Np, 4 Np]; the upper macro tiles are never written and never read.  NW weight rows w [NW, ld] share the loads of X
// and the A operand; only b = w_k x differs, so a row's product does not depend on NW.
// SQ: the non-symmetric product Y~ diag(w) X~^T of the index rows, Y the four d / dm planes that follow X (row + 4 Np), masked by the
// same rule: blockIdx.x walks the full square of macro tiles, part [G, 4 Np, 4 Np] is written everywhere.
template <int NW, bool SQ>
__global__ void __launch_bounds__(64) k_pcw_gram(int Np, int ld, int nChunks, int G, const double *__restrict__ X, const double *__restrict__ w,
                                                 const int *__restrict__ nmax, double *__restrict__ part) {
  const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
  const int M = 4 * Np;
  int R, C;
  if constexpr (SQ) {
    R = (int)blockIdx.x / (M / kMacro), C = (int)blockIdx.x % (M / kMacro);
  } else {
    R = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((R + 1) * (R + 2) / 2 <= (int)blockIdx.x) ++R;
    while (R * (R + 1) / 2 > (int)blockIdx.x) --R;
    C = (int)blockIdx.x - R * (R + 1) / 2;
  }
  const double *XA = SQ ? X + (size_t)M * ld : X;  // the A operand's planes
  int row[2], col[2], prow[2], pcol[2];  // X rows of the lane in the two row tiles and the two column tiles; their order index
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    row[t] = kMacro * R + 16 * t + lr, col[t] = kMacro * C + 16 * t + lr;
    prow[t] = row[t] % Np, pcol[t] = col[t] % Np;
  }
  d4 acc[NW][2][2];
#pragma unroll
  for (int k = 0; k < NW; ++k)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[k][s][t] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int c = blockIdx.y; c < nChunks; c += G) {
    const int i0 = kChunk * c + 4 * lq;
    double wk[NW][4];
    int keep[4];  // order index p stays where p + 1 < n_max,i
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      keep[j] = nmax[i0 + j] - 1;
#pragma unroll
      for (int k = 0; k < NW; ++k) wk[k][j] = w[(size_t)k * ld + i0 + j];
    }
    double a[2][4], b[NW][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double va = XA[(size_t)row[t] * ld + i0 + j], vb = X[(size_t)col[t] * ld + i0 + j];
        a[t][j] = prow[t] < keep[j] ? va : 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) b[k][t][j] = pcol[t] < keep[j] ? wk[k][j] * vb : 0.0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NW; ++k)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[k][s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][j], b[k][t][j], acc[k][s][t], 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    double *out = part + ((size_t)k * G + blockIdx.y) * M * M;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)  // C lane, register r = C[row (lane >> 4) + 4 r][column lane & 15]
          out[(size_t)(kMacro * R + 16 * s + lq + 4 * r) * M + kMacro * C + 16 * t + lr] = acc[k][s][t][r];
  }
}

// ---- (d) chunk sum and the planes of (e) -----------------------------------------------------------------------------------
// One lane per pair (n, d = m - n), n fastest.  Q: six planes [Np, Np] by diagonal, [d][n - 1]:
//   0: Re(anam + anbm + bnam + bnbm)   1: Re(anam - anbm - bnam + bnbm)              (compute_PCW.jl:174)
//   2, 3: anam + bnam - anbm - bnbm    4, 5: anam' - bnam' + anbm' - bnbm'           (:151; ' the conjugate)
// each added in the order written there.  diag2 [2, Np]: anan - anbn + bnan - bnbn (:159).  pairs, when given: the four complex
// averages themselves as eight arrays [N, N], entry [m - 1][n - 1] (test access).
// MODE 0: part is the symmetric product of one weight row.  MODE 1 (d / dn_r) and 2 (d / dn_i): part is H = Y~ diag(w_0) X~^T of
// k_pcw_gram<1, true>, and what stands for the product is its derivative dG[(q1, n), (q2, m)] = Hd[(q1, n), (q2, m)] + Hd[(q2, m),
// (q1, n)], Hd the rows of H mapped to the parameter: d / dn_r of a plane pair (Re, Im) is (Re y, Im y), d / dn_i is (-Im y, Re y).
// Everything after g is the same text, so the derivative planes are added in the order of the value planes.
struct PcwPairsOut {
  double *p[8];
};

template <int MODE>
__global__ void __launch_bounds__(256) k_pcw_combine(int N, int Np, int G, const double *__restrict__ part, double *__restrict__ Q,
                                                     double *__restrict__ diag2, PcwPairsOut po) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int pn = (int)(idx % Np), d = (int)(idx / Np), pm = pn + d;
  if (d >= Np || pn >= N || pm >= N) return;
  const int M = 4 * Np;
  const size_t MM = (size_t)M * M;
  // sum_i w_i X~[qa Np + pn, i] X~[qb Np + pm, i]: the product is symmetric, stored where the row's macro tile is not above the column's
  auto chunk_sum = [&](int r1, int r2) {
    const double *p = part + (size_t)r1 * M + r2;
    double v = 0.0;
    for (int c = 0; c < G; ++c) v += p[c * MM];
    return v;
  };
  // row (q, p) of Hd against X row r2: plane q of dX / dn_r is plane q of Y, of dX / dn_i plane q ^ 1 with the sign of i y
  auto hd = [&](int q, int p, int r2) {
    if constexpr (MODE == 1) return chunk_sum(q * Np + p, r2);
    const double v = chunk_sum((q ^ 1) * Np + p, r2);
    return (q & 1) ? v : -v;
  };
  auto g = [&](int qa, int qb) {
    int r1 = qa * Np + pn, r2 = qb * Np + pm;
    if constexpr (MODE != 0) return hd(qa, pn, r2) + hd(qb, pm, r1);
    if (r1 / kMacro < r2 / kMacro) {
      const int t = r1;
      r1 = r2, r2 = t;
    }
    return chunk_sum(r1, r2);
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
// A workgroup is one degree l = 0 .. 2 N - 2 (the reference's l - 1), the highest first: a column's walk is min(2 n, l) steps long, so
// the long workgroups start first and the short ones fill the device behind them.  Thread t takes n = t + 1, t + 1 + 256, ...  A lane
// walks its column from m = n + l down to max(l - n, n): steps with m > N only advance the recursion and read nothing; the terms
// with max(l - n, n + 1) <= m <= min(l + n, N) go into the first sums of compute_Sl, m = n into the second.  diag as k_pcw_diag
// writes it, Q and diag2 as k_pcw_combine.  greek [6, 2 N - 1] in the order alpha, beta, gamma, delta, epsilon, zeta, not divided by
// C_sca.  The 12 sums (first and second of S00, S0-0, S22, S2-2, Re S02, Im S02) are reduced over the workgroup by a fixed tree.
// NO output rows share ONE walk: a lane produces each symbol once and accumulates every row from that row's Q [NO, 6, Np, Np], diag
// [NO, 4, Np] and diag2 [NO, 2, Np] into 12 NO registers; greek [NO, 6, 2 N - 1].  A row's statements and its reduction tree are
// those of NO = 1, so a row does not depend on what else is in the call.  The rows are reduced one after the other through the
// same 24 KiB of LDS.
template <int NO>
__global__ void __launch_bounds__(kSumThreads) k_pcw_sums(int N, int Np, const double *__restrict__ Q, const double *__restrict__ diag,
                                                          const double *__restrict__ diag2, const double *__restrict__ fac, double pi,
                                                          double k2, double *__restrict__ greek) {
#pragma clang fp contract(off)
  __shared__ double red[12][kSumThreads];
  const int l = 2 * N - 2 - (int)blockIdx.x, tid = threadIdx.x;
  const size_t QQ = (size_t)Np * Np;
  const double fl = fac[l];
  double f[NO][6], s[NO][6];
#pragma unroll
  for (int r = 0; r < NO; ++r)
#pragma unroll
    for (int q = 0; q < 6; ++q) f[r][q] = 0.0, s[r][q] = 0.0;
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
#pragma unroll
          for (int r = 0; r < NO; ++r) {
            const double *Qr = Q + (size_t)r * 6 * QQ;
            const double p1 = Qr[o], p2 = Qr[QQ + o];
            f[r][0] += (p1 * (A * A)) * (double)c2;
            f[r][1] += (p2 * (A * A)) * (double)(c2 * sg);
            f[r][2] += (p1 * (B * B)) * (double)c2;
            f[r][3] += (p2 * (B * B)) * (double)(c2 * sg);
            const double ar = (double)sg * Qr[2 * QQ + o] + Qr[4 * QQ + o], ai = (double)sg * Qr[3 * QQ + o] + Qr[5 * QQ + o];
            f[r][4] += ar * 2.0 * (double)c1 * (double)(2 * m + 1) * A * B;
            f[r][5] += ai * 2.0 * (double)c1 * (double)(2 * m + 1) * A * B;
          }
        }
        if (m == n) {
          const long long sgl = (l & 1) ? -1 : 1;
#pragma unroll
          for (int r = 0; r < NO; ++r) {
            const double *dr = diag + (size_t)r * 4 * Np, *d2 = diag2 + (size_t)r * 2 * Np;
            s[r][0] += (dr[n - 1] * (A * A)) * (double)(c1 * c1);
            s[r][1] += (dr[Np + n - 1] * (A * A)) * (double)(c1 * c1 * sgl);
            s[r][2] += (dr[n - 1] * (B * B)) * (double)(c1 * c1);
            s[r][3] += (dr[Np + n - 1] * (B * B)) * (double)(c1 * c1 * sgl);
            s[r][4] += d2[n - 1] * 2.0 * (double)c1 * (double)c1 * A * B;
            s[r][5] += d2[Np + n - 1] * 2.0 * (double)c1 * (double)c1 * A * B;
          }
        }
      }
      if (m == lo) break;
      c.step();
    }
  }
  const size_t L = (size_t)2 * N - 1;
#pragma unroll
  for (int r = 0; r < NO; ++r) {
    // the tree below ends with a barrier, and thread 0 reads only its own slots after it: the next row may be written at once
#pragma unroll
    for (int q = 0; q < 6; ++q) red[q][tid] = f[r][q], red[6 + q][tid] = s[r][q];
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
      double *gr = greek + (size_t)r * 6 * L;
      gr[l] = S[2] + S[3];
      gr[L + l] = S[0] + S[1];
      gr[2 * L + l] = S[4];
      gr[3 * L + l] = S[0] - S[1];
      gr[4 * L + l] = S[5];
      gr[5 * L + l] = S[2] - S[3];
    }
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

// The launches of (b), (c) and (e) by their template arguments
void launch_diag(hipStream_t st, int nW, bool index, int N, int nR, int ld, int Np, size_t ps, const double *pl, const double *w, double *diag) {
#define PCW_DIAG(NW, IDX) hipLaunchKernelGGL((k_pcw_diag<NW, IDX>), dim3(N), dim3(64), 0, st, nR, ld, Np, ps, pl, w, diag)
  switch (2 * nW + (index ? 1 : 0)) {
    case 2: PCW_DIAG(1, false); break;
    case 3: PCW_DIAG(1, true); break;
    case 4: PCW_DIAG(2, false); break;
    case 5: PCW_DIAG(2, true); break;
    case 6: PCW_DIAG(3, false); break;
    default: PCW_DIAG(3, true); break;
  }
#undef PCW_DIAG
}

void launch_gram(hipStream_t st, int nW, int nMacro, int G, int Np, int ld, int nChunks, const double *X, const double *w, const int *nmax,
                 double *part) {
#define PCW_GRAM(NW) hipLaunchKernelGGL((k_pcw_gram<NW, false>), dim3(nMacro, G), dim3(64), 0, st, Np, ld, nChunks, G, X, w, nmax, part)
  switch (nW) {
    case 1: PCW_GRAM(1); break;
    case 2: PCW_GRAM(2); break;
    default: PCW_GRAM(3); break;
  }
#undef PCW_GRAM
}

void launch_sums(hipStream_t st, int nO, int L, int N, int Np, const double *Q, const double *diag, const double *diag2, const double *fac,
                 double k2, double *greek) {
#define PCW_SUMS(NO) hipLaunchKernelGGL((k_pcw_sums<NO>), dim3((unsigned)L), dim3(kSumThreads), 0, st, N, Np, Q, diag, diag2, fac, M_PI, k2, greek)
  switch (nO) {
    case 1: PCW_SUMS(1); break;
    case 2: PCW_SUMS(2); break;
    case 3: PCW_SUMS(3); break;
    case 4: PCW_SUMS(4); break;
    default: PCW_SUMS(5); break;
  }
#undef PCW_SUMS
}

// All four entry points.  w [nW, nR]; index: two more output rows, d / dn_r and d / dn_i of row 0 (nO = nW + 2).  pairs null: greek
// [nO, 6, L] and C [nO, 2]; pairs given, nO x 8 arrays [N, N]: stops after (d).  A weight row k takes the launches, the chunk groups
// (G) and the statements of the single-row call, so its results are bitwise those of mom_mie_pcw(w[k]); the index rows' product has
// a chunk group count of its own (GH), sized for the full square of macro tiles.
int pcw_run(const char *fn, int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i, int N, int flags,
            int known_flags, double *const *pairs, double *greek, double *C, double *gpu_ms) {
  if (nR < 1) return pcw_fail(fn, "nR must be at least 1");
  if (nW < 1 || nW > MOM_PCW_MAX_WEIGHT_ROWS) return pcw_fail(fn, "nW must be 1..3");
  if (!(lambda > 0.0)) return pcw_fail(fn, "lambda must be positive");
  if (!(n_i >= 0.0) || !std::isfinite(n_r) || !std::isfinite(n_i)) return pcw_fail(fn, "n_i must be >= 0 (m = n_r + i n_i)");
  if (N < 1 || N > kMaxOrder) return pcw_fail(fn, "N_max must be 1..640 (MOM_PCW_MAX_ORDER)");
  if (flags & ~known_flags) return pcw_fail(fn, "unknown flag");
  const bool index = (flags & MOM_PCW_INDEX_ROWS) != 0;
  const int nO = nW + (index ? 2 : 0);
  if (!r || !w || (!pairs && (!greek || !C))) return pcw_fail(fn, "null pointer");
  if (pairs)
    for (int q = 0; q < 8 * nO; ++q)
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
  int GH = 4096 / (nRows * nRows);  // the same for the square of the index rows' product
  GH = GH < 1 ? 1 : (GH > nChunks ? nChunks : GH);
  // one allocation, carved in doubles: planes (index: eight) | w [nW, ld] | diag [nO, 4, Np] | diag2 [nO, 2, Np] | fac [L] |
  // Q [nO, 6, Np, Np] | greek [nO, 6, L] | part [nW, G, M, M] | partH [GH, M, M] | pairs [nO, 8, N, N] | the workspace of the
  // coefficient kernel
  const size_t nPl = (index ? 8 : 4) * ps, nQ = 6 * Np * Np, nPart = (size_t)nW * G * M * M, nPartH = index ? (size_t)GH * M * M : 0;
  const size_t nPairs = pairs ? 8 * (size_t)N * N : 0;
  const size_t nDbl = nPl + nW * ld + nO * 6 * Np + L + nO * nQ + nO * 6 * L + nPart + nPartH + nO * nPairs;
  const size_t bytes = nDbl * sizeof(double) + mom_mie_ab::workspace_bytes(N, ld, index);
  const std::vector<double> hfac = pcw_fac((int)L);
  std::vector<double> hdiag((size_t)nO * 4 * Np);
  char *base = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  PCHK(hipSetDevice(device));
  PCHK(hipStreamCreate(&st));
  PCHK(hipMalloc((void **)&base, bytes));
  {
    double *p = (double *)base;
    double *d_pl = p; p += nPl;
    double *d_w = p; p += nW * ld;
    double *d_diag = p; p += nO * 4 * Np;
    double *d_diag2 = p; p += nO * 2 * Np;
    double *d_fac = p; p += L;
    double *d_Q = p; p += nO * nQ;
    double *d_greek = p; p += nO * 6 * L;
    double *d_part = p; p += nPart;
    double *d_partH = p; p += nPartH;
    double *d_pairs = p; p += nO * nPairs;
    const size_t nZero = (size_t)((char *)d_part - base);  // planes (rows above n_max,i, padding), w padding, Q; part is written where read
    const int *d_nmax = nullptr;
    PCHK(hipMemsetAsync(base, 0, nZero, st));
    if (nPairs) PCHK(hipMemsetAsync(d_pairs, 0, nO * nPairs * sizeof(double), st));
    for (int k = 0; k < nW; ++k)
      PCHK(hipMemcpyAsync(d_w + k * ld, w + (size_t)k * nR, (size_t)nR * sizeof(double), hipMemcpyHostToDevice, st));
    PCHK(hipMemcpyAsync(d_fac, hfac.data(), L * sizeof(double), hipMemcpyHostToDevice, st));
    for (int q = 0; q < 4; ++q) PCHK(hipEventCreate(&ev[q]));
    rc = mom_mie_ab::launch(fn, st, nR, ld, hx.data(), n_r, n_i, N, ps, d_pl, (char *)p, nullptr, &d_nmax, ev[0], ev[1], index);
    if (rc != MOM_OK) goto done;
    launch_diag(st, nW, index, N, nR, (int)ld, (int)Np, ps, d_pl, d_w, d_diag);
    PCHK(hipGetLastError());
    launch_gram(st, nW, nMacro, G, (int)Np, (int)ld, nChunks, d_pl, d_w, d_nmax, d_part);
    PCHK(hipGetLastError());
    if (index) {
      hipLaunchKernelGGL((k_pcw_gram<1, true>), dim3(nRows * nRows, GH), dim3(64), 0, st, (int)Np, (int)ld, nChunks, GH, d_pl, d_w, d_nmax, d_partH);
      PCHK(hipGetLastError());
    }
    for (int k = 0; k < nO; ++k) {
      PcwPairsOut po;
      for (int q = 0; q < 8; ++q) po.p[q] = pairs ? d_pairs + ((size_t)k * 8 + q) * N * N : nullptr;
      const dim3 grid((unsigned)((Np * Np + 255) / 256));
      double *Qk = d_Q + k * nQ, *d2k = d_diag2 + k * 2 * Np;
      if (k < nW)
        hipLaunchKernelGGL(k_pcw_combine<0>, grid, dim3(256), 0, st, N, (int)Np, G, d_part + (size_t)k * G * M * M, Qk, d2k, po);
      else if (k == nW)
        hipLaunchKernelGGL(k_pcw_combine<1>, grid, dim3(256), 0, st, N, (int)Np, GH, d_partH, Qk, d2k, po);
      else
        hipLaunchKernelGGL(k_pcw_combine<2>, grid, dim3(256), 0, st, N, (int)Np, GH, d_partH, Qk, d2k, po);
      PCHK(hipGetLastError());
    }
    PCHK(hipEventRecord(ev[2], st));
    if (!pairs) {
      launch_sums(st, nO, (int)L, N, (int)Np, d_Q, d_diag, d_diag2, d_fac, kw * kw, d_greek);
      PCHK(hipGetLastError());
    }
    PCHK(hipEventRecord(ev[3], st));
    if (pairs) {
      for (int q = 0; q < 8 * nO; ++q)
        PCHK(hipMemcpyAsync(pairs[q], d_pairs + (size_t)q * N * N, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
      PCHK(hipMemcpyAsync(greek, d_greek, nO * 6 * L * sizeof(double), hipMemcpyDeviceToHost, st));
      PCHK(hipMemcpyAsync(hdiag.data(), d_diag, hdiag.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PCHK(hipStreamSynchronize(st));
    if (!pairs) {
      // compute_avg_C_scatt_ext: 2 pi / k^2 (2 n + 1) times the weighted sums of k_pcw_diag, added in the order of n, per row
      for (int k = 0; k < nO; ++k) {
        const double *hd = hdiag.data() + (size_t)k * 4 * Np;
        double cs = 0.0, ce = 0.0;
        for (int n = 1; n <= N; ++n) {
          const double coef = 2.0 * M_PI / (kw * kw) * (double)(2 * n + 1);
          cs += coef * hd[2 * Np + n - 1];
          ce += coef * hd[3 * Np + n - 1];
        }
        C[2 * k] = cs, C[2 * k + 1] = ce;
      }
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
  return pcw_run("mom_mie_pcw", device, nR, r, 1, w, lambda, n_r, n_i, N_max, flags, 0, nullptr, greek, C, gpu_ms);
}

extern "C" int mom_mie_pcw_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i, int N_max,
                                int flags, double *greek, double *C, double *gpu_ms) {
  return pcw_run("mom_mie_pcw_dual", device, nR, r, nW, w, lambda, n_r, n_i, N_max, flags, MOM_PCW_INDEX_ROWS, nullptr, greek, C, gpu_ms);
}

extern "C" int mom_pcw_pair_averages(int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N_max,
                                     double *anam_re, double *anam_im, double *anbm_re, double *anbm_im, double *bnam_re, double *bnam_im,
                                     double *bnbm_re, double *bnbm_im) {
  double *const pairs[8] = {anam_re, anam_im, anbm_re, anbm_im, bnam_re, bnam_im, bnbm_re, bnbm_im};
  return pcw_run("mom_pcw_pair_averages", device, nR, r, 1, w, lambda, n_r, n_i, N_max, 0, 0, pairs, nullptr, nullptr, nullptr);
}

extern "C" int mom_pcw_pair_averages_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                                          int N_max, int flags, double *pairs) {
  const char *fn = "mom_pcw_pair_averages_dual";
  if (!pairs) return pcw_fail(fn, "null pointer");
  if (N_max < 1 || N_max > kMaxOrder) return pcw_fail(fn, "N_max must be 1..640 (MOM_PCW_MAX_ORDER)");
  double *out[8 * (MOM_PCW_MAX_WEIGHT_ROWS + 2)];
  for (int q = 0; q < 8 * (MOM_PCW_MAX_WEIGHT_ROWS + 2); ++q) out[q] = pairs + (size_t)q * N_max * N_max;
  return pcw_run(fn, device, nR, r, nW, w, lambda, n_r, n_i, N_max, flags, MOM_PCW_INDEX_ROWS, out, nullptr, nullptr, nullptr);
}

extern "C" int mom_wigner_tables(int device, int m_max, int n_max, int l_max, double *A, double *B) {
  return wigner_tables_run("mom_wigner_tables", device, m_max, n_max, l_max, A, B);
}
