// mom_trunc.hip -- the delta-BGE truncation of Greek coefficients on gfx950 (Float64).
//
// Restates truncate_phase(mod::dBGE, aero) (src/Scattering/truncate_phase.jl:95-220) as scattering.truncate_phase writes it, with the
// forward-mode partials of that function, for a batch of nG Greek sets of one length l_full, each with nP derivative sets.  The three
// weighted least-squares fits (beta on P, gamma and epsilon on fac P2 from degree 2) run over all n_mu Gauss nodes.  Every matrix and
// right-hand side of the value run and of the forward-mode run is one product G(d) = B^T diag(d) B with one more column B^T d':
//   A = G(w / f^2), b = B^T (w / f);  dA = G(-2 w df / f^3), db = B^T (-w df / f^2);  A c = b,  A dc = db - dA c.
// Launches:
//   (t) k_mie_tables  (mom_mie.hip, through mom_host.hpp) P and P2 [l_full, n_mu] from the nodes, bitwise the host's.
//   (w) k_trunc_weights  one lane per (node, fit, set): f = P beta, P2 (fac gamma), P2 (fac epsilon) over all l_full terms, the same
//                        map of every derivative set, and from them d and d' of the 1 + nP products.  The sums carry their rounding
//                        errors along (TwoProduct / TwoSum), so f is the sum of the Float64 products rounded once whatever the
//                        order: at the back-scattering nodes the terms are 10^4 times their sum.  A divisor that is zero or
//                        not finite sets bit `fit` of the set's status word and leaves d = d' = 0: nothing is divided by it.
//   (g) k_trunc_gram     G(d) and B^T d' on v_mfma_f64_16x16x4, one product per (set, fit, row of the Dual): the factor diag(d) B
//                        with d' as its column l_q is formed while it is staged in LDS, 16 nodes at a time.  Only the lower triangle
//                        of 64 x 64 tiles and the tile that holds column l_q are computed; the edges of n_mu and l_q are predicated.
//   (s) k_trunc_solve    one workgroup per (set, fit): Cholesky of A in LDS, the value solve, the nP right-hand sides db - dA c
//                        against the same factor, the quotient rules and the stores.  A pivot that is not positive and finite sets
//                        the status bit and is replaced by 1: no branch or trip count depends on the data.
//                        Each solution then takes ONE correction from the residual at the nodes (the corrected semi-normal
//                        equations): x += A^-1 B^T (w / f) t with t = 1 - B c / f for the value and t = (df / f) (2 B c / f - 1) -
//                        B dc / f for a partial.  The error of the normal equations, of the order cond(A) 2^-52, comes from the
//                        rounding of A; the residual is formed from B itself, so what is left is of the order sqrt(cond(A)) 2^-52
//                        (DESIGN section 4 has the measured distances with and without the step).
//   (m) k_trunc_mark     the rows of a set whose status word is not zero become NaN.
// Every sum has a fixed order that depends on the set's own data and on (n_mu, l_full, l_tr) only: two calls are bitwise equal and a
// set's rows do not depend on the batch.  The host part is a plan and a launch (MomTruncPlan, mom_host.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "momcore.h"
#include "mom_host.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;     // output tile of a workgroup: 64 x 64, four wavefronts of 32 x 32 (2 x 2 MFMA tiles each)
constexpr int kKStep = 16;    // nodes staged per step: four MFMA k-steps
constexpr int kLd = 80;       // LDS row pitch in doubles: the four k rows a wavefront reads at once start 32 banks apart
constexpr int kThreads = 256;
constexpr int kMax = kMomTruncMax;  // edge of the largest normal matrix
constexpr int kLdA = kMax + 1;      // its row pitch in LDS: a column walk touches every bank once
constexpr int kRhs = 4;             // right-hand sides solved together
// the solve's LDS: the factor, kRhs right-hand sides and kRhs solutions under correction, the value solution and the diagonal
constexpr size_t kSolveLds = ((size_t)kMax * kLdA + (size_t)(2 * kRhs + 2) * kMax) * sizeof(double);
static_assert(kSolveLds == 142336 && kSolveLds <= 160 * 1024, "the solve's LDS image has to fit a CU");
// rows [n_mu] of a (set, fit) in D behind d, d' of its R products: 1 / f, B c / f, and kRhs node vectors of the correction step
constexpr int kNodeRows = 2 + kRhs;
constexpr size_t kGramWorkspace = (size_t)1 << 30;  // bytes the Gram products of one sub-batch of sets may take

__device__ __forceinline__ int fit_row(int q) { return q == 0 ? 1 : (q == 1 ? 2 : 4); }  // beta, gamma, epsilon of alpha .. zeta

// ---- (w) phase functions and diagonal weights -------------------------------------------------------------------------------
// s + e += a b with the rounding errors of the product and of the sum kept in e (Ogita, Rump, Oishi: Dot2)
__device__ __forceinline__ void dot2_step(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
  const double p = a * b, pe = __builtin_fma(a, b, -p);
  const double t = s + p, bb = t - s;
  e += ((s - (t - bb)) + (p - bb)) + pe;
  s = t;
}

// greek [l_full, 6, R, nG] (R = 1 + nP), P / P2 [l_full, n_mu], fac [l_full] (zero below degree 2).
// D [nG, 3, 2 R + kNodeRows, n_mu]: d and d' of product (set, fit, row), then 1 / f (0 for a refused divisor) and the rows the solve
// uses as scratch.  grid (nodes / 64, fits, sets)
__global__ void __launch_bounds__(64) k_trunc_weights(int n_mu, int l_full, int R, const double *__restrict__ w_mu,
                                                      const double *__restrict__ greek, const double *__restrict__ P,
                                                      const double *__restrict__ P2, const double *__restrict__ fac,
                                                      double *__restrict__ D, int *__restrict__ status) {
  const int i = blockIdx.x * 64 + threadIdx.x, q = blockIdx.y, g = blockIdx.z;
  if (i >= n_mu) return;
  const double *tab = (q == 0 ? P : P2) + i;
  const double w = w_mu[i];
  double *o = D + ((size_t)(g * 3 + q) * (2 * R + kNodeRows)) * n_mu + i;
  double f = 0.0, wf = 0.0, wff = 0.0;
  bool ok = true;
  for (int r = 0; r < R; ++r) {
    const double *gk = greek + (size_t)l_full * (fit_row(q) + 6 * (r + (size_t)R * g));
    double s = 0.0, e = 0.0;
    for (int l = q == 0 ? 0 : 2; l < l_full; ++l) dot2_step(tab[(size_t)l * n_mu], q == 0 ? gk[l] : fac[l] * gk[l], s, e);
    s += e;
    double d = 0.0, d1 = 0.0;
    if (r == 0) {
      f = s;
      ok = f != 0.0 && isfinite(f);
      if (ok) {
        wf = w / f;
        wff = wf / f;
        d = wff;
        d1 = wf;
      } else {
        atomicOr(status + g, 1 << q);
      }
      o[(size_t)(2 * R) * n_mu] = ok ? 1.0 / f : 0.0;
    } else if (ok) {
      const double df = s / f;
      d = -2.0 * wff * df;
      d1 = -(wf * df);
    }
    o[(size_t)(2 * r) * n_mu] = d;
    o[(size_t)(2 * r + 1) * n_mu] = d1;
  }
}

// ---- (g) the weighted Gram products -----------------------------------------------------------------------------------------
// Product (set g, fit q, row r): G[a][b] = sum_i B[i][a] d[i] B[i][b] for b < l_q and G[a][l_q] = sum_i B[i][a] d'[i], with
// B[i][a] = P[a][i] (q = 0, l_q = l_tr) or fac[2 + a] P2[2 + a][i] (q = 1, 2, l_q = l_tr - 2), stored as rows a of pitch l_tr + 1
// in block (g, q, r) of Gm.  grid (row tiles x column tiles, fit x row, sets); a tile that is neither in the lower triangle nor
// the one of column l_q ends at once.  The MFMA's row index runs over a, its column index (on the lanes) over b.
__global__ void __launch_bounds__(kThreads) k_trunc_gram(int n_mu, int l_tr, int R, int tilesC, const double *__restrict__ P,
                                                         const double *__restrict__ P2, const double *__restrict__ fac,
                                                         const double *__restrict__ D, double *__restrict__ Gm) {
  __shared__ double Xs[kKStep][kLd];  // B[i][a] at [k][a of the tile]
  __shared__ double Ys[kKStep][kLd];  // d[i] B[i][b], d'[i] at b = l_q, at [k][b of the tile]
  const int ta = blockIdx.x / tilesC, tb = blockIdx.x - ta * tilesC;
  const int q = blockIdx.y / R, r = blockIdx.y - q * R, g = blockIdx.z;
  const int first = q == 0 ? 0 : 2, lq = l_tr - first;
  if (ta * kTile >= lq || tb * kTile > lq) return;
  if (tb > ta && lq / kTile != tb) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4, wa = w >> 1, wb = w & 1;
  const double *tab = q == 0 ? P : P2;
  const double *d = D + ((size_t)(g * 3 + q) * (2 * R + kNodeRows) + 2 * r) * n_mu, *d1 = d + n_mu;
  // staging: node k of the step on the low four bits of the thread, so that a wavefront reads runs of 16 nodes of four rows
  const int sk = threadIdx.x & 15, sr = threadIdx.x >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) acc[p][s] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n_mu; k0 += kKStep) {
    const int i = k0 + sk;
    const double di = i < n_mu ? d[i] : 0.0, d1i = i < n_mu ? d1[i] : 0.0;
#pragma unroll
    for (int p = 0; p < kTile / 16; ++p) {
      const int row = sr + 16 * p, a = ta * kTile + row, b = tb * kTile + row;
      double x = 0.0, y = 0.0;
      if (i < n_mu) {
        if (a < lq) {
          x = tab[(size_t)(first + a) * n_mu + i];
          if (q) x = fac[first + a] * x;
        }
        if (b < lq) {
          y = tab[(size_t)(first + b) * n_mu + i];
          if (q) y = fac[first + b] * y;
          y = di * y;
        } else if (b == lq) {
          y = d1i;
        }
      }
      Xs[sk][row] = x;
      Ys[sk][row] = y;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kKStep / 4; ++s) {
      const int kr = 4 * s + lk;
      const double xa[2] = {Xs[kr][wa * 32 + lr], Xs[kr][wa * 32 + 16 + lr]};
      const double yb[2] = {Ys[kr][wb * 32 + lr], Ys[kr][wb * 32 + 16 + lr]};
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[p][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[p], yb[t], acc[p][t], 0, 0, 0);
    }
    __syncthreads();
  }
  const int pitch = l_tr + 1;
  double *out = Gm + ((size_t)(g * 3 + q) * R + r) * l_tr * pitch;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int a = ta * kTile + wa * 32 + p * 16 + lk + 4 * v, b = tb * kTile + wb * 32 + t * 16 + lr;
        if (a < lq && b <= lq) out[(size_t)a * pitch + b] = acc[p][t][v];
      }
}

// ---- (s) Cholesky, the solves, the quotient rules ---------------------------------------------------------------------------
// L y = x, L^T x = y for nr <= kRhs right-hand sides X[r][0 .. n - 1]; L below the diagonal of A, its diagonal in dg
__device__ __forceinline__ void chol_solve(int n, int nr, const double *A, const double *dg, double *X) {
  const int i = threadIdx.x & (kMax - 1), r0 = threadIdx.x >> 7;  // two right-hand sides at a time
  for (int j = 0; j < n; ++j) {
    if (i == j)
      for (int r = r0; r < nr; r += 2) X[r * kMax + j] /= dg[j];
    __syncthreads();
    if (i > j && i < n)
      for (int r = r0; r < nr; r += 2) X[r * kMax + i] -= A[i * kLdA + j] * X[r * kMax + j];
    __syncthreads();
  }
  for (int j = n - 1; j >= 0; --j) {
    if (i == j)
      for (int r = r0; r < nr; r += 2) X[r * kMax + j] /= dg[j];
    __syncthreads();
    if (i < j)
      for (int r = r0; r < nr; r += 2) X[r * kMax + i] -= A[j * kLdA + i] * X[r * kMax + j];
    __syncthreads();
  }
}

// B[i][a] of a fit: the entry the Gram product stages (fac P2 rounded once)
__device__ __forceinline__ double basis(const double *tab, const double *fac, int q, int first, int n_mu, int a, int i) {
  const double x = tab[(size_t)(first + a) * n_mu + i];
  return q ? fac[first + a] * x : x;
}

// One correction of nr solutions Y[r] (LDS) from their residuals at the nodes: node rows S[r][i] = hi[r][i] - d0[i] (B Y[r])[i]
// (global scratch), X[r] = B^T S[r], X[r] = A^-1 X[r], Y[r] += X[r].  hi: the part of the residual that does not depend on Y[r],
// row r at hi + r hi_stride.  All sums run in index order.
__device__ __forceinline__ void correct(int q, int first, int n, int nr, int n_mu, const double *tab, const double *fac, const double *d0,
                                        const double *hi, size_t hi_stride, const double *ur, double *S, const double *A,
                                        const double *dg, double *X, double *Y) {
  for (int e = threadIdx.x; e < nr * n_mu; e += kThreads) {
    const int r = e / n_mu, i = e - r * n_mu;
    double v = 0.0;
    for (int a = 0; a < n; ++a) v += basis(tab, fac, q, first, n_mu, a, i) * Y[r * kMax + a];
    const double h = hi[r * hi_stride + i];
    S[(size_t)r * n_mu + i] = (ur ? -h * (2.0 * ur[i] - 1.0) : h) - d0[i] * v;
  }
  __syncthreads();
  {
    const int a = threadIdx.x & (kMax - 1);
    for (int r = threadIdx.x >> 7; r < nr; r += 2) {
      if (a >= n) continue;
      double v = 0.0;
      for (int i = 0; i < n_mu; ++i) v += basis(tab, fac, q, first, n_mu, a, i) * S[(size_t)r * n_mu + i];
      X[r * kMax + a] = v;
    }
  }
  __syncthreads();
  chol_solve(n, nr, A, dg, X);
  for (int e = threadIdx.x; e < nr * n; e += kThreads) {
    const int r = e / n, a = e - r * n;
    Y[r * kMax + a] += X[r * kMax + a];
  }
  __syncthreads();
}

// grid (fits, sets).  greek_t [l_tr, 6, R, nG], c0 [R, nG].  Fit 0 writes alpha, beta, delta, zeta and c0, fit 1 gamma, fit 2 epsilon.
// D: the rows of k_trunc_weights; rows 2 R + 1 .. of a (set, fit) are this workgroup's scratch at the nodes
__global__ void __launch_bounds__(kThreads) k_trunc_solve(int n_mu, int l_full, int l_tr, int R, const double *__restrict__ greek,
                                                          const double *__restrict__ P, const double *__restrict__ P2,
                                                          const double *__restrict__ fac, double *D, const double *__restrict__ Gm,
                                                          double *__restrict__ greek_t, double *__restrict__ c0_out,
                                                          int *__restrict__ status) {
#pragma clang fp contract(off)  // the quotient rules are the host's statements, operation by operation
  __shared__ double A[kMax * kLdA];
  __shared__ double X[kRhs * kMax];
  __shared__ double Y[kRhs * kMax];
  __shared__ double cs[kMax];
  __shared__ double dg[kMax];
  const int q = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int first = q == 0 ? 0 : 2, n = l_tr - first, pitch = l_tr + 1;
  double *out = greek_t + (size_t)l_tr * 6 * R * g;
  if (n <= 0) {  // l_tr <= 2: gamma^t and epsilon^t are exact zeros
    for (int e = tid; e < R * l_tr; e += kThreads) out[(size_t)l_tr * (fit_row(q) + 6 * (e / l_tr)) + e % l_tr] = 0.0;
    return;
  }
  const double *tab = q == 0 ? P : P2;
  double *Dq = D + ((size_t)(g * 3 + q) * (2 * R + kNodeRows)) * n_mu;
  const double *d0 = Dq, *d0p = Dq + n_mu, *finv = Dq + (size_t)(2 * R) * n_mu;
  double *ur = Dq + (size_t)(2 * R + 1) * n_mu, *S = Dq + (size_t)(2 * R + 2) * n_mu;
  const double *G0 = Gm + ((size_t)(g * 3 + q) * R) * l_tr * pitch;
  for (int e = tid; e < n * n; e += kThreads) {
    const int a = e / n, b = e - a * n;
    if (b <= a) A[a * kLdA + b] = G0[(size_t)a * pitch + b];
  }
  if (tid < n) X[tid] = G0[(size_t)tid * pitch + n];
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    double piv = A[j * kLdA + j];
    if (!(piv > 0.0) || !isfinite(piv)) {
      bad = true;
      piv = 1.0;
    }
    const double s = sqrt(piv);
    if (tid == 0) dg[j] = s;
    for (int i = j + 1 + tid; i < n; i += kThreads) A[i * kLdA + j] /= s;
    __syncthreads();
    const int m = n - j - 1;
    for (int e = tid; e < m * m; e += kThreads) {
      const int i = j + 1 + e / m, k = j + 1 + e % m;
      if (k <= i) A[i * kLdA + k] -= A[i * kLdA + j] * A[k * kLdA + j];
    }
    __syncthreads();
  }
  chol_solve(n, 1, A, dg, X);
  if (tid < n) cs[tid] = X[tid];
  __syncthreads();
  // (w / f) (1 - B c / f) = d0' - d0 (B c)
  correct(q, first, n, 1, n_mu, tab, fac, d0, d0p, 0, nullptr, S, A, dg, X, cs);
  for (int i = tid; i < n_mu; i += kThreads) {  // B c / f of the corrected solution, for the partials' residuals
    double v = 0.0;
    for (int a = 0; a < n; ++a) v += basis(tab, fac, q, first, n_mu, a, i) * cs[a];
    ur[i] = v * finv[i];
  }
  const double c0 = cs[0];
  if (q == 0 && (c0 == 0.0 || !isfinite(c0))) bad = true;
  if (bad && tid == 0) atomicOr(status + g, 1 << q);
  const double *gv = greek + (size_t)l_full * 6 * R * g;
  // the value rows
  for (int l = tid; l < l_tr; l += kThreads) {
    if (q == 0) {
      const double cl = cs[l], sh = gv[(size_t)l_full + l] - cl;
      out[l] = (gv[l] - sh) / c0;
      out[(size_t)l_tr + l] = cl / c0;
      out[(size_t)3 * l_tr + l] = (gv[(size_t)3 * l_full + l] - sh) / c0;
      out[(size_t)5 * l_tr + l] = (gv[(size_t)5 * l_full + l] - sh) / c0;
    } else {
      out[(size_t)fit_row(q) * l_tr + l] = l < 2 ? 0.0 : cs[l - 2];
    }
  }
  if (q == 0 && tid == 0) c0_out[(size_t)R * g] = c0;
  // the partials, kRhs at a time: rhs = db - dA c (dA symmetric, its lower triangle of tiles computed), then the same factor
  for (int rb = 1; rb < R; rb += kRhs) {
    const int nr = min(kRhs, R - rb);
    __syncthreads();
    {
      const int a = tid & (kMax - 1);
      for (int r = tid >> 7; r < nr; r += 2) {
        if (a >= n) continue;
        const double *Gr = G0 + (size_t)(rb + r) * l_tr * pitch;
        double s = Gr[(size_t)a * pitch + n];
        for (int b = 0; b <= a; ++b) s -= Gr[(size_t)a * pitch + b] * cs[b];
        for (int b = a + 1; b < n; ++b) s -= Gr[(size_t)b * pitch + a] * cs[b];
        X[r * kMax + a] = s;
      }
    }
    __syncthreads();
    chol_solve(n, nr, A, dg, X);
    for (int e = tid; e < nr * n; e += kThreads) Y[(e / n) * kMax + e % n] = X[(e / n) * kMax + e % n];
    __syncthreads();
    // (w / f) ((df / f) (2 B c / f - 1) - B dc / f) = -d_r' (2 B c / f - 1) - d0 (B dc)
    correct(q, first, n, nr, n_mu, tab, fac, d0, Dq + (size_t)(2 * rb + 1) * n_mu, (size_t)2 * n_mu, ur, S, A, dg, X, Y);
    for (int e = tid; e < nr * l_tr; e += kThreads) {
      const int r = e / l_tr, l = e - r * l_tr;
      const double *gd = gv + (size_t)l_full * 6 * (rb + r);
      double *od = out + (size_t)l_tr * 6 * (rb + r);
      if (q == 0) {
        const double dc0 = Y[r * kMax], dc = Y[r * kMax + l], cl = cs[l], sh = gv[(size_t)l_full + l] - cl;
        const double dsh = gd[(size_t)l_full + l] - dc, cc = c0 * c0;
        od[l] = (gd[l] - dsh) / c0 - (gv[l] - sh) * dc0 / cc;
        od[(size_t)l_tr + l] = dc / c0 - cl * dc0 / cc;
        od[(size_t)3 * l_tr + l] = (gd[(size_t)3 * l_full + l] - dsh) / c0 - (gv[(size_t)3 * l_full + l] - sh) * dc0 / cc;
        od[(size_t)5 * l_tr + l] = (gd[(size_t)5 * l_full + l] - dsh) / c0 - (gv[(size_t)5 * l_full + l] - sh) * dc0 / cc;
        if (l == 0) c0_out[(size_t)R * g + rb + r] = dc0;
      } else {
        od[(size_t)fit_row(q) * l_tr + l] = l < 2 ? 0.0 : Y[r * kMax + l - 2];
      }
    }
  }
}

// ---- (m) a set with a status word becomes NaN -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_trunc_mark(int l_tr, int R, const int *__restrict__ status, double *__restrict__ greek_t,
                                                         double *__restrict__ c0) {
  const int g = blockIdx.x;
  if (status[g] == 0) return;
  const double nan = __builtin_nan("");
  double *o = greek_t + (size_t)l_tr * 6 * R * g;
  for (int e = threadIdx.x; e < l_tr * 6 * R; e += kThreads) o[e] = nan;
  for (int e = threadIdx.x; e < R; e += kThreads) c0[(size_t)R * g + e] = nan;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int trunc_fail(const char *fn, int rc, const char *what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  mom_set_global_error(buf);
  return rc;
}

#define TCHK(call)                                                                                     \
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

}  // namespace

const char *mom_trunc_check(int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr, const double *greek) {
  if (n_mu < 1) return "n_mu must be at least 1";
  if (nG < 1) return "nG must be at least 1";
  if (nP < 0) return "nP must not be negative";
  if (l_full < 1) return "l_full must be at least 1";
  if (l_tr < 1) return "l_tr must be at least 1";
  if (l_tr > l_full) return "l_tr must not exceed l_full";
  if (!mu || !w_mu || !greek) return "null pointer";
  if (nG > 65535 || nP > 16383 || (long long)n_mu * l_full > 0x7fffffffLL) return "size out of range (nG <= 65535, nP <= 16383)";
  for (int i = 0; i < n_mu; ++i) {
    if (!(mu[i] >= -1.0 && mu[i] <= 1.0)) return "every mu has to be in [-1, 1]";
    if (!std::isfinite(w_mu[i])) return "w_mu is not finite";
  }
  const size_t nGreek = (size_t)l_full * 6 * (1 + nP) * nG;
  for (size_t e = 0; e < nGreek; ++e)
    if (!std::isfinite(greek[e])) return "a Greek coefficient is not finite";
  return nullptr;
}

#define PCHK(call)                          \
  do {                                      \
    const hipError_t e__ = (call);          \
    if (e__ != hipSuccess) return e__;      \
  } while (0)

hipError_t mom_trunc_plan(MomTruncPlan &pl, int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr,
                          const double *greek, hipStream_t st) {
  const int R = 1 + nP;
  pl.n_mu = n_mu; pl.nG = nG; pl.nP = nP; pl.l_full = l_full; pl.l_tr = l_tr;
  const size_t perSet = (size_t)3 * R * l_tr * (l_tr + 1);  // doubles of a set's Gram products
  pl.chunk = (int)std::min<size_t>((size_t)nG, std::max<size_t>(1, kGramWorkspace / sizeof(double) / perSet));
  pl.coef = mom_legendre_table_coef(l_full);
  pl.fac.assign((size_t)l_full, 0.0);
  for (int l = 2; l < l_full; ++l) pl.fac[l] = std::sqrt(1.0 / (((double)l - 1.0) * (double)l * ((double)l + 1.0) * ((double)l + 2.0)));
  PCHK(mom_upload(pl.d_mu, mu, (size_t)n_mu, st));
  PCHK(mom_upload(pl.d_w, w_mu, (size_t)n_mu, st));
  PCHK(mom_upload(pl.d_coef, pl.coef.data(), pl.coef.size(), st));
  PCHK(mom_upload(pl.d_fac, pl.fac.data(), pl.fac.size(), st));
  PCHK(mom_upload(pl.d_greek, greek, (size_t)l_full * 6 * R * nG, st));
  PCHK(pl.d_tab.renew(2 * (size_t)n_mu + 4 * (size_t)l_full * n_mu));
  PCHK(pl.d_D.renew((size_t)nG * 3 * (2 * R + kNodeRows) * n_mu));
  return pl.d_G.renew(perSet * pl.chunk);
}

hipError_t mom_trunc_launch(const MomTruncPlan &pl, hipStream_t st, double *greek_t, double *c0, int *status) {
  const int n_mu = pl.n_mu, l_full = pl.l_full, l_tr = pl.l_tr, R = 1 + pl.nP, fits = l_tr > 2 ? 3 : 1;
  if (l_tr < 1 || l_tr > kMomTruncMax || l_tr > l_full) return hipErrorInvalidValue;
  const size_t nLeg = (size_t)l_full * n_mu;
  double *pitau = pl.d_tab.get(), *leg0 = pitau + 2 * (size_t)n_mu;
  double *const leg[4] = {leg0, leg0 + nLeg, leg0 + 2 * nLeg, leg0 + 3 * nLeg};
  PCHK(hipMemsetAsync(status, 0, (size_t)pl.nG * sizeof(int), st));
  PCHK(mom_legendre_tables_launch(st, n_mu, l_full, pl.d_mu.get(), pl.d_coef.get(), pitau, leg));
  hipLaunchKernelGGL(k_trunc_weights, dim3((unsigned)((n_mu + 63) / 64), (unsigned)fits, (unsigned)pl.nG), dim3(64), 0, st, n_mu, l_full,
                     R, pl.d_w.get(), pl.d_greek.get(), leg[0], leg[1], pl.d_fac.get(), pl.d_D.get(), status);
  PCHK(hipGetLastError());
  const int tilesR = (l_tr + kTile - 1) / kTile, tilesC = (l_tr + kTile) / kTile;  // columns 0 .. l_tr
  for (int g0 = 0; g0 < pl.nG; g0 += pl.chunk) {
    const int ng = std::min(pl.chunk, pl.nG - g0);
    double *D = pl.d_D.get() + (size_t)g0 * 3 * (2 * R + kNodeRows) * n_mu;
    hipLaunchKernelGGL(k_trunc_gram, dim3((unsigned)(tilesR * tilesC), (unsigned)(fits * R), (unsigned)ng), dim3(kThreads), 0, st, n_mu,
                       l_tr, R, tilesC, leg[0], leg[1], pl.d_fac.get(), D, pl.d_G.get());
    PCHK(hipGetLastError());
    hipLaunchKernelGGL(k_trunc_solve, dim3(3, (unsigned)ng), dim3(kThreads), 0, st, n_mu, l_full, l_tr, R,
                       pl.d_greek.get() + (size_t)g0 * l_full * 6 * R, leg[0], leg[1], pl.d_fac.get(), D, pl.d_G.get(), greek_t + (size_t)g0 * l_tr * 6 * R,
                       c0 + (size_t)g0 * R, status + g0);
    PCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_trunc_mark, dim3((unsigned)pl.nG), dim3(kThreads), 0, st, l_tr, R, status, greek_t, c0);
  return hipGetLastError();
}

extern "C" int mom_truncate_phase(int device, int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr,
                                  const double *greek, double *greek_t, double *c0, int *status, double *gpu_ms) {
  const char *fn = "mom_truncate_phase";
  if (const char *bad = mom_trunc_check(n_mu, mu, w_mu, nG, nP, l_full, l_tr, greek)) return trunc_fail(fn, MOM_EINVAL, bad);
  if (!greek_t || !c0 || !status) return trunc_fail(fn, MOM_EINVAL, "null pointer");
  if (l_tr > kMomTruncMax) return trunc_fail(fn, MOM_EUNSUPPORTED, "l_tr above 128 is not built");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return trunc_fail(fn, MOM_EHIP, "no HIP device available");
  if (device < 0 || device >= ndev) return trunc_fail(fn, MOM_EINVAL, "device index out of range");

  int rc = MOM_OK;
  const int R = 1 + nP;
  const size_t nOut = (size_t)l_tr * 6 * R * nG, nC0 = (size_t)R * nG;
  MomTruncPlan pl;
  MomDevBuf<double> d_out;
  MomDevBuf<int> d_status;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  TCHK(hipSetDevice(device));
  TCHK(hipStreamCreate(&st));
  TCHK(hipEventCreate(&ev[0]));
  TCHK(hipEventCreate(&ev[1]));
  TCHK(mom_trunc_plan(pl, n_mu, mu, w_mu, nG, nP, l_full, l_tr, greek, st));
  TCHK(d_out.renew(nOut + nC0));
  TCHK(d_status.renew((size_t)nG));
  TCHK(hipEventRecord(ev[0], st));
  TCHK(mom_trunc_launch(pl, st, d_out.get(), d_out.get() + nOut, d_status.get()));
  TCHK(hipEventRecord(ev[1], st));
  TCHK(hipMemcpyAsync(greek_t, d_out.get(), nOut * sizeof(double), hipMemcpyDeviceToHost, st));
  TCHK(hipMemcpyAsync(c0, d_out.get() + nOut, nC0 * sizeof(double), hipMemcpyDeviceToHost, st));
  TCHK(hipMemcpyAsync(status, d_status.get(), (size_t)nG * sizeof(int), hipMemcpyDeviceToHost, st));
  TCHK(hipStreamSynchronize(st));
  if (gpu_ms) {
    float t = 0.f;
    TCHK(hipEventElapsedTime(&t, ev[0], ev[1]));
    *gpu_ms = t;
  }
  for (int g = 0; g < nG && rc == MOM_OK; ++g)
    if (status[g]) {
      int q = 0;
      while (!((status[g] >> q) & 1)) ++q;
      char buf[160];
      snprintf(buf, sizeof buf, "set %d, fit %d: a divisor or a pivot of the fit is zero or not finite (the set's rows are NaN)", g, q);
      rc = trunc_fail(fn, MOM_ESINGULAR, buf);
    }
done:
  if (st) (void)hipStreamSynchronize(st);  // the buffers and the plan's host vectors end with this call
  for (int q = 0; q < 2; ++q)
    if (ev[q]) (void)hipEventDestroy(ev[q]);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}
