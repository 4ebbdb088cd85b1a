// mom_mie.hip -- Mie aerosol optics by the Siewert NAI-2 method on gfx950 (Float64).
//
// Restates compute_aerosol_optical_properties(::MieModel{NAI2}) (src/Scattering/compute_NAI2.jl:16-182) with
// compute_mie_ab!, compute_mie_S1S2! and get_n_max (mie_helper_functions.jl:17-71, 154-167).  The reference loops over the
// radii of the size distribution on the host; here the call is four launches:
//   (a) k_mie_ab     one radius per lane: downward recurrence of the logarithmic derivative D_n(m x), upward recurrence of
//                    psi, chi, xi and a_n, b_n; writes c_n a_n, c_n b_n (c_n = (2n+1) / (n (n+1))) as four real planes
//                    [Kp, nRp], radius fastest, exact zeros above the radius' own n_max
//   (b) k_mie_amp    S1 = sum_l (c a)_l tau_l + (c b)_l pi_l, S2 = sum_l (c a)_l pi_l + (c b)_l tau_l as a real GEMM on
//                    v_mfma_f64_16x16x4 ([tau | pi] times the four planes), with the epilogue in registers: f11, f33, f12,
//                    f34 of the tile, times each weight row, summed over the tile's radii.  No [n_mu, nR] array exists.
//   (c) k_mie_sum    the per-chunk partials of (b) added in chunk order (no floating-point atomics: two runs are bitwise equal)
//   (d) k_mie_greek  the projections of the bulk elements onto P, P2, R2, T2 (compute_NAI2.jl:146-160), one wavefront per l
// The radii arrive ascending, so n_max is monotone over them and a radius tile's K loop ends at the tile's largest n_max
// (rounded up to the k-step of 4): what is left out are products with the exact zeros of (a).
//
// The Dual run (mom_mie_nai2_dual) adds the partials with respect to the refractive index m = n_r + i n_i.  a_n and b_n are
// holomorphic in m, so ONE complex derivative a' = da/dm carries both: d/dn_r = a', d/dn_i = i a'.  k_mie_ab<., true> carries
// D' = dD/dm through the downward recurrence and writes c a', c b' as four more planes; k_mie_amp<NW, true> forms S1', S2' with
// the same A operands and accumulates two more bulk rows, weight row 0 times df/dn_r and df/dn_i; (c) and (d) are linear and
// run unchanged on NW + 2 rows.  n_max and the start of the downward recurrence are integers and are not differentiated.
//
// A batch of wavelengths (mom_mie_nai2_spectral) is one more grid dimension of the same four kernels: radii, weight rows, the angle
// grid and its tables are shared, and what differs per wavelength -- m, x, sin x, cos x, n_max, the planes, the sums -- is found
// through a small device array (MieWave) indexed by that dimension.  The single-wavelength calls are the batch of one.  For a batch
// the tables of (b) and (d) are built on the device from the Gauss nodes (k_mie_tables) instead of uploaded.
//
// The PCW route (mom_pcw.hip) starts from the same a_n, b_n: it launches (a) through mom_mie_ab.hpp (at the end of this file).
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

constexpr int kTileR = 16;    // radii per tile of (b): the N extent of the MFMA
constexpr int kMuBlock = 32;  // mu rows per wavefront of (b): two M tiles share every B operand
constexpr int kKStep = 4;     // K extent of the MFMA
constexpr int kMaxChunks = 128;  // radius chunks of (b): beyond 2048 radii a wavefront takes several tiles

// ---- (a) Mie coefficients ------------------------------------------------------------------------------------------------
// SCALE: write c_n a_n, c_n b_n (the planes (b) reads); otherwise a_n, b_n themselves (mom_mie_coefficients).
// Complex arithmetic is written out on the real and imaginary parts, a quotient u / v as u conj(v) / |v|^2, and the compiler
// may not contract a product and a sum into an FMA here: the upward psi recurrence is only conditionally stable, so the
// order and the rounding of every operation are part of the result (tests/mie_oracle.py performs the same operations).
// DUAL: also D' = dD/dm (two more [n_max, ld] planes), c a', c b' (four more planes) and the d/dn_r, d/dn_i forms of the two
// cross-section sums (dsum [4, ld]: sca, ext for n_r, then for n_i).  The value statements are the same in both forms.
// sin x and cos x, the start values psi_0, psi_1 of the upward recurrence, come from the host (mie_sin_cos): psi_1 = sin x / x - cos x
// cancels to x^2 / 3 and the recurrence above x magnifies what is left of a last-bit error further, so they have to be as good
// as Float64 allows; the device's sin and cos miss the correctly rounded value in a good third of the arguments.
struct MieDualOut {
  double *Dre, *Dim, *aR, *aI, *bR, *bI, *sum;
};

// One wavelength of a batch: the refractive index and where the wavelength's arrays start, in elements from the bases the kernels
// are given: oR the per-radius arrays (x, sin x, cos x, n_max, nmx), oS the per-radius sums, oD the D planes, oPl the coefficient planes.
struct MieWave {
  double mr, mi;
  long long oR, oS, oD, oPl;
};

template <bool SCALE, bool DUAL>
__global__ void __launch_bounds__(64) k_mie_ab(int nR, int ld, const MieWave *__restrict__ waves, const double *__restrict__ x,
                                               const double *__restrict__ sinx, const double *__restrict__ cosx,
                                               const int *__restrict__ nmax, const int *__restrict__ nmx, double *__restrict__ Dre,
                                               double *__restrict__ Dim, double *__restrict__ aR, double *__restrict__ aI,
                                               double *__restrict__ bR, double *__restrict__ bI, double *__restrict__ ssca,
                                               double *__restrict__ sext, MieDualOut dd) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nR) return;
  const MieWave wv = waves[blockIdx.y];  // this block's wavelength
  const double mr = wv.mr, mi = wv.mi;
  x += wv.oR, sinx += wv.oR, cosx += wv.oR, nmax += wv.oR, nmx += wv.oR;
  Dre += wv.oD, Dim += wv.oD;
  aR += wv.oPl, aI += wv.oPl, bR += wv.oPl, bI += wv.oPl;
  if (ssca) ssca += wv.oS;
  if (sext) sext += wv.oS;
  if constexpr (DUAL) {
    dd.Dre += wv.oD, dd.Dim += wv.oD;
    dd.aR += wv.oPl, dd.aI += wv.oPl, dd.bR += wv.oPl, dd.bI += wv.oPl;
    if (dd.sum) dd.sum += wv.oS;
  }
  const double xi = x[i];
  const int nm = nmax[i], ntop = nmx[i];
  // 1 / m and 1 / m^2 (Dual run)
  const double mm = mr * mr + mi * mi, imr = mr / mm, imi = -mi / mm;
  [[maybe_unused]] const double i2r = imr * imr - imi * imi, i2i = 2.0 * (imr * imi);
  [[maybe_unused]] double ddr = 0.0, ddi = 0.0;  // D'_ntop = 0
  // y = x m; (n + 1) / y = (n + 1) * (conj(y) / |y|^2)
  const double yr = xi * mr, yi = xi * mi, y2 = yr * yr + yi * yi;
  const double iyr = yr / y2, iyi = -yi / y2;
  double dr = 0.0, di = 0.0;  // D_ntop = 0
  for (int n = ntop - 1; n >= 1; --n) {
    const double c = (double)(n + 1), qr = c * iyr, qi = c * iyi;
    const double sr = dr + qr, si = di + qi, s2 = sr * sr + si * si;
    dr = qr - sr / s2;  // D_n = (n+1)/y - 1 / (D_{n+1} + (n+1)/y)
    di = qi + si / s2;
    if (n <= nm) {
      Dre[(size_t)(n - 1) * ld + i] = dr;
      Dim[(size_t)(n - 1) * ld + i] = di;
    }
    if constexpr (DUAL) {
      // q = (n+1)/y, q' = -q / m;  D'_n = q' + (D'_{n+1} + q') / (D_{n+1} + q)^2
      const double pr = -(qr * imr - qi * imi), pi_ = -(qr * imi + qi * imr);
      const double ur = sr / s2, ui = -si / s2, vr = ur * ur - ui * ui, vi = 2.0 * (ur * ui);
      const double gr = ddr + pr, gi = ddi + pi_;
      ddr = pr + (gr * vr - gi * vi);
      ddi = pi_ + (gr * vi + gi * vr);
      if (n <= nm) {
        dd.Dre[(size_t)(n - 1) * ld + i] = ddr;
        dd.Dim[(size_t)(n - 1) * ld + i] = ddi;
      }
    }
  }
  const double m2 = mr * mr + mi * mi;
  double psi0 = cosx[i], psi1 = sinx[i], chi0 = -psi1, chi1 = psi0;
  double sca = 0.0, ext = 0.0;
  [[maybe_unused]] double dsca_r = 0.0, dext_r = 0.0, dsca_i = 0.0, dext_i = 0.0;
  for (int n = 1; n <= nm; ++n) {
    const double tn = (double)(2 * n - 1);
    const double psi = tn * psi1 / xi - psi0, chi = tn * chi1 / xi - chi0;  // xi_n = psi - i chi
    const double er = Dre[(size_t)(n - 1) * ld + i], ei = Dim[(size_t)(n - 1) * ld + i];
    const double nx = (double)n / xi;
    // t_a = D / m + n / x, t_b = D m + n / x
    const double tar = (er * mr + ei * mi) / m2 + nx, tai = (ei * mr - er * mi) / m2;
    const double tbr = (er * mr - ei * mi) + nx, tbi = er * mi + ei * mr;
    // (t psi - psi_1) / (t xi - xi_1)
    const double anr = tar * psi - psi1, ani = tai * psi;
    const double adr = (tar * psi + tai * chi) - psi1, adi = (tai * psi - tar * chi) + chi1, ad2 = adr * adr + adi * adi;
    const double ar = (anr * adr + ani * adi) / ad2, ai = (ani * adr - anr * adi) / ad2;
    const double bnr = tbr * psi - psi1, bni = tbi * psi;
    const double bdr = (tbr * psi + tbi * chi) - psi1, bdi = (tbi * psi - tbr * chi) + chi1, bd2 = bdr * bdr + bdi * bdi;
    const double br = (bnr * bdr + bni * bdi) / bd2, bi = (bni * bdr - bnr * bdi) / bd2;
    const double w2 = (double)(2 * n + 1);
    sca = sca + w2 * ((ar * ar + ai * ai) + (br * br + bi * bi));
    ext = ext + w2 * (ar + br);
    const double c = SCALE ? w2 / ((double)n * (double)(n + 1)) : 1.0;
    const size_t o = (size_t)(n - 1) * ld + i;
    aR[o] = c * ar;
    aI[o] = c * ai;
    bR[o] = c * br;
    bI[o] = c * bi;
    if constexpr (DUAL) {
      const double fr = dd.Dre[o], fi = dd.Dim[o];
      // t_a' = D' / m - D / m^2, t_b' = D' m + D
      const double tapr = (fr * imr - fi * imi) - (er * i2r - ei * i2i), tapi = (fr * imi + fi * imr) - (er * i2i + ei * i2r);
      const double tbpr = (fr * mr - fi * mi) + er, tbpi = (fr * mi + fi * mr) + ei;
      // a' = t' (xi_n psi_{n-1} - psi_n xi_{n-1}) / (t xi_n - xi_{n-1})^2; the bracket is i (psi_n chi_{n-1} - chi_n psi_{n-1})
      const double wi = psi * chi1 - chi * psi1;
      const double uar = adr / ad2, uai = -adi / ad2, var = uar * uar - uai * uai, vai = 2.0 * (uar * uai);
      const double par = tapr * var - tapi * vai, pai = tapr * vai + tapi * var;
      const double dar = -(wi * pai), dai = wi * par;
      const double ubr = bdr / bd2, ubi = -bdi / bd2, vbr = ubr * ubr - ubi * ubi, vbi = 2.0 * (ubr * ubi);
      const double pbr = tbpr * vbr - tbpi * vbi, pbi = tbpr * vbi + tbpi * vbr;
      const double dbr = -(wi * pbi), dbi = wi * pbr;
      // d/dn_r: e = a'; d/dn_i: e = i a'.  d|a|^2 = 2 Re(conj(a) e), d Re(a) = Re(e)
      dsca_r = dsca_r + w2 * (2.0 * ((ar * dar + ai * dai) + (br * dbr + bi * dbi)));
      dext_r = dext_r + w2 * (dar + dbr);
      dsca_i = dsca_i - w2 * (2.0 * ((ar * dai - ai * dar) + (br * dbi - bi * dbr)));
      dext_i = dext_i - w2 * (dai + dbi);
      dd.aR[o] = c * dar;
      dd.aI[o] = c * dai;
      dd.bR[o] = c * dbr;
      dd.bI[o] = c * dbi;
    }
    psi0 = psi1;
    psi1 = psi;
    chi0 = chi1;
    chi1 = chi;
  }
  if (ssca) ssca[i] = sca;
  if (sext) sext[i] = ext;
  if constexpr (DUAL)
    if (dd.sum) {
      dd.sum[i] = dsca_r;
      dd.sum[(size_t)ld + i] = dext_r;
      dd.sum[(size_t)2 * ld + i] = dsca_i;
      dd.sum[(size_t)3 * ld + i] = dext_i;
    }
}

// ---- (b) amplitude GEMM with the phase-matrix epilogue -------------------------------------------------------------------
// One wavefront per block: MT M tiles of 16 mu rows (blockIdx.x) times the radius tiles of chunk g = blockIdx.y (one tile of every G,
// in ascending order) of wavelength blockIdx.z.  The value form has MT = 2 (32 mu rows: two M tiles share every B operand); the Dual form has MT = 1 and twice
// the blocks in x, because its eight accumulators and NW + 2 bulk rows of two M tiles do not fit the 512 registers of a wavefront.
// Operand layouts of v_mfma_f64_16x16x4 as in mom_tile.hpp: A lane l = A[row l & 15][k l >> 4], B lane l = B[k l >> 4][col l & 15],
// C lane l register r = C[row (l >> 4) + 4 r][col l & 15].  tau, pi: [Kp, nMuP]; the planes: [Kp, nRp]; all zero padded, so
// the loads carry no masks.  partial: [nL, G, NWO, 4, nMuP] with NWO = NW (+ 2 in the Dual form: weight row 0 times df/dn_r, df/dn_i).
// Every element of S1, S2 and of the bulk rows 0 .. NW - 1 sees the same operations in the same order in both forms.
struct MieDualPlanes {
  const double *aR, *aI, *bR, *bI;  // c a', c b' (d/dm)
};

template <int NW, bool DUAL>
__global__ void __launch_bounds__(64) k_mie_amp(int nR, int nMuP, int nRp, int Kp, int nTiles, int G, const MieWave *__restrict__ waves,
                                                const double *__restrict__ tau, const double *__restrict__ pi,
                                                const double *__restrict__ caR, const double *__restrict__ caI,
                                                const double *__restrict__ cbR, const double *__restrict__ cbI,
                                                const double *__restrict__ x, const int *__restrict__ nmax,
                                                const double *__restrict__ w, int fullK, double *__restrict__ partial, MieDualPlanes dp) {
  constexpr int MT = DUAL ? 1 : 2, NWO = DUAL ? NW + 2 : NW, NS = DUAL ? 8 : 4;
  const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
  const int mu0 = 16 * MT * blockIdx.x, g = blockIdx.y;
  {
    const long long oR = waves[blockIdx.z].oR, oPl = waves[blockIdx.z].oPl;
    caR += oPl, caI += oPl, cbR += oPl, cbI += oPl;
    if constexpr (DUAL) dp.aR += oPl, dp.aI += oPl, dp.bR += oPl, dp.bI += oPl;
    x += oR, nmax += oR;
    partial += (size_t)blockIdx.z * G * NWO * 4 * nMuP;
  }
  d4 bulk[NWO][4][MT];
#pragma unroll
  for (int k = 0; k < NWO; ++k)
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int m = 0; m < MT; ++m) bulk[k][f][m] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j * G < nTiles; ++j) {
    const int t = j * G + ((j & 1) ? G - 1 - g : g);  // boustrophedon: n_max grows with t, so the chunks' K sums stay close
    if (t >= nTiles) continue;
    const int i0 = kTileR * t, ilast = min(i0 + kTileR - 1, nR - 1);
    const int kEnd = fullK ? Kp : min(Kp, (nmax[ilast] + kKStep - 1) / kKStep * kKStep);
    d4 s[NS][MT];  // S1 re, S1 im, S2 re, S2 im of the M tiles (Dual: then the same of S1', S2')
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int m = 0; m < MT; ++m) s[q][m] = (d4){0.0, 0.0, 0.0, 0.0};
    const double *pt = tau + (size_t)lq * nMuP + mu0 + lr, *pp = pi + (size_t)lq * nMuP + mu0 + lr;
    const size_t ob = (size_t)lq * nRp + i0 + lr;
    for (int k0 = 0; k0 < kEnd; k0 += kKStep) {
      const size_t oa = (size_t)k0 * nMuP, obk = ob + (size_t)k0 * nRp;
      double aT[MT], aP[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        aT[m] = pt[oa + 16 * m];
        aP[m] = pp[oa + 16 * m];
      }
      const double bAR = caR[obk], bAI = caI[obk], bBR = cbR[obk], bBI = cbI[obk];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        s[0][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], bAR, s[0][m], 0, 0, 0);
        s[1][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], bAI, s[1][m], 0, 0, 0);
        s[2][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], bAR, s[2][m], 0, 0, 0);
        s[3][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], bAI, s[3][m], 0, 0, 0);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        s[0][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], bBR, s[0][m], 0, 0, 0);
        s[1][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], bBI, s[1][m], 0, 0, 0);
        s[2][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], bBR, s[2][m], 0, 0, 0);
        s[3][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], bBI, s[3][m], 0, 0, 0);
      }
      if constexpr (DUAL) {
        const double dAR = dp.aR[obk], dAI = dp.aI[obk], dBR = dp.bR[obk], dBI = dp.bI[obk];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          s[4][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], dAR, s[4][m], 0, 0, 0);
          s[5][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], dAI, s[5][m], 0, 0, 0);
          s[6][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], dAR, s[6][m], 0, 0, 0);
          s[7][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], dAI, s[7][m], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          s[4][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], dBR, s[4][m], 0, 0, 0);
          s[5][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[m], dBI, s[5][m], 0, 0, 0);
          s[6][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], dBR, s[6][m], 0, 0, 0);
          s[7][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[m], dBI, s[7][m], 0, 0, 0);
        }
      }
    }
    // epilogue: this lane's column is radius i0 + lr (padding: x = 0, weights 0, S = 0)
    const double xi = x[i0 + lr], hx = xi > 0.0 ? 0.5 / (xi * xi) : 0.0;
    double wk[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) wk[k] = w[(size_t)k * nRp + i0 + lr];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s1r = s[0][m][r], s1i = s[1][m][r], s2r = s[2][m][r], s2i = s[3][m][r];
        const double n1 = s1r * s1r + s1i * s1i, n2 = s2r * s2r + s2i * s2i;
        const double f[4] = {hx * (n1 + n2),                            // f11 =  1/2x^2 (|S1|^2 + |S2|^2)
                             hx * (2.0 * (s1r * s2r + s1i * s2i)),      // f33 =  1/2x^2 Re(S1 S2* + S2 S1*)
                             -hx * (n1 - n2),                           // f12 = -1/2x^2 (|S1|^2 - |S2|^2)
                             -hx * (2.0 * (s1i * s2r - s1r * s2i))};    // f34 = -1/2x^2 Im(S1 S2* - S2 S1*)
#pragma unroll
        for (int k = 0; k < NW; ++k)
#pragma unroll
          for (int q = 0; q < 4; ++q) bulk[k][q][m][r] = fma(wk[k], f[q], bulk[k][q][m][r]);
        if constexpr (DUAL) {
          // e_j = S_j' for d/dn_r and i S_j' for d/dn_i:  df11 = 1/2x^2 2 (Re(S1* e1) + Re(S2* e2)), df12 = -1/2x^2 2 (Re(S1* e1) - Re(S2* e2)),
          // df33 = 1/2x^2 2 Re(e1 S2* + S1 e2*), df34 = -1/2x^2 2 Im(e1 S2* + S1 e2*)
          const double d1r = s[4][m][r], d1i = s[5][m][r], d2r = s[6][m][r], d2i = s[7][m][r];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const double e1r = c ? -d1i : d1r, e1i = c ? d1r : d1i, e2r = c ? -d2i : d2r, e2i = c ? d2r : d2i;
            const double p1 = s1r * e1r + s1i * e1i, p2 = s2r * e2r + s2i * e2i;
            const double zr = (e1r * s2r + e1i * s2i) + (s1r * e2r + s1i * e2i);
            const double zi = (e1i * s2r - e1r * s2i) + (s1i * e2r - s1r * e2i);
            const double df[4] = {hx * (2.0 * (p1 + p2)), hx * (2.0 * zr), -hx * (2.0 * (p1 - p2)), -hx * (2.0 * zi)};
#pragma unroll
            for (int q = 0; q < 4; ++q) bulk[NW + c][q][m][r] = fma(wk[0], df[q], bulk[NW + c][q][m][r]);
          }
        }
      }
  }
  // sum over the 16 radii of the tile columns (fixed butterfly), lane lr = 0 of every row writes
#pragma unroll
  for (int k = 0; k < NWO; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = bulk[k][q][m][r];
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
          if (lr == 0) partial[(((size_t)g * NWO + k) * 4 + q) * nMuP + mu0 + 16 * m + lq + 4 * r] = v;
        }
}

// ---- (c) partials of the G radius chunks, in chunk order; wavelength blockIdx.y --------------------------------------------
__global__ void k_mie_sum(int G, int rows, int n_mu, int nMuP, const double *__restrict__ partial, double *__restrict__ bulk) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;  // (row = k * 4 + q, mu)
  if (j >= rows * n_mu) return;
  partial += (size_t)blockIdx.y * G * rows * nMuP;
  bulk += (size_t)blockIdx.y * rows * n_mu;
  const int row = j / n_mu, mu = j - row * n_mu;
  double v = 0.0;
  for (int g = 0; g < G; ++g) v += partial[((size_t)g * rows + row) * nMuP + mu];
  bulk[j] = v;
}

// ---- (d) Greek coefficients (unnormalised) -------------------------------------------------------------------------------
// one wavefront per (l, weight row, wavelength); per wavelength bulk: [nW, 4, n_mu] in the order f11, f33, f12, f34; tables [l_max, n_mu], mu fastest;
// greek: [nW, 6, l_max] in the order alpha, beta, gamma, delta, epsilon, zeta
__global__ void __launch_bounds__(64) k_mie_greek(int n_mu, int l_max, const double *__restrict__ w_mu, const double *__restrict__ bulk,
                                                  const double *__restrict__ P, const double *__restrict__ P2,
                                                  const double *__restrict__ R2, const double *__restrict__ T2,
                                                  double *__restrict__ greek) {
  const int l = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  bulk += (size_t)blockIdx.z * gridDim.y * 4 * n_mu;
  greek += (size_t)blockIdx.z * gridDim.y * 6 * l_max;
  const double *f11 = bulk + (size_t)k * 4 * n_mu, *f33 = f11 + n_mu, *f12 = f33 + n_mu, *f34 = f12 + n_mu;
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = lane; j < n_mu; j += 64) {
    const size_t o = (size_t)l * n_mu + j;
    const double wm = w_mu[j], p = P[o], p2 = P2[o], r2 = R2[o], t2 = T2[o];
    a[0] += wm * (f11[j] * r2 + f33[j] * t2);
    a[1] += wm * (f11[j] * p);
    a[2] += wm * (f12[j] * p2);
    a[3] += wm * (f33[j] * p);
    a[4] += wm * (f34[j] * p2);
    a[5] += wm * (f33[j] * r2 + f11[j] * t2);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) a[q] += __shfl_xor(a[q], off);
  if (lane == 0) {
    const double dl = (double)l, pre = (2.0 * dl + 1.0) / 2.0;
    const double fac = l >= 2 ? pre * sqrt(1.0 / ((dl - 1.0) * dl * (dl + 1.0) * (dl + 2.0))) : 0.0;
    double *o = greek + (size_t)k * 6 * l_max + l;
    o[0] = fac * a[0];
    o[(size_t)l_max] = pre * a[1];
    o[(size_t)2 * l_max] = fac * a[2];
    o[(size_t)3 * l_max] = pre * a[3];
    o[(size_t)4 * l_max] = fac * a[4];
    o[(size_t)5 * l_max] = fac * a[5];
  }
}

// ---- (t) the angle tables of (b) and (d), from the Gauss nodes -----------------------------------------------------------
// One lane per mu, serial over the order: pi_n, tau_n (compute_mie_pi_tau, legendre_functions.jl:188-208) as rows n - 1 of
// [n_max, ldTab], and P, P2, R2, T2 (compute_legendre_poly, :217-259) as rows l of [l_max, n_mu]; mu fastest, so every store is
// coalesced and nothing is transposed.  The statements are those of scattering.compute_mie_pi_tau and compute_legendre_poly in
// their order, without contraction, so the tables are bitwise the host's.  coef [l_max, 4]: the per-degree scalars of the R2 / T2
// recurrence of row c (l = c - 1 >= 2): 2 l + 1, ib, ic, id, formed on the host as the host text forms them (sqrt, integer
// products); s15 = sqrt(1.5), s6 = sqrt(6).
__global__ void __launch_bounds__(64) k_mie_tables(int n_mu, int ldTab, int n_max, int l_max, const double *__restrict__ mu,
                                                   const double *__restrict__ coef, double s15, double s6, double *__restrict__ pi,
                                                   double *__restrict__ tau, double *__restrict__ P, double *__restrict__ P2,
                                                   double *__restrict__ R2, double *__restrict__ T2) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_mu) return;
  const double m = mu[j];
  {
    double p0 = 1.0, p1 = 3.0 * m;  // pi of the two orders before
    pi[j] = p0;
    tau[j] = m;
    if (n_max > 1) {
      pi[(size_t)ldTab + j] = p1;
      tau[(size_t)ldTab + j] = 6.0 * (m * m) - 3.0;
    }
    for (int n = 2; n < n_max; ++n) {
      const double pn = ((double)(2 * n + 1) * m * p1 - (double)(n + 1) * p0) / (double)n;
      pi[(size_t)n * ldTab + j] = pn;
      tau[(size_t)n * ldTab + j] = (double)(n + 1) * m * pn - (double)(n + 2) * p1;
      p0 = p1;
      p1 = pn;
    }
  }
  double a0 = 1.0, a1 = m;  // P of the two degrees before; then the same of P2, R2, T2
  double b0 = 0.0, b1 = 3.0 * (1.0 - m * m), r0 = 0.0, r1 = s15 * (1.0 + m * m), t0 = 0.0, t1 = s6 * m;
  for (int c = 0; c < l_max && c < 3; ++c) {
    const size_t o = (size_t)c * n_mu + j;
    P[o] = c == 0 ? 1.0 : (c == 1 ? m : ((double)3 * m * a1 - (double)1 * a0) / (double)2);
    P2[o] = c == 2 ? b1 : 0.0;
    R2[o] = c == 2 ? r1 : 0.0;
    T2[o] = c == 2 ? t1 : 0.0;
  }
  {
    const double a2 = ((double)3 * m * a1 - (double)1 * a0) / (double)2;
    a0 = a1;
    a1 = a2;
  }
  for (int c = 3; c < l_max; ++c) {
    const int l = c - 1;
    const size_t o = (size_t)c * n_mu + j;
    const double an = ((double)(2 * l + 1) * m * a1 - (double)l * a0) / (double)(l + 1);
    const double ia = coef[4 * c] * m, ib = coef[4 * c + 1], ic = coef[4 * c + 2], id = coef[4 * c + 3];
    const double bn = (ia * b1 - (double)(l + 2) * b0) / (double)(l - 1);
    const double rn = (ia * r1 - ib * r0 - ic * t1) / id;
    const double tn = (ia * t1 - ib * t0 - ic * r1) / id;
    P[o] = an;
    P2[o] = bn;
    R2[o] = rn;
    T2[o] = tn;
    a0 = a1, a1 = an;
    b0 = b1, b1 = bn;
    r0 = r1, r1 = rn;
    t0 = t1, t1 = tn;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int mie_fail(const char *fn, const char *what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  mom_set_global_error(buf);
  return MOM_EINVAL;
}

// a rejected argument of wavelength j of a batch (j < 0: of a single-wavelength call)
int mie_fail_at(const char *fn, int j, const char *what) {
  if (j < 0) return mie_fail(fn, what);
  char buf[256];
  snprintf(buf, sizeof buf, "wavelength %d: %s", j, what);
  return mie_fail(fn, buf);
}

// the per-degree scalars of k_mie_tables, [l_max, 4], in the words of scattering.compute_legendre_poly
std::vector<double> mie_table_coef(int l_max) {
  std::vector<double> c(4 * (size_t)l_max, 0.0);
  for (int row = 3; row < l_max; ++row) {
    const long long l = row - 1;
    c[4 * (size_t)row] = (double)(2 * l + 1);
    c[4 * (size_t)row + 1] = std::sqrt((double)((l + 2) * (l - 2))) * (double)(l + 2) / (double)l;
    c[4 * (size_t)row + 2] = 4.0 * (double)(2 * l + 1) / (double)((l + 1) * l);
    c[4 * (size_t)row + 3] = std::sqrt((double)((l + 3) * (l - 1))) * (double)(l - 1) / (double)(l + 1);
  }
  return c;
}

// get_n_max (mie_helper_functions.jl:17) and the start of the downward recurrence (compute_NAI2.jl:94-95); round = to nearest even
int mie_n_max(double x) { return (int)std::nearbyint(x + 4.05 * std::pow(x, 1.0 / 3.0) + 10.0); }
int mie_nmx(double x, int nmax, double n_r, double n_i) {
  return (int)std::nearbyint(std::fmax((double)nmax, std::fabs(x * (n_r - n_i))) + 51.0);
}

// sin x | cos x for k_mie_ab, [2, n]: the host library's, which rounds correctly in all but a few arguments in a thousand
std::vector<double> mie_sin_cos(const double *x, int n, size_t ld) {
  std::vector<double> sc(2 * ld, 0.0);
  for (int i = 0; i < n; ++i) {
    sc[i] = std::sin(x[i]);
    sc[ld + i] = std::cos(x[i]);
  }
  return sc;
}

int mie_device(const char *fn, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    char buf[128];
    snprintf(buf, sizeof buf, "%s: no HIP device available", fn);
    mom_set_global_error(buf);
    return MOM_EHIP;
  }
  if (device < 0 || device >= ndev) return mie_fail(fn, "device index out of range");
  return MOM_OK;
}

#define MCHK(call)                                                                                     \
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

template <int NW, bool DUAL>
void launch_amp(hipStream_t st, int nMuP, int G, int nL, int nR, int nRp, int Kp, int nTiles, const MieWave *waves, const double *tau,
                const double *pi, const double *const *pl, const double *x, const int *nmax, const double *w, int fullK,
                double *partial) {
  const dim3 grid(nMuP / (DUAL ? 16 : kMuBlock), G, nL);
  const MieDualPlanes dp = {pl[4], pl[5], pl[6], pl[7]};
  hipLaunchKernelGGL((k_mie_amp<NW, DUAL>), grid, dim3(64), 0, st, nR, nMuP, nRp, Kp, nTiles, G, waves, tau, pi, pl[0], pl[1], pl[2], pl[3],
                     x, nmax, w, fullK, partial, dp);
}

void launch_tables(hipStream_t st, int n_mu, int ldTab, int n_max, int l_max, const double *mu, const double *coef, double *pi,
                   double *tau, double *const *leg) {
  hipLaunchKernelGGL(k_mie_tables, dim3((n_mu + 63) / 64), dim3(64), 0, st, n_mu, ldTab, n_max, l_max, mu, coef, std::sqrt(1.5),
                     std::sqrt(6.0), pi, tau, leg[0], leg[1], leg[2], leg[3]);
}

// the device memory one sub-batch of a spectral call may take (max_batch = 0): the planes of a wavelength are its bulk
constexpr size_t kSpectralWorkspaceBytes = (size_t)2 << 30;
constexpr int kMaxBatch = 65535;  // wavelengths per launch: a grid's y and z extents

// The tables of a single-wavelength call come from the host, [n_max, n_mu] and [l_max, n_mu]
struct MieHostTables {
  const double *pi, *tau, *leg[4];
};

// All four NAI-2 entry points.  mom_mie_nai2 (dual = false) and mom_mie_nai2_dual (dual = true) differ in the kernel forms, in the
// four more planes, the two more D planes and the four more per-radius sums of the Dual run, and in nO = nW + 2 output rows.  The
// single-wavelength calls (tabs given, mu null, nL = 1) upload the host's tables; the spectral calls (mu given, tabs null) build
// them with k_mie_tables and run their nL wavelengths in sub-batches of at most B consecutive ones.  Every kernel treats a
// wavelength by itself (grid dimension), with the chunk count G of the single call, so its rows do not depend on the batch.
int mie_nai2_run(const char *fn, bool dual, int device, int nR, const double *r, int nW, const double *w, int nL, const double *lambda,
                 const double *n_r, const double *n_i, int n_mu, const double *mu, const double *w_mu, int n_max,
                 const MieHostTables *tabs, int l_max, int flags, int max_batch, double *bulk_f, double *C, double *greek,
                 double *ms4) {
  const bool spectral = tabs == nullptr;
  if (nR < 1 || n_mu < 1) return mie_fail(fn, "nR and n_mu must be at least 1");
  if (nW < 1 || nW > (dual ? MOM_MIE_DUAL_MAX_WEIGHT_ROWS : MOM_MIE_MAX_WEIGHT_ROWS)) return mie_fail(fn, dual ? "nW must be 1..3" : "nW must be 1..4");
  if (nL < 1) return mie_fail(fn, "nL must be at least 1");
  if (max_batch < 0) return mie_fail(fn, "max_batch must be >= 0 (0: sized to the workspace budget)");
  if (!lambda || !n_r || !n_i) return mie_fail(fn, "null pointer");
  for (int j = 0; j < nL; ++j) {
    const int at = spectral ? j : -1;
    if (!(lambda[j] > 0.0)) return mie_fail_at(fn, at, "lambda must be positive");
    if (!(n_i[j] >= 0.0) || !std::isfinite(n_r[j]) || !std::isfinite(n_i[j])) return mie_fail_at(fn, at, "n_i must be >= 0 (m = n_r + i n_i)");
  }
  if (l_max < 1 || n_max < 1) return mie_fail(fn, "l_max and n_max must be at least 1");
  if (flags & ~MOM_MIE_FULL_K) return mie_fail(fn, "unknown flag");
  if (!r || !w || !w_mu || !bulk_f || !C || !greek || (spectral && !mu) ||
      (!spectral && (!tabs->pi || !tabs->tau || !tabs->leg[0] || !tabs->leg[1] || !tabs->leg[2] || !tabs->leg[3])))
    return mie_fail(fn, "null pointer");
  if (!(r[0] > 0.0) || !std::isfinite(r[nR - 1])) return mie_fail(fn, "r[0] must be positive and r finite");
  for (int i = 1; i < nR; ++i)
    if (!(r[i] > r[i - 1])) return mie_fail(fn, "r must be ascending");
  const size_t nRp = round_up(nR, kTileR), Kp = round_up(n_max, kKStep), nMuP = round_up(n_mu, kMuBlock);
  // per wavelength, [nL, nRp] each: x = k r, sin x, cos x, n_max,i, nmx_i
  std::vector<double> hx(nL * nRp, 0.0), hsin(nL * nRp, 0.0), hcos(nL * nRp, 0.0);
  std::vector<int> hnmax(nL * nRp, 0), hnmx(nL * nRp, 0);
  for (int j = 0; j < nL; ++j) {
    const int at = spectral ? j : -1;
    const double kw = 2.0 * M_PI / lambda[j];  // wavenumber
    double *x = hx.data() + j * nRp;
    int *nm = hnmax.data() + j * nRp, *nx = hnmx.data() + j * nRp;
    for (int i = 0; i < nR; ++i) {
      x[i] = kw * r[i];
      nm[i] = mie_n_max(x[i]);
      nx[i] = mie_nmx(x[i], nm[i], n_r[j], n_i[j]);
      if (nm[i] > n_max) return mie_fail_at(fn, at, "n_max is smaller than the largest per-radius n_max");
      if (i > 0 && nm[i] < nm[i - 1]) return mie_fail_at(fn, at, "per-radius n_max not monotone");
    }
    const std::vector<double> sc = mie_sin_cos(x, nR, nRp);
    std::copy(sc.begin(), sc.begin() + nRp, hsin.begin() + j * nRp);
    std::copy(sc.begin() + nRp, sc.end(), hcos.begin() + j * nRp);
  }
  int rc = mie_device(fn, device);
  if (rc != MOM_OK) return rc;

  const int nTiles = (int)(nRp / kTileR), nMuBlk = (int)(nMuP / kMuBlock);
  int G = 2048 / nMuBlk;  // about two wavefronts per SIMD of the device, at most kMaxChunks partials per bulk element
  G = G < 1 ? 1 : (G > kMaxChunks ? kMaxChunks : G);
  G = G > nTiles ? nTiles : G;  // the same chunks in both forms: the rows they share are bitwise equal
  const int nO = dual ? nW + MOM_MIE_INDEX_ROWS : nW;      // output rows
  const int nPlanes = dual ? 8 : 4, nDp = dual ? 4 : 2, nSum = dual ? 6 : 2;
  // one allocation, carved in doubles: what the wavelengths share, then the arrays of a sub-batch, each [B, ...] (the MieWave
  // array and the two int arrays last)
  const size_t nTab = Kp * nMuP, nPl = Kp * nRp, nD = (size_t)n_max * nRp, nLeg = (size_t)l_max * n_mu;
  const size_t nPart = (size_t)G * nO * 4 * nMuP, nBulk = (size_t)nO * 4 * n_mu, nGreek = (size_t)nO * 6 * l_max;
  const size_t nShared = 2 * nTab + (size_t)nW * nRp + n_mu + 4 * nLeg + (spectral ? n_mu + 4 * (size_t)l_max : 0);
  const size_t perWave = nPlanes * nPl + nDp * nD + (3 + nSum) * nRp + nPart + nBulk + nGreek;
  const size_t perWaveBytes = perWave * sizeof(double) + sizeof(MieWave) + 2 * nRp * sizeof(int);
  size_t B = max_batch > 0 ? (size_t)max_batch : kSpectralWorkspaceBytes / perWaveBytes;
  B = B < 1 ? 1 : B;
  B = B > (size_t)nL ? (size_t)nL : B;
  B = B > (size_t)kMaxBatch ? (size_t)kMaxBatch : B;
  const size_t sharedBytes = nShared * sizeof(double), batchBytes = B * perWaveBytes, bytes = sharedBytes + batchBytes;
  char *base = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // sub-batch: 0 .. 3; tables: 4, 5
  std::vector<double> hs(B * nSum * nRp);
  std::vector<MieWave> hw(B);
  const std::vector<double> hcoef = spectral ? mie_table_coef(l_max) : std::vector<double>();
  double ms[4] = {0.0, 0.0, 0.0, 0.0};  // tables, coefficients, GEMM with reduction, projection
  MCHK(hipSetDevice(device));
  MCHK(hipStreamCreate(&st));
  MCHK(hipMalloc((void **)&base, bytes));
  {
    double *p = (double *)base;
    double *d_tau = p; p += nTab;
    double *d_pi = p; p += nTab;
    double *d_w = p; p += (size_t)nW * nRp;
    double *d_wmu = p; p += n_mu;
    double *d_leg[4];
    for (int q = 0; q < 4; ++q) { d_leg[q] = p; p += nLeg; }
    double *d_mu = nullptr, *d_coef = nullptr;
    if (spectral) {
      d_mu = p; p += n_mu;
      d_coef = p; p += 4 * (size_t)l_max;
    }
    double *d_pl[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // c a, c b; Dual: c a', c b'
    for (int q = 0; q < nPlanes; ++q) d_pl[q] = p + q * nPl;  // [B, nPlanes, nPl]
    p += B * nPlanes * nPl;
    double *d_D[4] = {nullptr, nullptr, nullptr, nullptr};  // D re, im; Dual: D' re, im
    for (int q = 0; q < nDp; ++q) d_D[q] = p + q * nD;  // [B, nDp, nD]
    p += B * nDp * nD;
    double *d_x = p; p += B * nRp;
    double *d_sin = p; p += B * nRp;
    double *d_cos = p; p += B * nRp;
    // [B, nSum, nRp]: sum (2n+1)(|a|^2 + |b|^2) | sum (2n+1) Re(a + b); Dual: their d/dn_r forms, then their d/dn_i forms
    double *d_ss = p; p += B * nSum * nRp;
    double *d_part = p; p += B * nPart;
    double *d_bulk = p; p += B * nBulk;
    double *d_greek = p; p += B * nGreek;
    MieWave *d_waves = (MieWave *)p;
    int *d_n = (int *)(d_waves + B);  // n_max,i [B, nRp] | nmx_i [B, nRp]
    MCHK(hipMemsetAsync(base, 0, bytes, st));  // the padding of every table and plane, and the planes above each radius' n_max
    for (int q = 0; q < 6; ++q) MCHK(hipEventCreate(&ev[q]));
    MCHK(hipMemcpy2DAsync(d_w, nRp * sizeof(double), w, (size_t)nR * sizeof(double), (size_t)nR * sizeof(double), nW,
                          hipMemcpyHostToDevice, st));
    MCHK(hipMemcpyAsync(d_wmu, w_mu, (size_t)n_mu * sizeof(double), hipMemcpyHostToDevice, st));
    if (spectral) {
      MCHK(hipMemcpyAsync(d_mu, mu, (size_t)n_mu * sizeof(double), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice, st));
      MCHK(hipEventRecord(ev[4], st));
      launch_tables(st, n_mu, (int)nMuP, n_max, l_max, d_mu, d_coef, d_pi, d_tau, d_leg);
      MCHK(hipGetLastError());
      MCHK(hipEventRecord(ev[5], st));
    } else {
      MCHK(hipMemcpy2DAsync(d_tau, nMuP * sizeof(double), tabs->tau, (size_t)n_mu * sizeof(double), (size_t)n_mu * sizeof(double), n_max,
                            hipMemcpyHostToDevice, st));
      MCHK(hipMemcpy2DAsync(d_pi, nMuP * sizeof(double), tabs->pi, (size_t)n_mu * sizeof(double), (size_t)n_mu * sizeof(double), n_max,
                            hipMemcpyHostToDevice, st));
      for (int q = 0; q < 4; ++q) MCHK(hipMemcpyAsync(d_leg[q], tabs->leg[q], nLeg * sizeof(double), hipMemcpyHostToDevice, st));
    }
    for (size_t j0 = 0; j0 < (size_t)nL; j0 += B) {
      const size_t nb = std::min(B, (size_t)nL - j0);  // this sub-batch: wavelengths j0 .. j0 + nb - 1
      // a workspace used before holds the planes of other wavelengths: above a radius' own n_max they have to be exact zeros again
      if (j0 > 0) MCHK(hipMemsetAsync(base + sharedBytes, 0, batchBytes, st));
      for (size_t b = 0; b < nb; ++b)
        hw[b] = {n_r[j0 + b], n_i[j0 + b], (long long)(b * nRp), (long long)(b * nSum * nRp), (long long)(b * nDp * nD),
                 (long long)(b * nPlanes * nPl)};
      MCHK(hipMemcpyAsync(d_waves, hw.data(), nb * sizeof(MieWave), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_x, hx.data() + j0 * nRp, nb * nRp * sizeof(double), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_sin, hsin.data() + j0 * nRp, nb * nRp * sizeof(double), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_cos, hcos.data() + j0 * nRp, nb * nRp * sizeof(double), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_n, hnmax.data() + j0 * nRp, nb * nRp * sizeof(int), hipMemcpyHostToDevice, st));
      MCHK(hipMemcpyAsync(d_n + B * nRp, hnmx.data() + j0 * nRp, nb * nRp * sizeof(int), hipMemcpyHostToDevice, st));
      MCHK(hipEventRecord(ev[0], st));
      {
        const MieDualOut dd = {d_D[2], d_D[3], d_pl[4], d_pl[5], d_pl[6], d_pl[7], dual ? d_ss + 2 * nRp : nullptr};
        const dim3 grid((nR + 63) / 64, (unsigned)nb);
        if (dual)
          hipLaunchKernelGGL((k_mie_ab<true, true>), grid, dim3(64), 0, st, nR, (int)nRp, d_waves, d_x, d_sin, d_cos, d_n, d_n + B * nRp, d_D[0],
                             d_D[1], d_pl[0], d_pl[1], d_pl[2], d_pl[3], d_ss, d_ss + nRp, dd);
        else
          hipLaunchKernelGGL((k_mie_ab<true, false>), grid, dim3(64), 0, st, nR, (int)nRp, d_waves, d_x, d_sin, d_cos, d_n, d_n + B * nRp, d_D[0],
                             d_D[1], d_pl[0], d_pl[1], d_pl[2], d_pl[3], d_ss, d_ss + nRp, dd);
      }
      MCHK(hipGetLastError());
      MCHK(hipEventRecord(ev[1], st));
      {
        const int fullK = (flags & MOM_MIE_FULL_K) ? 1 : 0;
#define MIE_AMP(NW, DUAL) \
  launch_amp<NW, DUAL>(st, (int)nMuP, G, (int)nb, nR, (int)nRp, (int)Kp, nTiles, d_waves, d_tau, d_pi, d_pl, d_x, d_n, d_w, fullK, d_part)
        switch (dual ? 4 + nW : nW) {
          case 1: MIE_AMP(1, false); break;
          case 2: MIE_AMP(2, false); break;
          case 3: MIE_AMP(3, false); break;
          case 4: MIE_AMP(4, false); break;
          case 5: MIE_AMP(1, true); break;
          case 6: MIE_AMP(2, true); break;
          default: MIE_AMP(3, true); break;
        }
#undef MIE_AMP
        MCHK(hipGetLastError());
        hipLaunchKernelGGL(k_mie_sum, dim3((unsigned)((nBulk + 255) / 256), (unsigned)nb), dim3(256), 0, st, G, nO * 4, n_mu, (int)nMuP, d_part,
                           d_bulk);
        MCHK(hipGetLastError());
      }
      MCHK(hipEventRecord(ev[2], st));
      hipLaunchKernelGGL(k_mie_greek, dim3(l_max, nO, (unsigned)nb), dim3(64), 0, st, n_mu, l_max, d_wmu, d_bulk, d_leg[0], d_leg[1], d_leg[2],
                         d_leg[3], d_greek);
      MCHK(hipGetLastError());
      MCHK(hipEventRecord(ev[3], st));
      MCHK(hipMemcpyAsync(bulk_f + j0 * nBulk, d_bulk, nb * nBulk * sizeof(double), hipMemcpyDeviceToHost, st));
      MCHK(hipMemcpyAsync(greek + j0 * nGreek, d_greek, nb * nGreek * sizeof(double), hipMemcpyDeviceToHost, st));
      MCHK(hipMemcpyAsync(hs.data(), d_ss, nb * nSum * nRp * sizeof(double), hipMemcpyDeviceToHost, st));
      MCHK(hipStreamSynchronize(st));
      // C_sca,i = 2 pi / k^2 * sum, weighted by w_i / (4 pi r_i^2): w_i * sum_i / (2 x_i^2), added in radius order (the terms in
      // Float64, the running sum in the host's long double, so that the O(nR) sum adds no rounding of its own).  The two index rows
      // of the Dual run: weight row 0 on the d/dn_r and d/dn_i sums.
      for (size_t b = 0; b < nb; ++b) {
        const double *x = hx.data() + (j0 + b) * nRp, *sb = hs.data() + b * nSum * nRp;
        for (int k = 0; k < nO; ++k)
          for (int q = 0; q < 2; ++q) {
            const double *wk = w + (size_t)(k < nW ? k : 0) * nR, *sk = sb + (size_t)((k < nW ? 0 : 2 * (k - nW + 1)) + q) * nRp;
            long double acc = 0.0L;
            for (int i = 0; i < nR; ++i) acc += (long double)(wk[i] * (sk[i] / (2.0 * x[i] * x[i])));
            C[((j0 + b) * nO + k) * 2 + q] = (double)acc;
          }
      }
      for (int q = 0; q < 3; ++q) {
        float t = 0.f;
        MCHK(hipEventElapsedTime(&t, ev[q], ev[q + 1]));
        ms[q + 1] += t;
      }
    }
    if (spectral) {
      float t = 0.f;
      MCHK(hipEventElapsedTime(&t, ev[4], ev[5]));
      ms[0] = t;
    }
    if (ms4)
      for (int q = 0; q < 4; ++q) ms4[q] = ms[q];
  }
done:
  for (int q = 0; q < 6; ++q)
    if (ev[q]) (void)hipEventDestroy(ev[q]);
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

// mom_mie_tables: the tables alone, in the layouts of the C ABI ([n_max, n_mu] and [l_max, n_mu], mu fastest, no padding)
int mie_tables_run(const char *fn, int device, int n_mu, const double *mu, int n_max, int l_max, double *pi_tab, double *tau_tab,
                   double *const *leg) {
  if (n_mu < 1 || n_max < 1 || l_max < 1) return mie_fail(fn, "n_mu, n_max and l_max must be at least 1");
  if (!mu || !pi_tab || !tau_tab || !leg[0] || !leg[1] || !leg[2] || !leg[3]) return mie_fail(fn, "null pointer");
  int rc = mie_device(fn, device);
  if (rc != MOM_OK) return rc;
  const size_t nTab = (size_t)n_max * n_mu, nLeg = (size_t)l_max * n_mu;
  const size_t bytes = (2 * nTab + 4 * nLeg + n_mu + 4 * (size_t)l_max) * sizeof(double);
  const std::vector<double> hcoef = mie_table_coef(l_max);
  char *base = nullptr;
  hipStream_t st = nullptr;
  MCHK(hipSetDevice(device));
  MCHK(hipStreamCreate(&st));
  MCHK(hipMalloc((void **)&base, bytes));
  {
    double *d_pi = (double *)base, *d_tau = d_pi + nTab;
    double *d_leg[4] = {d_tau + nTab, d_tau + nTab + nLeg, d_tau + nTab + 2 * nLeg, d_tau + nTab + 3 * nLeg};
    double *d_mu = d_leg[3] + nLeg, *d_coef = d_mu + n_mu;
    MCHK(hipMemcpyAsync(d_mu, mu, (size_t)n_mu * sizeof(double), hipMemcpyHostToDevice, st));
    MCHK(hipMemcpyAsync(d_coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice, st));
    launch_tables(st, n_mu, n_mu, n_max, l_max, d_mu, d_coef, d_pi, d_tau, d_leg);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(pi_tab, d_pi, nTab * sizeof(double), hipMemcpyDeviceToHost, st));
    MCHK(hipMemcpyAsync(tau_tab, d_tau, nTab * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int q = 0; q < 4; ++q) MCHK(hipMemcpyAsync(leg[q], d_leg[q], nLeg * sizeof(double), hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
  }
done:
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

// mom_mie_coefficients (out: a, b as four planes) and mom_mie_coefficients_dual (out: then a', b' as four more)
int mie_coefficients_run(const char *fn, bool dual, int device, int nX, const double *x, double n_r, double n_i, int n_max,
                         double *const *out) {
  bool null = !x;
  for (int q = 0; q < (dual ? 8 : 4); ++q) null = null || !out[q];
  if (nX < 1 || n_max < 1 || null) return mie_fail(fn, "bad argument (null pointer or non-positive size)");
  if (!(n_i >= 0.0) || !std::isfinite(n_r) || !std::isfinite(n_i)) return mie_fail(fn, "n_i must be >= 0 (m = n_r + i n_i)");
  for (int i = 0; i < nX; ++i) {
    if (!(x[i] > 0.0) || !std::isfinite(x[i])) return mie_fail(fn, "x must be positive");
    if (mie_n_max(x[i]) > n_max) return mie_fail(fn, "n_max is smaller than the largest per-x n_max");
  }
  int rc = mie_device(fn, device);
  if (rc != MOM_OK) return rc;
  const size_t nPl = (size_t)n_max * nX;
  const int nOut = dual ? 8 : 4;  // planes a, b (Dual: a', b')
  const size_t bytes = nOut * nPl * sizeof(double) + mom_mie_ab::workspace_bytes(n_max, (size_t)nX, dual);
  char *base = nullptr;
  hipStream_t st = nullptr;
  MCHK(hipSetDevice(device));
  MCHK(hipStreamCreate(&st));
  MCHK(hipMalloc((void **)&base, bytes));
  {
    double *d_pl = (double *)base;
    const int *d_n = nullptr;
    MCHK(hipMemsetAsync(base, 0, bytes, st));
    rc = mom_mie_ab::launch(fn, st, nX, (size_t)nX, x, n_r, n_i, n_max, nPl, d_pl, base + nOut * nPl * sizeof(double), nullptr, &d_n, nullptr,
                            nullptr, dual);
    if (rc != MOM_OK) goto done;
    for (int q = 0; q < nOut; ++q) MCHK(hipMemcpyAsync(out[q], d_pl + q * nPl, nPl * sizeof(double), hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
  }
done:
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

}  // namespace

// ---- the coefficient kernel for the other routes (mom_mie_ab.hpp) ---------------------------------------------------------
namespace mom_mie_ab {

int n_max_of(double x) { return mie_n_max(x); }

size_t workspace_bytes(int n_max, size_t ld, bool dual) {
  return ((dual ? 4 : 2) * (size_t)n_max * ld + 3 * ld) * sizeof(double) + sizeof(MieWave) + 2 * ld * sizeof(int);
}

int launch(const char *fn, hipStream_t st, int nX, size_t ld, const double *x, double n_r, double n_i, int n_max, size_t plane_stride,
           double *d_planes, char *d_ws, int *h_nmax, const int **d_nmax, hipEvent_t ev0, hipEvent_t ev1, bool dual) {
  std::vector<int> hn(2 * ld, 0);
  for (int i = 0; i < nX; ++i) {
    hn[i] = mie_n_max(x[i]);
    hn[ld + i] = mie_nmx(x[i], hn[i], n_r, n_i);
    if (hn[i] > n_max) return mie_fail(fn, "n_max is smaller than the largest per-x n_max");
    if (h_nmax) h_nmax[i] = hn[i];
  }
  const MieWave hw = {n_r, n_i, 0, 0, 0, 0};  // a batch of one
  const std::vector<double> hsc = mie_sin_cos(x, nX, ld);
  const size_t nD = (size_t)n_max * ld, ps = plane_stride;
  double *d_D = (double *)d_ws, *d_x = d_D + (dual ? 4 : 2) * nD, *d_sc = d_x + ld;  // D (Dual: D'), x, sin x | cos x
  MieWave *d_wave = (MieWave *)(d_sc + 2 * ld);
  int *d_n = (int *)(d_wave + 1);
  int rc = MOM_OK;
  MCHK(hipMemcpyAsync(d_wave, &hw, sizeof hw, hipMemcpyHostToDevice, st));
  MCHK(hipMemcpyAsync(d_x, x, (size_t)nX * sizeof(double), hipMemcpyHostToDevice, st));
  MCHK(hipMemcpyAsync(d_sc, hsc.data(), 2 * ld * sizeof(double), hipMemcpyHostToDevice, st));
  MCHK(hipMemcpyAsync(d_n, hn.data(), 2 * ld * sizeof(int), hipMemcpyHostToDevice, st));
  MCHK(hipStreamSynchronize(st));  // the host arrays above end with this call
  if (ev0) MCHK(hipEventRecord(ev0, st));
  {
    const dim3 grid((nX + 63) / 64);
    if (dual) {
      const MieDualOut dd = {d_D + 2 * nD, d_D + 3 * nD, d_planes + 4 * ps, d_planes + 5 * ps, d_planes + 6 * ps, d_planes + 7 * ps, nullptr};
      hipLaunchKernelGGL((k_mie_ab<false, true>), grid, dim3(64), 0, st, nX, (int)ld, d_wave, d_x, d_sc, d_sc + ld, d_n, d_n + ld, d_D, d_D + nD,
                         d_planes, d_planes + ps, d_planes + 2 * ps, d_planes + 3 * ps, (double *)nullptr, (double *)nullptr, dd);
    } else {
      const MieDualOut dd = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      hipLaunchKernelGGL((k_mie_ab<false, false>), grid, dim3(64), 0, st, nX, (int)ld, d_wave, d_x, d_sc, d_sc + ld, d_n, d_n + ld, d_D, d_D + nD,
                         d_planes, d_planes + ps, d_planes + 2 * ps, d_planes + 3 * ps, (double *)nullptr, (double *)nullptr, dd);
    }
  }
  MCHK(hipGetLastError());
  if (ev1) MCHK(hipEventRecord(ev1, st));
  *d_nmax = d_n;
done:
  return rc;
}

}  // namespace mom_mie_ab

// the single-wavelength calls: the batch of one on the host's tables; gpu_ms [3] is without the tables group
static int mie_nai2_single(const char *fn, bool dual, int device, int nR, const double *r, int nW, const double *w, double lambda,
                           double n_r, double n_i, int n_mu, const double *w_mu, int n_max, const double *pi_tab, const double *tau_tab,
                           int l_max, const double *P, const double *P2, const double *R2, const double *T2, int flags, double *bulk_f,
                           double *C, double *greek, double *gpu_ms) {
  const MieHostTables tabs = {pi_tab, tau_tab, {P, P2, R2, T2}};
  double ms[4];
  const int rc = mie_nai2_run(fn, dual, device, nR, r, nW, w, 1, &lambda, &n_r, &n_i, n_mu, nullptr, w_mu, n_max, &tabs, l_max, flags, 0,
                              bulk_f, C, greek, ms);
  if (rc == MOM_OK && gpu_ms)
    for (int q = 0; q < 3; ++q) gpu_ms[q] = ms[q + 1];
  return rc;
}

extern "C" int mom_mie_nai2(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                            int n_mu, const double *w_mu, int n_max, const double *pi_tab, const double *tau_tab, int l_max,
                            const double *P, const double *P2, const double *R2, const double *T2, int flags, double *bulk_f,
                            double *C, double *greek, double *gpu_ms) {
  return mie_nai2_single("mom_mie_nai2", false, device, nR, r, nW, w, lambda, n_r, n_i, n_mu, w_mu, n_max, pi_tab, tau_tab, l_max, P, P2,
                         R2, T2, flags, bulk_f, C, greek, gpu_ms);
}

extern "C" int mom_mie_nai2_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                                 int n_mu, const double *w_mu, int n_max, const double *pi_tab, const double *tau_tab, int l_max,
                                 const double *P, const double *P2, const double *R2, const double *T2, int flags, double *bulk_f,
                                 double *C, double *greek, double *gpu_ms) {
  return mie_nai2_single("mom_mie_nai2_dual", true, device, nR, r, nW, w, lambda, n_r, n_i, n_mu, w_mu, n_max, pi_tab, tau_tab, l_max, P,
                         P2, R2, T2, flags, bulk_f, C, greek, gpu_ms);
}

extern "C" int mom_mie_nai2_spectral(int device, int nR, const double *r, int nW, const double *w, int nL, const double *lambda,
                                     const double *n_r, const double *n_i, int n_mu, const double *mu, const double *w_mu, int n_max,
                                     int l_max, int flags, int max_batch, double *bulk_f, double *C, double *greek, double *gpu_ms) {
  return mie_nai2_run("mom_mie_nai2_spectral", false, device, nR, r, nW, w, nL, lambda, n_r, n_i, n_mu, mu, w_mu, n_max, nullptr, l_max,
                      flags, max_batch, bulk_f, C, greek, gpu_ms);
}

extern "C" int mom_mie_nai2_spectral_dual(int device, int nR, const double *r, int nW, const double *w, int nL, const double *lambda,
                                          const double *n_r, const double *n_i, int n_mu, const double *mu, const double *w_mu,
                                          int n_max, int l_max, int flags, int max_batch, double *bulk_f, double *C, double *greek,
                                          double *gpu_ms) {
  return mie_nai2_run("mom_mie_nai2_spectral_dual", true, device, nR, r, nW, w, nL, lambda, n_r, n_i, n_mu, mu, w_mu, n_max, nullptr,
                      l_max, flags, max_batch, bulk_f, C, greek, gpu_ms);
}

extern "C" int mom_mie_tables(int device, int n_mu, const double *mu, int n_max, int l_max, double *pi_tab, double *tau_tab, double *P,
                              double *P2, double *R2, double *T2) {
  double *const leg[4] = {P, P2, R2, T2};
  return mie_tables_run("mom_mie_tables", device, n_mu, mu, n_max, l_max, pi_tab, tau_tab, leg);
}

extern "C" int mom_mie_coefficients(int device, int nX, const double *x, double n_r, double n_i, int n_max, double *a_re, double *a_im,
                                    double *b_re, double *b_im) {
  double *const out[8] = {a_re, a_im, b_re, b_im, nullptr, nullptr, nullptr, nullptr};
  return mie_coefficients_run("mom_mie_coefficients", false, device, nX, x, n_r, n_i, n_max, out);
}

extern "C" int mom_mie_coefficients_dual(int device, int nX, const double *x, double n_r, double n_i, int n_max, double *a_re,
                                         double *a_im, double *b_re, double *b_im, double *da_re, double *da_im, double *db_re,
                                         double *db_im) {
  double *const out[8] = {a_re, a_im, b_re, b_im, da_re, da_im, db_re, db_im};
  return mie_coefficients_run("mom_mie_coefficients_dual", true, device, nX, x, n_r, n_i, n_max, out);
}

// ---- the Legendre tables for other units (mom_host.hpp): k_mie_tables with the pi / tau part cut to its first row ------------
std::vector<double> mom_legendre_table_coef(int l_max) { return mie_table_coef(l_max); }

hipError_t mom_legendre_tables_launch(hipStream_t st, int n_mu, int l_max, const double *mu, const double *coef, double *pitau,
                                      double *const *leg) {
  launch_tables(st, n_mu, n_mu, 1, l_max, mu, coef, pitau, pitau + n_mu, leg);
  return hipGetLastError();
}
