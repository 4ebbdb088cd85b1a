// voigt.hip -- line-by-line absorption cross section on gfx950.
//
// Restates line_shape!(::Voigt) (src/Absorption/compute_absorption_cross_section.jl:179-183)
// with w(::HumlicekWeidemann32SDErrorFunction, z) (complex_error_functions.jl:226-234:
// humlicek2 :24-30 for |x|+y >= 8, weideman32a :170-190 otherwise), accumulated over the
// host loop over lines (:73-126).  The other absorption models -- line_shape!(::Doppler) (:167-171),
// line_shape!(::Lorentz) (:173-177) and Voigt with w(::HumlicekWeidemann32VoigtErrorFunction, z)
// (complex_error_functions.jl:210-219) -- are further instantiations of the same block (LineShape below).  The reference launches one kernel per line; here ONE
// launch covers all lines: a workgroup owns 256 consecutive grid points, compacts (in line
// order) the lines whose window overlaps its range into LDS, and every thread sums its grid
// point's contributions in ascending line order -- the same accumulation order as the
// reference's sequential `A[I] += ...`, with no atomics, so results are reproducible.
// FP64 VALU-bound (about 300 flop per (line, grid point) evaluation), negligible HBM bytes.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "momcore.h"
#include "mom_host.hpp"

namespace {

struct cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__constant__ double kW32A[32] = {
    2.5722534081245696e+00,  2.2635372999002676e+00,  1.8256696296324824e+00,  1.3455441692345453e+00,
    9.0192548936480144e-01,  5.4601397206393498e-01,  2.9544451071508926e-01,  1.4060716226893769e-01,
    5.7304403529837900e-02,  1.9006155784845689e-02,  4.5195411053501429e-03,  3.9259136070122748e-04,
    -2.4532980269928922e-04, -1.3075449254548613e-04, -2.1409619200870880e-05, 6.8210319440412389e-06,
    4.4015317319048931e-06,  4.2558331390536872e-07,  -4.1840763666294341e-07, -1.4813078891201116e-07,
    2.2930439569075392e-08,  2.3797557105844622e-08,  8.1248960947953431e-10,  -3.2080150458594088e-09,
    -5.2310170266050247e-10, 4.1537465934749353e-10,  1.1658312885903929e-10,  -5.5441820344468828e-11,
    -2.1542618451370239e-11, 8.0314997274316680e-12,  3.7424975634801558e-12,  -1.3031797863050087e-12};

// 1 / d and n / d for d in a range where neither scaling nor special cases are needed (here 22 <= d <= 1e60): v_rcp_f64
// refined by two Newton steps, the quotient by one residual step -- 8 instructions instead of the 12 of the IEEE division
// sequence (2 v_div_scale, v_div_fmas, v_div_fixup around the same Newton steps).  Measured point by point against the oracle in
// extended precision (tests/test_gpu_voigt_edges.py, |x| to 1e6, y from 1e-8 to 1e4): on the humlicek2 branch sigma is within
// 2.2e-15 of its own value and its partials within 3.2e-15 of theirs, where the Float64 oracle with IEEE division stands at
// 2.4e-15 and 3.6e-15 -- the substitution costs nothing that shows.
__device__ __forceinline__ double rcp_refined(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double div_refined(double n, double d) {
  const double r = rcp_refined(d), q = n * r;
  return fma(fma(-d, q, n), r, q);
}

// V15 = false: w(::HumlicekWeidemann32SDErrorFunction, z); V15 = true: w(::HumlicekWeidemann32VoigtErrorFunction, z)
// (complex_error_functions.jl:210-219): region I of Humlicek (1982), w = (i / sqrt(pi)) z / (z^2 - 1/2), where |x| + y > 15
// (strictly), weideman32a elsewhere
template <bool V15>
__device__ __forceinline__ double w_hw32_re(double x, double y) {
  const double rsp = 0.5641895835477563;  // 1/sqrt(pi)
  if constexpr (V15) {
    if (fabs(x) + y > 15.0) {
      const cplx z = {x, y};
      cplx den = cmul(z, z);
      den.re -= 0.5;
      const cplx num = {-(rsp * y), rsp * x};  // (i / sqrt(pi)) z
      // the real part of num / den by one division, as on the humlicek2 branch: |den| = |z^2 - 1/2| > 50 here
      return div_refined(num.re * den.re + num.im * den.im, den.re * den.re + den.im * den.im);
    }
  } else
  if (fabs(x) + y >= 8.0) {               // humlicek2, t = y - i x
    const cplx t = {y, -x};
    const cplx u = cmul(t, t);
    const cplx num = cmul(t, cplx{1.410474 + u.re * rsp, u.im * rsp});
    const cplx up3 = {3.0 + u.re, u.im};
    cplx den = cmul(u, up3);
    den.re += 0.75;
    // only the real part of num/den is needed: one division (|den| ~ |t|^4 >= 4e3 here and < 1e30 for any
    // line/grid distance in cm^-1 units, so the squares neither overflow nor underflow)
    return div_refined(num.re * den.re + num.im * den.im, den.re * den.re + den.im * den.im);
  }
  const double L = 4.756828460010884;  // sqrt(32/sqrt(2))
  const cplx lpiz = {L - y, x}, lmiz = {L + y, -x};
  // 1 / (L - i z) = conj / |.|^2: ONE division and no branch (Julia's complex division, complex.jl, is Smith's
  // branching three-division scheme; |L - i z|^2 lies in [22, 200] here ([22, 400) below |x| + y = 15), so the plain form differs from it by rounding
  // only, and a wave no longer executes both branches.  Measured (tests/test_gpu_voigt_edges.py): relative to the terms the
  // rational form adds up, a |1 / (L - i z)| / sqrt(pi), sigma is within 6.4e-15 of the oracle in extended precision on this
  // branch -- the Float64 oracle with Smith's division 6.0e-15 -- and its partials within 8.9e-16 of their largest (7.9e-16))
  const double inv = rcp_refined(lmiz.re * lmiz.re + lmiz.im * lmiz.im);
  const cplx rec = {lmiz.re * inv, -lmiz.im * inv};
  const cplx Z = cmul(lpiz, rec);
  cplx p = {kW32A[31], 0.0};
#pragma unroll
  for (int k = 30; k >= 0; --k) {
    p = cmul(p, Z);
    p.re += kW32A[k];
  }
  cplx inner = cmul(cplx{2 * p.re, 2 * p.im}, rec);
  inner.re += rsp;
  return cmul(inner, rec).re;
}

// Dual run (ForwardDiff.Dual numbers through line_shape!(::Voigt)): Re w(z) as above and the complex derivative w'(z).  Both
// approximations are rational in z, so one w' serves every partial: d_k Re w = Re(w'(z) (d_k x + i d_k y)).  The branch is
// taken on the values, as ForwardDiff takes it.
//   humlicek2:   t = y - i x, u = t^2, w = N / D with N = t (1.410474 + u / sqrt(pi)), D = 3/4 + u (3 + u);
//                dw/dt = (N' - w D') / D with N' = 1.410474 + 3 u / sqrt(pi), D' = 2 t (3 + 2 u); dt/dz = -i
//   weideman32a: r = 1 / (L - i z), Z = (L + i z) r, P = sum a_k Z^k (P' carried by the same Horner loop),
//                w = (1 / sqrt(pi) + 2 P r) r;  r' = i r^2, Z' = i r (1 + Z),
//                w' = (2 P' Z' r + 2 P r') r + (1 / sqrt(pi) + 2 P r) r'
//   region I:    D = z^2 - 1/2, w = (i / sqrt(pi)) z / D, w' = -(i / sqrt(pi)) (z^2 + 1/2) / D^2
// The reciprocals take the refined form: |D|^2 > 1e5 and < 1e60, |L - i z|^2 in [22, 200] (see above); with V15 |L - i z|^2 stays
// below 400 and region I has |D|^2 > 2500.
template <bool V15>
__device__ __forceinline__ double w_hw32_dual(double x, double y, cplx &dw) {
  const double rsp = 0.5641895835477563;  // 1/sqrt(pi)
  if constexpr (V15) {
    if (fabs(x) + y > 15.0) {
      const cplx z = {x, y};
      const cplx u = cmul(z, z);
      const cplx den = {u.re - 0.5, u.im};
      const double inv = rcp_refined(den.re * den.re + den.im * den.im);
      const cplx rden = {den.re * inv, -den.im * inv};
      const cplx q = cmul(cplx{u.re + 0.5, u.im}, cmul(rden, rden));
      dw = {rsp * q.im, -(rsp * q.re)};  // times -i / sqrt(pi)
      return cmul(cplx{-(rsp * y), rsp * x}, rden).re;
    }
  } else
  if (fabs(x) + y >= 8.0) {
    const cplx t = {y, -x};
    const cplx u = cmul(t, t);
    const cplx num = cmul(t, cplx{1.410474 + u.re * rsp, u.im * rsp});
    const cplx up3 = {3.0 + u.re, u.im};
    cplx den = cmul(u, up3);
    den.re += 0.75;
    const double inv = rcp_refined(den.re * den.re + den.im * den.im);
    const cplx rden = {den.re * inv, -den.im * inv};
    const cplx w = cmul(num, rden);
    const cplx dnum = {1.410474 + 3.0 * u.re * rsp, 3.0 * u.im * rsp};
    const cplx dden = cmul(cplx{2.0 * t.re, 2.0 * t.im}, cplx{3.0 + 2.0 * u.re, 2.0 * u.im});
    const cplx wd = cmul(w, dden);
    const cplx q = cmul(cplx{dnum.re - wd.re, dnum.im - wd.im}, rden);  // dw/dt
    dw = {q.im, -q.re};                                                  // times dt/dz = -i
    return w.re;
  }
  const double L = 4.756828460010884;  // sqrt(32/sqrt(2))
  const cplx lpiz = {L - y, x}, lmiz = {L + y, -x};
  const double inv = rcp_refined(lmiz.re * lmiz.re + lmiz.im * lmiz.im);
  const cplx rec = {lmiz.re * inv, -lmiz.im * inv};
  const cplx Z = cmul(lpiz, rec);
  cplx p = {kW32A[31], 0.0}, dp = {0.0, 0.0};
#pragma unroll
  for (int k = 30; k >= 0; --k) {
    dp = cmul(dp, Z);
    dp.re += p.re;
    dp.im += p.im;
    p = cmul(p, Z);
    p.re += kW32A[k];
  }
  const cplx p2 = {2 * p.re, 2 * p.im};
  cplx inner = cmul(p2, rec);
  inner.re += rsp;
  const cplx r2 = cmul(rec, rec);
  const cplx dr = {-r2.im, r2.re};                                        // r' = i r^2
  const cplx dZ = cmul(cplx{-rec.im, rec.re}, cplx{1.0 + Z.re, Z.im});    // Z' = i r (1 + Z)
  const cplx a1 = cmul(cmul(cplx{2 * dp.re, 2 * dp.im}, dZ), rec), a2 = cmul(p2, dr);
  const cplx b1 = cmul(cplx{a1.re + a2.re, a1.im + a2.im}, rec), b2 = cmul(inner, dr);
  dw = {b1.re + b2.re, b1.im + b2.im};
  return cmul(inner, rec).re;
}

#ifndef MOM_VOIGT_BLOCK
#define MOM_VOIGT_BLOCK 256
#endif
constexpr int kBlock = MOM_VOIGT_BLOCK;  // grid points per workgroup

// Dual run of voigt_block: the partials of the per-line prefactors with respect to (k = 0) pressure and (k = 1) temperature,
// partial k of line j at p[j + ks k] (a null array counts as zeros), and the output partials dsigma[g + os k]
struct VoigtDualArgs {
  const double *dnu, *dgd, *dy, *dS;
  size_t ks;
  double *dsigma;
  size_t os;
};

// The absorption model (HitranModel.broadening x HitranModel.CEF) as the compile-time shape of voigt_block.  It decides what is
// staged per candidate line, what is evaluated per (line, grid point) and which partials the Dual run stages; the candidate search,
// the ordered compaction, the accumulation order, the window compare and the tau_abs epilogue are the same for all four.
//   kVoigtSD, kVoigt15  a = S c / gamma_d, b = c' / gamma_d, y:  sigma = a Re w(b (g - nu) + i y)           (:179-183)
//   kDoppler            a = S c / gamma_d, b = 1 / gamma_d:      sigma = a exp(-ln 2 (b (g - nu))^2)        (:167-171)
//   kLorentz            a = S gamma_l, b = gamma_l^2:            sigma = a / (pi (b + (g - nu)^2))          (:173-177)
// MOM_BROADENING_* / MOM_CEF_* -> shape: mom_line_shape (mom_host.hpp)
enum LineShape : int { kVoigtSD = 0, kVoigt15 = 1, kDoppler = 2, kLorentz = 3 };

// DUAL = false is the value kernel; DUAL = true shares its candidate search and ordered compaction, stages d a, d b, d nu, d y
// (two each) next to a, b, nu, y and sums the two partials of every grid point in the same ascending line order.  gamma_l and its
// partials dgl (laid out like dd's arrays) are read by kLorentz only, gamma_d by the other three, y by the two Voigt shapes.
template <bool DUAL, int SHAPE>
__device__ __forceinline__ void voigt_block(int nLines, const double *__restrict__ nu,
                                            const double *__restrict__ gamma_d, const double *__restrict__ gamma_l,
                                            const double *__restrict__ y,
                                            const double *__restrict__ S, const int *__restrict__ i0,
                                            const int *__restrict__ i1, int nGrid,
                                            const double *__restrict__ grid, double *__restrict__ sigma,
                                            double factor, int accumulate, int sorted, const VoigtDualArgs dd,
                                            const double *__restrict__ dgl) {
  constexpr bool kIsVoigt = SHAPE == kVoigtSD || SHAPE == kVoigt15;
  // per-line constants of the candidates, staged once per workgroup: centre, S c/gamma_d, c'/gamma_d, y and the
  // 0-based window -- the two divisions by gamma_d are per LINE here, not per evaluation (same expressions, same values)
  __shared__ double c_nu[kBlock], c_a[kBlock], c_b[kBlock], c_y[kBlock];
  __shared__ int2 c_win[kBlock];  // {first point, last - first} of the window: ONE read and ONE unsigned compare per candidate
  __shared__ int wcount[kBlock / 64];
  __shared__ double c_d[DUAL ? 8 * kBlock : 1];  // Dual run: [d a | d b | d nu | d y][k][candidate]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = blockIdx.x * kBlock;             // 0-based first grid index of this block
  const int g1 = min(nGrid, g0 + kBlock) - 1;     // last
  const int gi = g0 + tid;
  const double gx = (gi < nGrid) ? grid[gi] : 0.0;
  const double cSqrtLn2divSqrtPi = 0.469718639319144059835, cSqrtLn2 = 0.8325546111577;
  [[maybe_unused]] const double cLn2 = 0.6931471805599, cPi = 3.141592653589793;
  const double kB = SHAPE == kDoppler ? 1.0 : cSqrtLn2;  // numerator of b
  double acc = 0.0;
  [[maybe_unused]] double dacc[2] = {0.0, 0.0};
  // Range [jlo, jhi] of line indices whose window touches this block: one cheap strided pass (two loads and a compare
  // per line, no barrier) instead of running the ordered compaction below over the whole list -- line lists are
  // sorted by wavenumber, so the range is tight (an unsorted list still works, it only gets no benefit).  The sum
  // stays in ascending line order.
  __shared__ int s_lo, s_hi;
  if (tid == 0) { s_lo = nLines; s_hi = -1; }
  __syncthreads();
  if (sorted) {
    // window starts and stops both non-decreasing in the line index (the host checked): two binary searches
    if (tid == 0) {
      int a = 0, b = nLines;
      while (a < b) { const int mid = (a + b) >> 1; if (i1[mid] - 1 >= g0) b = mid; else a = mid + 1; }
      s_lo = a;   // first line whose window ends at or after the block's first point
      a = 0; b = nLines;
      while (a < b) { const int mid = (a + b) >> 1; if (i0[mid] - 1 > g1) b = mid; else a = mid + 1; }
      s_hi = a - 1;  // last line whose window starts at or before the block's last point
    }
  } else {
    int mylo = nLines, myhi = -1;
    for (int j = tid; j < nLines; j += kBlock) {
      const int lo = i0[j] - 1, hi = i1[j] - 1;
      if (lo <= g1 && hi >= g0 && hi >= lo) { mylo = min(mylo, j); myhi = max(myhi, j); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mylo = min(mylo, __shfl_xor(mylo, off));
      myhi = max(myhi, __shfl_xor(myhi, off));
    }
    if (lane == 0) { atomicMin(&s_lo, mylo); atomicMax(&s_hi, myhi); }
  }
  __syncthreads();
  const int jlo = s_lo, jhi = s_hi;
  for (int base = jlo; base <= jhi; base += kBlock) {
    const int j = base + tid;
    bool hit = false;
    int lo = 0, hi = -1;
    if (j <= jhi) {
      lo = i0[j] - 1;
      hi = i1[j] - 1;
      hit = (lo <= g1) && (hi >= g0) && (hi >= lo);
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wcount[w];
    if (hit) {  // ordered compaction: candidates keep the line order (the reference's accumulation order)
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
      if constexpr (SHAPE == kLorentz) {  // a = S gamma_l, b = gamma_l^2 and their partials by the product rule
        const double gl = gamma_l[j], s = S[j];
        c_nu[pos] = nu[j];
        c_a[pos] = s * gl;
        c_b[pos] = gl * gl;
        c_win[pos] = make_int2(lo, hi - lo);
        if constexpr (DUAL) {
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const size_t o = (size_t)j + dd.ks * k;
            const double dg = dgl ? dgl[o] : 0.0, ds = dd.dS ? dd.dS[o] : 0.0;
            c_d[k * kBlock + pos] = ds * gl + s * dg;
            c_d[(2 + k) * kBlock + pos] = 2.0 * gl * dg;
            c_d[(4 + k) * kBlock + pos] = dd.dnu ? dd.dnu[o] : 0.0;
          }
        }
      } else {
        const double gd = gamma_d[j];
        c_nu[pos] = nu[j];
        c_a[pos] = S[j] * cSqrtLn2divSqrtPi / gd;
        c_b[pos] = kB / gd;
        if constexpr (kIsVoigt) c_y[pos] = y[j];
        c_win[pos] = make_int2(lo, hi - lo);  // hi >= lo for a hit
        if constexpr (DUAL) {  // a = S c / gamma_d, b = c' / gamma_d by the quotient rule, per LINE like the values
          const double a = c_a[pos], b = c_b[pos];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const size_t o = (size_t)j + dd.ks * k;
            const double dg = dd.dgd ? dd.dgd[o] : 0.0, ds = dd.dS ? dd.dS[o] : 0.0;
            c_d[k * kBlock + pos] = (ds * cSqrtLn2divSqrtPi - a * dg) / gd;
            c_d[(2 + k) * kBlock + pos] = -(b * dg) / gd;
            c_d[(4 + k) * kBlock + pos] = dd.dnu ? dd.dnu[o] : 0.0;
            if constexpr (kIsVoigt) c_d[(6 + k) * kBlock + pos] = dd.dy ? dd.dy[o] : 0.0;
          }
        }
      }
    }
    int nc = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) nc += wcount[w];
    nc = __builtin_amdgcn_readfirstlane(nc);  // workgroup-uniform: scalar loop control
    __syncthreads();
    // r5 (0.37 -> 0.40 of the vector peak, profiles/r05_voigt_ab.txt): the window as ONE LDS read and one unsigned compare
    // (r4: first point, last point and then the four doubles in three dependent round trips, each behind its own exec-masked
    // region); the evaluation is skipped only when the WHOLE wavefront lies outside the window; the quotient of the Humlicek
    // branch by the refined reciprocal.  Measured and NOT shipped: two / four grid points per thread (0.39 / 0.34: the two
    // evaluations of a thread do not overlap better than two wavefronts do, and the core workload loses its early exits), a
    // straight-line two-point Humlicek path, the strided range pass instead of the bisection for short line lists.
    const int gt = (gi < nGrid) ? gi : -1;  // a point past the end of the grid lies in no window: (unsigned)(-1 - lo) > any span
#ifndef MOM_VOIGT_DIAG_NOEVAL
    for (int c = 0; c < nc; ++c) {
      const int2 win = c_win[c];
      const double cn = c_nu[c], ca = c_a[c], cb = c_b[c];
      [[maybe_unused]] double cy = 0.0;
      if constexpr (kIsVoigt) cy = c_y[c];
      const bool in = (unsigned)(gt - win.x) <= (unsigned)win.y;
      if (__builtin_amdgcn_ballot_w64(in) == 0) continue;
      if constexpr (SHAPE == kDoppler) {
        // q = b (g - nu), e = exp(-ln 2 q^2): far from the line e underflows to 0.0 and every product below is 0.0 with it
        // (q^2 stays finite for any distance in cm^-1).  Dual run: d_k q = d_k b (g - nu) - b d_k nu (d_k b = -b d_k gamma_d / gamma_d),
        // d_k e = e (-2 ln 2 q d_k q), d_k sigma = d_k a e + a d_k e
        const double dist = gx - cn, q = cb * dist;
        const double e = exp(-cLn2 * (q * q));
        if (in) {
          acc = fma(ca, e, acc);
          if constexpr (DUAL) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const double dq = c_d[(2 + k) * kBlock + c] * dist - cb * c_d[(4 + k) * kBlock + c];
              dacc[k] += c_d[k * kBlock + c] * e + ca * (e * (-2.0 * cLn2 * q * dq));
            }
          }
        }
      } else if constexpr (SHAPE == kLorentz) {
        // D = pi (gamma_l^2 + (g - nu)^2), sigma = S gamma_l / D: the reference's operations in its order (one IEEE division, no
        // contraction).  Dual run: d_k D = pi (2 gamma_l d_k gamma_l - 2 (g - nu) d_k nu), d_k sigma = (d_k a - sigma d_k D) / D
#pragma clang fp contract(off)
        const double dist = gx - cn;
        const double D = cPi * (cb + dist * dist);
        const double sg = ca / D;
        if (in) {
          acc += sg;
          if constexpr (DUAL) {
            const double rD = 1.0 / D;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const double dD = cPi * (c_d[(2 + k) * kBlock + c] - 2.0 * dist * c_d[(4 + k) * kBlock + c]);
              dacc[k] += (c_d[k * kBlock + c] - sg * dD) * rD;
            }
          }
        }
      } else if constexpr (DUAL) {
        // x = b (g - nu): d_k x = d_k b (g - nu) - b d_k nu;  d_k sigma += d_k a Re w + a Re(w' (d_k x + i d_k y))
        const double dist = gx - cn;
        cplx dw;
        const double w = w_hw32_dual<SHAPE == kVoigt15>(cb * dist, cy, dw);
        if (in) {
          acc = fma(ca, w, acc);
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const double dx = c_d[(2 + k) * kBlock + c] * dist - cb * c_d[(4 + k) * kBlock + c];
            dacc[k] += c_d[k * kBlock + c] * w + ca * (dw.re * dx - dw.im * c_d[(6 + k) * kBlock + c]);
          }
        }
      } else {
        const double w = w_hw32_re<SHAPE == kVoigt15>(cb * (gx - cn), cy);
        if (in) acc = fma(ca, w, acc);   // acc += a w, one rounding as before
      }
    }
#else
    (void)gt;
    if (nc > 0) acc += c_a[nc - 1] + c_nu[0] + c_b[0] + (kIsVoigt ? c_y[0] : 0.0) + c_win[0].x;   // (diagnostic build: the setup without the evaluations)
#endif
    __syncthreads();
  }
  // accumulate: tau_abs[:, iz] += sigma * (vcd_dry[iz] * vmr)  (atmo_prof.jl:446), fused into the line-shape kernel
  // (separately rounded product and sum, like the host expression: no FMA contraction)
  if (gi < nGrid) {
#pragma clang fp contract(off)
    const double scaled = acc * factor;
    sigma[gi] = accumulate ? sigma[gi] + scaled : acc;
    if constexpr (DUAL) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        double *o = dd.dsigma + gi + dd.os * k;
        const double dscaled = dacc[k] * factor;
        *o = accumulate ? *o + dscaled : dacc[k];
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_voigt(int nLines, const double *__restrict__ nu,
                                                  const double *__restrict__ gamma_d, const double *__restrict__ y,
                                                  const double *__restrict__ S, const int *__restrict__ i0,
                                                  const int *__restrict__ i1, int nGrid,
                                                  const double *__restrict__ grid, double *__restrict__ sigma,
                                                  double factor, int accumulate, int sorted) {
  voigt_block<false, kVoigtSD>(nLines, nu, gamma_d, nullptr, y, S, i0, i1, nGrid, grid, sigma, factor, accumulate, sorted, VoigtDualArgs{},
                               nullptr);
}
__global__ void __launch_bounds__(kBlock) k_voigt_dual(int nLines, const double *__restrict__ nu,
                                                       const double *__restrict__ gamma_d, const double *__restrict__ y,
                                                       const double *__restrict__ S, const int *__restrict__ i0,
                                                       const int *__restrict__ i1, int nGrid,
                                                       const double *__restrict__ grid, double *__restrict__ sigma,
                                                       double factor, int accumulate, int sorted, VoigtDualArgs dd) {
  voigt_block<true, kVoigtSD>(nLines, nu, gamma_d, nullptr, y, S, i0, i1, nGrid, grid, sigma, factor, accumulate, sorted, dd, nullptr);
}

// All layers of a profile in ONE launch (blockIdx.y = layer): the per-line prefactors of layer z sit at [k][z][cap]
// (k = nu, gamma_d, y, S; the two window arrays likewise as ints in slot 4; gamma_l in slot 5), tau_abs[:, z] += sigma_z * factor[z]; whether the
// bisection applies is read from the layer's flag on the device (no host round trip between the two kernels).
__global__ void __launch_bounds__(kBlock) k_voigt_profile(int nLines, int Nz, size_t cap, const double *__restrict__ pf,
                                                          const int *__restrict__ win, int nGrid, const double *__restrict__ grid,
                                                          double *__restrict__ tau_abs, const double *__restrict__ factor,
                                                          const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  voigt_block<false, kVoigtSD>(nLines, pf + lz, pf + ks + lz, nullptr, pf + 2 * ks + lz, pf + 3 * ks + lz, win + lz, win + ks + lz, nGrid,
                               grid, tau_abs + (size_t)nGrid * z, factor[z], 1, unsorted[z] ? 0 : 1, VoigtDualArgs{}, nullptr);
}
// ... and its Dual run: the partials of layer z's prefactors at dpf[q][k][z][cap] (q = nu, gamma_d, y, S, gamma_l), dtau_abs [nGrid, Nz, 2]
__global__ void __launch_bounds__(kBlock) k_voigt_profile_dual(int nLines, int Nz, size_t cap, const double *__restrict__ pf,
                                                               const double *__restrict__ dpf, const int *__restrict__ win, int nGrid,
                                                               const double *__restrict__ grid, double *__restrict__ tau_abs,
                                                               double *__restrict__ dtau_abs, const double *__restrict__ factor,
                                                               const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  const VoigtDualArgs dd = {dpf + lz, dpf + 2 * ks + lz, dpf + 4 * ks + lz, dpf + 6 * ks + lz, ks, dtau_abs + (size_t)nGrid * z,
                            (size_t)nGrid * Nz};
  voigt_block<true, kVoigtSD>(nLines, pf + lz, pf + ks + lz, nullptr, pf + 2 * ks + lz, pf + 3 * ks + lz, win + lz, win + ks + lz, nGrid,
                              grid, tau_abs + (size_t)nGrid * z, factor[z], 1, unsorted[z] ? 0 : 1, dd, nullptr);
}

// The other three shapes: the same four kernels with gamma_l (and, Dual run, its partials) as one more argument.  The
// Voigt / HW32SD kernels above keep their argument lists, so the default model runs the code it always ran.
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_lineshape(int nLines, const double *__restrict__ nu, const double *__restrict__ gamma_d,
                                                      const double *__restrict__ gamma_l, const double *__restrict__ y,
                                                      const double *__restrict__ S, const int *__restrict__ i0,
                                                      const int *__restrict__ i1, int nGrid, const double *__restrict__ grid,
                                                      double *__restrict__ sigma, double factor, int accumulate, int sorted) {
  voigt_block<false, SHAPE>(nLines, nu, gamma_d, gamma_l, y, S, i0, i1, nGrid, grid, sigma, factor, accumulate, sorted, VoigtDualArgs{},
                            nullptr);
}
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_lineshape_dual(int nLines, const double *__restrict__ nu, const double *__restrict__ gamma_d,
                                                           const double *__restrict__ gamma_l, const double *__restrict__ y,
                                                           const double *__restrict__ S, const int *__restrict__ i0,
                                                           const int *__restrict__ i1, int nGrid, const double *__restrict__ grid,
                                                           double *__restrict__ sigma, double factor, int accumulate, int sorted,
                                                           VoigtDualArgs dd, const double *__restrict__ dgl) {
  voigt_block<true, SHAPE>(nLines, nu, gamma_d, gamma_l, y, S, i0, i1, nGrid, grid, sigma, factor, accumulate, sorted, dd, dgl);
}
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_lineshape_profile(int nLines, int Nz, size_t cap, const double *__restrict__ pf,
                                                              const int *__restrict__ win, int nGrid, const double *__restrict__ grid,
                                                              double *__restrict__ tau_abs, const double *__restrict__ factor,
                                                              const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  voigt_block<false, SHAPE>(nLines, pf + lz, pf + ks + lz, pf + 5 * ks + lz, pf + 2 * ks + lz, pf + 3 * ks + lz, win + lz, win + ks + lz,
                            nGrid, grid, tau_abs + (size_t)nGrid * z, factor[z], 1, unsorted[z] ? 0 : 1, VoigtDualArgs{}, nullptr);
}
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_lineshape_profile_dual(int nLines, int Nz, size_t cap, const double *__restrict__ pf,
                                                                   const double *__restrict__ dpf, const int *__restrict__ win, int nGrid,
                                                                   const double *__restrict__ grid, double *__restrict__ tau_abs,
                                                                   double *__restrict__ dtau_abs, const double *__restrict__ factor,
                                                                   const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  const VoigtDualArgs dd = {dpf + lz, dpf + 2 * ks + lz, dpf + 4 * ks + lz, dpf + 6 * ks + lz, ks, dtau_abs + (size_t)nGrid * z,
                            (size_t)nGrid * Nz};
  voigt_block<true, SHAPE>(nLines, pf + lz, pf + ks + lz, pf + 5 * ks + lz, pf + 2 * ks + lz, pf + 3 * ks + lz, win + lz, win + ks + lz,
                           nGrid, grid, tau_abs + (size_t)nGrid * z, factor[z], 1, unsorted[z] ? 0 : 1, dd, dpf + 8 * ks + lz);
}

// STMT(shape) for one of the three shapes that are not the default
#define MOM_SHAPE_SWITCH(shape, STMT)      \
  switch (shape) {                         \
    case kVoigt15: STMT(kVoigt15); break;  \
    case kDoppler: STMT(kDoppler); break;  \
    default: STMT(kLorentz); break;        \
  }

thread_local double v_last_ms = 0.0;

}  // namespace

// one launch for all lines on `st` (device pointers); used by mom_voigt_xsec below and by the handle-level
// mom_voigt_tau_abs (mom_optics.hip), which accumulates straight into the resident tau_abs table
// ---------------------------------------------------------------------------------------------------------------------
// Per-line prefactors of compute_absorption_cross_section (compute_absorption_cross_section.jl:73-107) on the device, from
// ONE resident HITRAN table per absorber: pressure shift (:79), Lorentz half width (:82-84), Doppler half width (:87-88),
// y (:91), the temperature correction of the strength with the TIPS-2017 partition-sum ratio qoft! (:95-101, :197-214:
// cubic spline of the isotopologue's table, evaluated at T_ref and T) and the grid window of the line (:104-107: linear
// interpolation grid -> index with the constant fill values 1 / n outside the grid, rounded half-to-even).  One thread per line; per layer only (p, T, vmr, wing) are
// kernel arguments.  Same expression order as the host route (absorption.line_prefactors); exp / pow come from the
// device math library, so the two routes agree to a few ulp, not bitwise.
// ---------------------------------------------------------------------------------------------------------------------
// searchsortedlast restricted to [0, n - 2]: the interval lo with a[lo] <= x < a[lo + 1] (lo = 0 below a[0], n - 2 from a[n - 1]
// on) of an ascending table a[0 .. n - 1].  r5: a guess from the mean spacing of a[first .. n - 1] and a walk of at most three
// steps replace the bisection wherever the table is (nearly) uniform -- the wavenumber grid always, the TIPS temperature
// knots from the second one on: two dependent memory latencies instead of log2(n).  k_line_prefactors_profile ran 76 dependent
// loads per thread (four window indices on a 22 801-point grid, two spline intervals on 251 knots): 23 us of the operating
// point's 132 us.  Any other table falls through to the bisection; the interval, hence every value computed from it, is the
// same either way.
__device__ __forceinline__ int locate_interval(const double *a, int n, double x, int first) {
  if (n < 2) return 0;
  const double a0 = a[first], a1 = a[n - 1];
  if (n - 1 > first && a1 > a0) {
    const double g = (x - a0) * ((double)(n - 1 - first) / (a1 - a0));
    int lo = first + (int)fmin(fmax(g, 0.0), (double)(n - 2 - first));
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      if (a[lo] > x) { if (lo == 0) break; --lo; }
      else if (a[lo + 1] <= x) { if (lo == n - 2) break; ++lo; }
      else break;
    }
    const bool below = (lo == 0 && x < a[0]), above = (lo == n - 2 && a[n - 1] <= x);
    if (below || above || (a[lo] <= x && x < a[lo + 1])) return lo;
  }
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}
// dq (optional): the derivative of the same piece with respect to x -- I + C + D differentiated term by term
__device__ __forceinline__ double spline_eval(const double *t, const double *u, const double *z, int n1, double x, double *dq = nullptr) {
  // DataInterpolations.CubicSpline evaluation (restated in absorption.CubicSpline.__call__): interval by searchsortedlast
  const int i = min(max(locate_interval(t, n1 + 1, x, n1 >= 2 ? 1 : 0), 0), n1 - 1);  // knots t[0 .. n1]
  // the tables are Float32 (TIPS_2017.nc); products of two table entries are Float32 operations, as in the reference's
  // (and the host route's) evaluation -- only the terms that involve the Float64 argument x are Float64
  const float hf = (float)t[i + 1] - (float)t[i];
  const float cu = (float)u[i + 1] / hf - (float)z[i + 1] * hf / 6.0f;
  const float du = (float)u[i] / hf - (float)z[i] * hf / 6.0f;
  const double h6 = (double)(6.0f * hf);
  const double a = t[i + 1] - x, b = x - t[i];
  const double I = z[i] * (a * a * a) / h6 + z[i + 1] * (b * b * b) / h6;
  const double C = (double)cu * b;
  const double D = (double)du * a;
  if (dq) *dq = (z[i + 1] * (3.0 * (b * b)) / h6 - z[i] * (3.0 * (a * a)) / h6) + (double)cu - (double)du;
  return I + C + D;
}
__device__ __forceinline__ double interp_index(const double *grid, int n, double x, double fill) {
  // LinearInterpolation(grid, 1:n, extrapolation_bc = fill) (compute_absorption_cross_section.jl:60-61): linear inside the
  // grid, the CONSTANT `fill` on BOTH sides outside it (fill = 1 for the window start, n for the stop); grid ascending
  if (n == 1) return 1.0;
  if (x < grid[0] || x > grid[n - 1]) return fill;
  if (x == grid[n - 1]) return (double)n;
  const int lo = locate_interval(grid, n, x, 0);
  const double slope = 1.0 / (grid[lo + 1] - grid[lo]);
  return slope * (x - grid[lo]) + (double)(lo + 1);
}
// Dual run: where the partials of nu, gamma_d, y, S, gamma_l of one layer go (partial k of line j at p[j + ks k]; k = 0 pressure,
// 1 temperature) and d cgd / dT
struct LineDualOut {
  double *dnu, *dgd, *dy, *dS, *dgl;
  size_t ks;
  double dcgd;
};
// DUAL: the same statements on ForwardDiff.Dual numbers -- every value below is formed exactly as in the value run, the
// partials follow each statement by its rule; windows and the sortedness flag come from the values
template <bool DUAL>
__device__ __forceinline__ void line_prefactors_one(int j, const MomLineTable &tb, int nGrid, const double *grid, double p, double T,
                                                    double vmr, double wing, double cgd, double *nu, double *gd, double *yy, double *SS,
                                                    double *gll, int *i0, int *i1, int *unsorted, const LineDualOut dd) {
#pragma clang fp contract(off)
  if (j >= tb.nLines) return;
  const double p_ref = 1013.25, t_ref = 296.0, c2 = 1.4387769, cLn2 = 0.6931471805599;
  const double nu0 = tb.nu0[j], E = tb.E[j];
  const double v = nu0 + p / p_ref * tb.d_air[j];
  const double tpow = pow(t_ref / T, tb.n_air[j]);
  const double gl = (tb.g_air[j] * (1 - vmr) * p / p_ref + tb.g_self[j] * vmr * p / p_ref) * tpow;
  const double g = cgd * nu0 / tb.sqw[j];
  double S = tb.S0[j];
  [[maybe_unused]] double dS_T = 0.0;
  if (E != -1.0) {
    const int is = tb.iso[j];
    const double *t = tb.tT + (size_t)is * tb.nTmax, *u = tb.tQ + (size_t)is * tb.nTmax, *z = tb.tZ + (size_t)is * tb.nTmax;
    const int n1 = tb.nT[is] - 1;
    double dQ = 0.0;
    const double Qref = spline_eval(t, u, z, n1, t_ref), Q = spline_eval(t, u, z, n1, T, DUAL ? &dQ : nullptr);
    const double rate = Qref / Q;
    const double e1 = exp(c2 * E * (1 / t_ref - 1 / T)), ex2 = exp(-c2 * nu0 / T), e2 = 1 - ex2, e3 = 1 - exp(-c2 * nu0 / t_ref);
    const double corr = rate * e1 * e2 / e3;
    if constexpr (DUAL) {  // S0 rate e1 e2 / e3: d rate = -Q(t_ref) Q'(T) / Q(T)^2, d e1 = e1 c2 E'' / T^2, d e2 = -exp(-c2 nu0 / T) c2 nu0 / T^2
      const double drate = -(Qref / (Q * Q)) * dQ, de1 = e1 * (c2 * E * (1 / (T * T))), de2 = -(ex2 * (c2 * nu0 / (T * T)));
      const double r1 = rate * e1, dr1 = drate * e1 + rate * de1;
      dS_T = S * ((dr1 * e2 + r1 * de2) / e3);
    }
    S = S * corr;
  }
  nu[j] = v;
  gd[j] = g;
  const double ynum = sqrt(cLn2) * gl;
  yy[j] = ynum / g;
  SS[j] = S;
  gll[j] = gl;   // line_shape! takes gamma_l next to y (:118-124): the fifth prefactor, read by the Lorentz shape
  if constexpr (DUAL) {
    // nu = nu0 + p / p_ref delta;  gamma_l = lin(p) (t_ref / T)^n: d/dp = the bracket times the power (no gamma_l / p),
    // d/dT = lin n (t_ref / T)^(n - 1) (-t_ref / T^2);  gamma_d = cgd(T) nu0 / sqrt(w);  y = sqrt(ln 2) gamma_l / gamma_d
    const double n = tb.n_air[j];
    const double dgl_p = (tb.g_air[j] * (1 - vmr) / p_ref + tb.g_self[j] * vmr / p_ref) * tpow;
    const double lin = tb.g_air[j] * (1 - vmr) * p / p_ref + tb.g_self[j] * vmr * p / p_ref;
    const double dgl_T = lin * (n * pow(t_ref / T, n - 1) * (-(t_ref / (T * T))));
    const double dg_T = dd.dcgd * nu0 / tb.sqw[j];
    dd.dnu[j] = (1 / p_ref) * tb.d_air[j];
    dd.dnu[j + dd.ks] = 0.0;
    dd.dgd[j] = 0.0;
    dd.dgd[j + dd.ks] = dg_T;
    dd.dy[j] = sqrt(cLn2) * dgl_p * (1 / g);
    dd.dy[j + dd.ks] = sqrt(cLn2) * dgl_T * (1 / g) + dg_T * (-(ynum / (g * g)));
    dd.dS[j] = 0.0;
    dd.dS[j + dd.ks] = dS_T;
    dd.dgl[j] = dgl_p;
    dd.dgl[j + dd.ks] = dgl_T;
  }
  const int a = (int)rint(interp_index(grid, nGrid, v - wing, 1.0)), b = (int)rint(interp_index(grid, nGrid, v + wing, (double)nGrid));
  i0[j] = a;
  i1[j] = b;
  if (j > 0) {  // does the Voigt kernel's bisection apply?  (window starts and stops non-decreasing in the line index)
    const double vp = tb.nu0[j - 1] + p / p_ref * tb.d_air[j - 1];
    const int ap = (int)rint(interp_index(grid, nGrid, vp - wing, 1.0)), bp = (int)rint(interp_index(grid, nGrid, vp + wing, (double)nGrid));
    if (a < ap || b < bp) atomicOr(unsorted, 1);
  }
}
__global__ void k_line_prefactors(MomLineTable tb, int nGrid, const double *grid, double p, double T, double vmr, double wing,
                                  double cgd, double *nu, double *gd, double *yy, double *SS, double *gll, int *i0, int *i1,
                                  int *unsorted) {
  line_prefactors_one<false>(blockIdx.x * blockDim.x + threadIdx.x, tb, nGrid, grid, p, T, vmr, wing, cgd, nu, gd, yy, SS, gll, i0, i1,
                             unsorted, LineDualOut{});
}
// blockIdx.y = layer; prm = [p | T | cgd][Nz]; outputs at [k][z][cap], gamma_l at k = 5 (see k_voigt_profile)
__global__ void k_line_prefactors_profile(MomLineTable tb, int Nz, size_t cap, int nGrid, const double *grid, const double *prm,
                                          double vmr, double wing, double *pf, int *win, int *unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  line_prefactors_one<false>(blockIdx.x * blockDim.x + threadIdx.x, tb, nGrid, grid, prm[z], prm[Nz + z], vmr, wing, prm[2 * Nz + z], pf + lz,
                             pf + ks + lz, pf + 2 * ks + lz, pf + 3 * ks + lz, pf + 5 * ks + lz, win + lz, win + ks + lz, unsorted + z,
                             LineDualOut{});
}
// Dual run: prm = [p | T | cgd | factor | d cgd / dT][Nz]; partials at dpf[q][k][z][cap], q = 0 .. 4 (see k_voigt_profile_dual)
__global__ void k_line_prefactors_profile_dual(MomLineTable tb, int Nz, size_t cap, int nGrid, const double *grid, const double *prm,
                                               double vmr, double wing, double *pf, double *dpf, int *win, int *unsorted) {
  const int z = blockIdx.y;
  const size_t lz = (size_t)z * cap, ks = (size_t)Nz * cap;
  const LineDualOut dd = {dpf + lz, dpf + 2 * ks + lz, dpf + 4 * ks + lz, dpf + 6 * ks + lz, dpf + 8 * ks + lz, ks, prm[4 * Nz + z]};
  line_prefactors_one<true>(blockIdx.x * blockDim.x + threadIdx.x, tb, nGrid, grid, prm[z], prm[Nz + z], vmr, wing, prm[2 * Nz + z], pf + lz,
                            pf + ks + lz, pf + 2 * ks + lz, pf + 3 * ks + lz, pf + 5 * ks + lz, win + lz, win + ks + lz, unsorted + z, dd);
}
hipError_t mom_voigt_profile_launch(hipStream_t st, int shape, const MomLineTable &tb, int Nz, size_t cap, int nGrid, const double *grid,
                                    const double *prm, double vmr, double wing, double *pf, int *win, int *unsorted, double *tau_abs,
                                    const double *factor) {
  if (tb.nLines <= 0 || Nz <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_line_prefactors_profile, dim3((tb.nLines + 255) / 256, Nz), dim3(256), 0, st, tb, Nz, cap, nGrid, grid, prm, vmr,
                     wing, pf, win, unsorted);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 blocks((nGrid + kBlock - 1) / kBlock, Nz);
#define MOM_LAUNCH(SH) \
  hipLaunchKernelGGL(k_lineshape_profile<SH>, blocks, dim3(kBlock), 0, st, tb.nLines, Nz, cap, pf, win, nGrid, grid, tau_abs, factor, unsorted)
  if (shape == kVoigtSD)
    hipLaunchKernelGGL(k_voigt_profile, blocks, dim3(kBlock), 0, st, tb.nLines, Nz, cap, pf, win, nGrid, grid, tau_abs, factor, unsorted);
  else
    MOM_SHAPE_SWITCH(shape, MOM_LAUNCH)
#undef MOM_LAUNCH
  return hipGetLastError();
}
hipError_t mom_voigt_profile_dual_launch(hipStream_t st, int shape, const MomLineTable &tb, int Nz, size_t cap, int nGrid, const double *grid,
                                         const double *prm, double vmr, double wing, double *pf, double *dpf, int *win, int *unsorted,
                                         double *tau_abs, double *dtau_abs, const double *factor) {
  if (tb.nLines <= 0 || Nz <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_line_prefactors_profile_dual, dim3((tb.nLines + 255) / 256, Nz), dim3(256), 0, st, tb, Nz, cap, nGrid, grid, prm,
                     vmr, wing, pf, dpf, win, unsorted);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 blocks((nGrid + kBlock - 1) / kBlock, Nz);
#define MOM_LAUNCH(SH)                                                                                                                \
  hipLaunchKernelGGL(k_lineshape_profile_dual<SH>, blocks, dim3(kBlock), 0, st, tb.nLines, Nz, cap, pf, dpf, win, nGrid, grid, tau_abs, \
                     dtau_abs, factor, unsorted)
  if (shape == kVoigtSD)
    hipLaunchKernelGGL(k_voigt_profile_dual, blocks, dim3(kBlock), 0, st, tb.nLines, Nz, cap, pf, dpf, win, nGrid, grid, tau_abs, dtau_abs,
                       factor, unsorted);
  else
    MOM_SHAPE_SWITCH(shape, MOM_LAUNCH)
#undef MOM_LAUNCH
  return hipGetLastError();
}
hipError_t mom_line_prefactors_launch(hipStream_t st, const MomLineTable &tb, int nGrid, const double *grid, double p, double T,
                                      double vmr, double wing, double cgd, double *nu, double *gd, double *y, double *S, double *gl,
                                      int *i0, int *i1, int *unsorted) {
  if (tb.nLines <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_line_prefactors, dim3((tb.nLines + 255) / 256), dim3(256), 0, st, tb, nGrid, grid, p, T, vmr, wing, cgd, nu,
                     gd, y, S, gl, i0, i1, unsorted);
  return hipGetLastError();
}

hipError_t mom_voigt_launch(hipStream_t st, int shape, int nLines, const double *nu, const double *gamma_d, const double *gamma_l,
                            const double *y, const double *S, const int *i0, const int *i1, int nGrid, const double *grid, double *out,
                            double factor, int accumulate, int sorted) {
  const dim3 blocks((nGrid + kBlock - 1) / kBlock);
#define MOM_LAUNCH(SH)                                                                                                            \
  hipLaunchKernelGGL(k_lineshape<SH>, blocks, dim3(kBlock), 0, st, nLines, nu, gamma_d, gamma_l, y, S, i0, i1, nGrid, grid, out, factor, \
                     accumulate, sorted)
  if (shape == kVoigtSD)
    hipLaunchKernelGGL(k_voigt, blocks, dim3(kBlock), 0, st, nLines, nu, gamma_d, y, S, i0, i1, nGrid, grid, out, factor, accumulate, sorted);
  else
    MOM_SHAPE_SWITCH(shape, MOM_LAUNCH)
#undef MOM_LAUNCH
  return hipGetLastError();
}

hipError_t mom_voigt_dual_launch(hipStream_t st, int shape, int nLines, const double *nu, const double *gamma_d, const double *gamma_l,
                                 const double *y, const double *S, const int *i0, const int *i1, int nGrid, const double *grid,
                                 double *out, double factor, int accumulate, int sorted, const double *dnu, const double *dgd,
                                 const double *dgl, const double *dy, const double *dS, size_t ks, double *dout, size_t os) {
  const dim3 blocks((nGrid + kBlock - 1) / kBlock);
  const VoigtDualArgs dd = {dnu, dgd, dy, dS, ks, dout, os};
#define MOM_LAUNCH(SH)                                                                                                                 \
  hipLaunchKernelGGL(k_lineshape_dual<SH>, blocks, dim3(kBlock), 0, st, nLines, nu, gamma_d, gamma_l, y, S, i0, i1, nGrid, grid, out, factor, \
                     accumulate, sorted, dd, dgl)
  if (shape == kVoigtSD)
    hipLaunchKernelGGL(k_voigt_dual, blocks, dim3(kBlock), 0, st, nLines, nu, gamma_d, y, S, i0, i1, nGrid, grid, out, factor, accumulate,
                       sorted, dd);
  else
    MOM_SHAPE_SWITCH(shape, MOM_LAUNCH)
#undef MOM_LAUNCH
  return hipGetLastError();
}

#define VCHK(call)                                                                                     \
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

namespace {
// mom_voigt_xsec / mom_lineshape_xsec (dsigma = nullptr: the value kernel) and their Dual runs (dpart: dnu, dgamma_d, dy, dS,
// dgamma_l, each [nLines, 2] or null = zeros); line[] = nu, gamma_d, y, S, gamma_l, of which the shape's broadening reads some (the
// others may be null); `fn` is the entry point's name in the error texts
int lineshape_xsec_run(const char *fn, int device, int shape, int nLines, const double *const *line, const double *const *dpart,
                       const int *ind_start, const int *ind_stop, int nGrid, const double *grid, double *sigma, double *dsigma) {
  char buf[192];
  const bool dual = dsigma != nullptr;
  bool lines_ok = ind_start && ind_stop;
  for (int k = 0; k < 5; ++k) lines_ok = lines_ok && (line[k] || !mom_shape_reads(shape, k));
  if (nLines < 0 || nGrid <= 0 || !grid || !sigma || (nLines > 0 && !lines_ok)) {
    snprintf(buf, sizeof buf, "%s: bad argument (null pointer or non-positive size)", fn);
    mom_set_global_error(buf);
    return MOM_EINVAL;
  }
  int sorted = 1;  // window starts and stops non-decreasing: the kernel finds a block's lines by bisection
  for (int j = 1; j < nLines; ++j)
    if (ind_start[j] < ind_start[j - 1] || ind_stop[j] < ind_stop[j - 1]) { sorted = 0; break; }
  for (int j = 0; j < nLines; ++j)
    if (ind_start[j] < 1 || ind_stop[j] > nGrid) {  // empty windows (start > stop) are allowed
      snprintf(buf, sizeof buf, "%s: line %d: window [%d, %d] outside the grid 1..%d", fn, j + 1, ind_start[j], ind_stop[j], nGrid);
      mom_set_global_error(buf);
      return MOM_EINVAL;
    }
  int rc = MOM_OK;
  // one device allocation (lines | grid | sigma | windows; Dual run: the line partials and dsigma in front of the windows) and
  // one pinned-free staging copy per array on a private stream; callers that evaluate many layers should use the
  // handle-level mom_voigt_tau_abs, which keeps all of this resident
  const size_t lb = (size_t)(nLines > 0 ? nLines : 1);
  const size_t dual_doubles = dual ? 10 * lb + 2 * (size_t)nGrid : 0;
  const size_t bytes = (5 * lb + 2 * (size_t)nGrid + dual_doubles) * sizeof(double) + 2 * lb * sizeof(int);
  char *base = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    snprintf(buf, sizeof buf, "%s: no HIP device available", fn);
    mom_set_global_error(buf);
    return MOM_EHIP;
  }
  if (device < 0 || device >= ndev) {
    snprintf(buf, sizeof buf, "%s: device index out of range", fn);
    mom_set_global_error(buf);
    return MOM_EINVAL;
  }
  VCHK(hipSetDevice(device));
  VCHK(hipStreamCreate(&st));
  VCHK(hipMalloc((void **)&base, bytes));
  {
    double *d_line = (double *)base, *d_grid = d_line + 5 * lb, *d_sig = d_grid + nGrid;
    double *d_dline = d_sig + nGrid, *d_dsig = d_dline + (dual ? 10 * lb : 0);   // Dual run only: [q][k][lb], [nGrid, 2]
    int *d_win = (int *)(d_sig + nGrid + dual_doubles);
    for (int k = 0; k < 5; ++k)   // an array the shape does not read stays as allocated: the kernel never loads it
      if (nLines && line[k] && mom_shape_reads(shape, k))
        VCHK(hipMemcpyAsync(d_line + k * lb, line[k], (size_t)nLines * sizeof(double), hipMemcpyHostToDevice, st));
    if (nLines) {
      VCHK(hipMemcpyAsync(d_win, ind_start, (size_t)nLines * sizeof(int), hipMemcpyHostToDevice, st));
      VCHK(hipMemcpyAsync(d_win + lb, ind_stop, (size_t)nLines * sizeof(int), hipMemcpyHostToDevice, st));
    }
    VCHK(hipMemcpyAsync(d_grid, grid, (size_t)nGrid * sizeof(double), hipMemcpyHostToDevice, st));
    const double *d_part[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int q = 0; q < 5 && dual && nLines; ++q) {
      if (!dpart[q] || !mom_shape_reads(shape, q)) continue;
      for (int k = 0; k < 2; ++k)   // host [nLines, 2] column-major -> [k][lb]
        VCHK(hipMemcpyAsync(d_dline + (2 * q + k) * lb, dpart[q] + (size_t)nLines * k, (size_t)nLines * sizeof(double),
                            hipMemcpyHostToDevice, st));
      d_part[q] = d_dline + 2 * q * lb;
    }
    VCHK(hipEventCreate(&e0));
    VCHK(hipEventCreate(&e1));
    VCHK(hipEventRecord(e0, st));
    if (dual)
      VCHK(mom_voigt_dual_launch(st, shape, nLines, d_line, d_line + lb, d_line + 4 * lb, d_line + 2 * lb, d_line + 3 * lb, d_win,
                                 d_win + lb, nGrid, d_grid, d_sig, 1.0, 0, sorted, d_part[0], d_part[1], d_part[4], d_part[2], d_part[3],
                                 lb, d_dsig, (size_t)nGrid));
    else
      VCHK(mom_voigt_launch(st, shape, nLines, d_line, d_line + lb, d_line + 4 * lb, d_line + 2 * lb, d_line + 3 * lb, d_win, d_win + lb,
                            nGrid, d_grid, d_sig, 1.0, 0, sorted));
    VCHK(hipEventRecord(e1, st));
    VCHK(hipMemcpyAsync(sigma, d_sig, (size_t)nGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dual) VCHK(hipMemcpyAsync(dsigma, d_dsig, 2 * (size_t)nGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    VCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    VCHK(hipEventElapsedTime(&ms, e0, e1));
    v_last_ms = ms;
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (base) (void)hipFree(base);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}
}  // namespace

extern "C" int mom_voigt_xsec(int device, int nLines, const double *nu, const double *gamma_d, const double *y,
                              const double *S, const int *ind_start, const int *ind_stop, int nGrid, const double *grid,
                              double *sigma) {
  const double *line[5] = {nu, gamma_d, y, S, nullptr};
  return lineshape_xsec_run("mom_voigt_xsec", device, 0, nLines, line, nullptr, ind_start, ind_stop, nGrid, grid, sigma, nullptr);
}

extern "C" int mom_voigt_xsec_dual(int device, int nLines, const double *nu, const double *gamma_d, const double *y, const double *S,
                                   const double *dnu, const double *dgamma_d, const double *dy, const double *dS,
                                   const int *ind_start, const int *ind_stop, int nGrid, const double *grid, double *sigma,
                                   double *dsigma) {
  if (!dsigma) {
    mom_set_global_error("mom_voigt_xsec_dual: bad argument (null pointer or non-positive size)");
    return MOM_EINVAL;
  }
  const double *line[5] = {nu, gamma_d, y, S, nullptr}, *dpart[5] = {dnu, dgamma_d, dy, dS, nullptr};
  return lineshape_xsec_run("mom_voigt_xsec_dual", device, 0, nLines, line, dpart, ind_start, ind_stop, nGrid, grid, sigma, dsigma);
}

// line_shape!(A, grid, nu, gamma_d, gamma_l, y, S, broadening, CEF) (compute_absorption_cross_section.jl:167-183) summed over the
// lines: mom_voigt_xsec for any absorption model
extern "C" int mom_lineshape_xsec(int device, int broadening, int cef, int nLines, const double *nu, const double *gamma_d,
                                  const double *gamma_l, const double *y, const double *S, const int *ind_start, const int *ind_stop,
                                  int nGrid, const double *grid, double *sigma) {
  std::string err;
  const int shape = mom_line_shape("mom_lineshape_xsec", broadening, cef, &err);
  if (shape < 0) {
    mom_set_global_error(err.c_str());
    return MOM_EINVAL;
  }
  const double *line[5] = {nu, gamma_d, y, S, gamma_l};
  return lineshape_xsec_run("mom_lineshape_xsec", device, shape, nLines, line, nullptr, ind_start, ind_stop, nGrid, grid, sigma, nullptr);
}

extern "C" int mom_lineshape_xsec_dual(int device, int broadening, int cef, int nLines, const double *nu, const double *gamma_d,
                                       const double *gamma_l, const double *y, const double *S, const double *dnu,
                                       const double *dgamma_d, const double *dgamma_l, const double *dy, const double *dS,
                                       const int *ind_start, const int *ind_stop, int nGrid, const double *grid, double *sigma,
                                       double *dsigma) {
  std::string err;
  const int shape = mom_line_shape("mom_lineshape_xsec_dual", broadening, cef, &err);
  if (shape < 0 || !dsigma) {
    mom_set_global_error(shape < 0 ? err.c_str() : "mom_lineshape_xsec_dual: bad argument (null pointer or non-positive size)");
    return MOM_EINVAL;
  }
  const double *line[5] = {nu, gamma_d, y, S, gamma_l}, *dpart[5] = {dnu, dgamma_d, dy, dS, dgamma_l};
  return lineshape_xsec_run("mom_lineshape_xsec_dual", device, shape, nLines, line, dpart, ind_start, ind_stop, nGrid, grid, sigma,
                            dsigma);
}

// GPU time of the line-shape launch of the last mom_voigt_xsec / mom_lineshape_xsec call (or Dual run) on this thread (HIP events), ms.
extern "C" double mom_voigt_last_kernel_ms(void) { return v_last_ms; }
