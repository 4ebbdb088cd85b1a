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

// The absorption model (HitranModel.broadening x HitranModel.CEF) as the compile-time shape of voigt_block.  It decides what is
// staged per candidate line, what is evaluated per (line, grid point) and which partials the Dual run stages; the candidate search,
// the ordered compaction, the accumulation order, the window compare and the tau_abs epilogue are the same for all four.
//   kVoigtSD, kVoigt15  a = S c / gamma_d, b = c' / gamma_d, y:  sigma = a Re w(b (g - nu) + i y)           (:179-183)
//   kDoppler            a = S c / gamma_d, b = 1 / gamma_d:      sigma = a exp(-ln 2 (b (g - nu))^2)        (:167-171)
//   kLorentz            a = S gamma_l, b = gamma_l^2:            sigma = a / (pi (b + (g - nu)^2))          (:173-177)
// MOM_BROADENING_* / MOM_CEF_* -> shape: mom_line_shape (mom_host.hpp)
enum LineShape : int { kVoigtSD = 0, kVoigt15 = 1, kDoppler = 2, kLorentz = 3 };

// DUAL = false is the value kernel; DUAL = true shares its candidate search and ordered compaction, stages d a, d b, d nu, d y
// (two each) next to a, b, nu, y and sums the two partials of every grid point in the same ascending line order: dd holds the
// partials of the prefactors (MomLinePartials, mom_host.hpp), the output partials go to dsigma[g + os k].  gamma_l and its partials
// are read by kLorentz only, gamma_d by the other three, y by the two Voigt shapes.
template <bool DUAL, int SHAPE>
__device__ __forceinline__ void voigt_block(int nLines, const double *__restrict__ nu,
                                            const double *__restrict__ gamma_d, const double *__restrict__ gamma_l,
                                            const double *__restrict__ y,
                                            const double *__restrict__ S, const int *__restrict__ i0,
                                            const int *__restrict__ i1, int nGrid,
                                            const double *__restrict__ grid, double *__restrict__ sigma,
                                            double factor, int accumulate, int sorted, const MomLinePartials dd,
                                            double *__restrict__ dsigma, size_t os) {
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
            const double dg = dd.dgamma_l ? dd.dgamma_l[o] : 0.0, ds = dd.dS ? dd.dS[o] : 0.0;
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
            const double dg = dd.dgamma_d ? dd.dgamma_d[o] : 0.0, ds = dd.dS ? dd.dS[o] : 0.0;
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
        double *o = dsigma + gi + os * k;
        const double dscaled = dacc[k] * factor;
        *o = accumulate ? *o + dscaled : dacc[k];
      }
    }
  }
}

// The four line-shape kernels, each instantiated for the four shapes (the default model is the kVoigtSD instantiation).  A view
// is unpacked into voigt_block's __restrict__ parameters: the qualifier is not honoured on struct members.
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_voigt(int nLines, MomLineView ln, int nGrid, const double *__restrict__ grid,
                                                  double *__restrict__ sigma, double factor, int accumulate, int sorted) {
  voigt_block<false, SHAPE>(nLines, ln.nu, ln.gamma_d, ln.gamma_l, ln.y, ln.S, ln.i0, ln.i1, nGrid, grid, sigma, factor, accumulate, sorted,
                            MomLinePartials{}, nullptr, 0);
}
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_voigt_dual(int nLines, MomLineView ln, MomLinePartials dd, int nGrid,
                                                       const double *__restrict__ grid, double *__restrict__ sigma,
                                                       double *__restrict__ dsigma, size_t os, double factor, int accumulate, int sorted) {
  voigt_block<true, SHAPE>(nLines, ln.nu, ln.gamma_d, ln.gamma_l, ln.y, ln.S, ln.i0, ln.i1, nGrid, grid, sigma, factor, accumulate, sorted, dd,
                           dsigma, os);
}
// All layers of a profile in ONE launch (blockIdx.y = layer): tau_abs[:, z] += sigma_z * factor[z]; whether the bisection applies is
// read from the layer's flag on the device (no host round trip between the two kernels).
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_voigt_profile(int nLines, MomLineBlock pf, int nGrid, const double *__restrict__ grid,
                                                          double *__restrict__ tau_abs, const double *__restrict__ factor,
                                                          const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const MomLineView ln = pf.layer(z);
  voigt_block<false, SHAPE>(nLines, ln.nu, ln.gamma_d, ln.gamma_l, ln.y, ln.S, ln.i0, ln.i1, nGrid, grid, tau_abs + (size_t)nGrid * z,
                            factor[z], 1, unsorted[z] ? 0 : 1, MomLinePartials{}, nullptr, 0);
}
// ... and its Dual run: dtau_abs [nGrid, nz, 2]
template <int SHAPE>
__global__ void __launch_bounds__(kBlock) k_voigt_profile_dual(int nLines, MomLineBlock pf, MomLinePartialBlock dpf, int nGrid,
                                                               const double *__restrict__ grid, double *__restrict__ tau_abs,
                                                               double *__restrict__ dtau_abs, const double *__restrict__ factor,
                                                               const int *__restrict__ unsorted) {
  const int z = blockIdx.y;
  const MomLineView ln = pf.layer(z);
  voigt_block<true, SHAPE>(nLines, ln.nu, ln.gamma_d, ln.gamma_l, ln.y, ln.S, ln.i0, ln.i1, nGrid, grid, tau_abs + (size_t)nGrid * z,
                           factor[z], 1, unsorted[z] ? 0 : 1, dpf.layer(z), dtau_abs + (size_t)nGrid * z, (size_t)nGrid * pf.nz);
}
// the instantiations of a kernel template, indexed by LineShape: the one place the shape is dispatched
#define MOM_BY_SHAPE(K) {K<kVoigtSD>, K<kVoigt15>, K<kDoppler>, K<kLorentz>}
decltype(&k_voigt<kVoigtSD>) const kValueKernel[4] = MOM_BY_SHAPE(k_voigt);
decltype(&k_voigt_dual<kVoigtSD>) const kDualKernel[4] = MOM_BY_SHAPE(k_voigt_dual);
decltype(&k_voigt_profile<kVoigtSD>) const kProfileKernel[4] = MOM_BY_SHAPE(k_voigt_profile);
decltype(&k_voigt_profile_dual<kVoigtSD>) const kProfileDualKernel[4] = MOM_BY_SHAPE(k_voigt_profile_dual);
#undef MOM_BY_SHAPE

thread_local double v_last_ms = 0.0;

}  // namespace

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
// DUAL: the same statements on ForwardDiff.Dual numbers -- every value below is formed exactly as in the value run, the
// partials follow each statement by its rule (into dd, with dcgd = d cgd / dT); windows and the sortedness flag come from the values
template <bool DUAL>
__device__ __forceinline__ void line_prefactors_one(int j, const MomLineTable &tb, int nGrid, const double *grid, double p, double T,
                                                    double vmr, double wing, double cgd, const MomLineOut out, int *unsorted,
                                                    const MomLinePartialsOut dd, double dcgd) {
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
  out.nu[j] = v;
  out.gamma_d[j] = g;
  const double ynum = sqrt(cLn2) * gl;
  out.y[j] = ynum / g;
  out.S[j] = S;
  out.gamma_l[j] = gl;   // line_shape! takes gamma_l next to y (:118-124): the fifth prefactor, read by the Lorentz shape
  if constexpr (DUAL) {
    // nu = nu0 + p / p_ref delta;  gamma_l = lin(p) (t_ref / T)^n: d/dp = the bracket times the power (no gamma_l / p),
    // d/dT = lin n (t_ref / T)^(n - 1) (-t_ref / T^2);  gamma_d = cgd(T) nu0 / sqrt(w);  y = sqrt(ln 2) gamma_l / gamma_d
    const double n = tb.n_air[j];
    const double dgl_p = (tb.g_air[j] * (1 - vmr) / p_ref + tb.g_self[j] * vmr / p_ref) * tpow;
    const double lin = tb.g_air[j] * (1 - vmr) * p / p_ref + tb.g_self[j] * vmr * p / p_ref;
    const double dgl_T = lin * (n * pow(t_ref / T, n - 1) * (-(t_ref / (T * T))));
    const double dg_T = dcgd * nu0 / tb.sqw[j];
    dd.dnu[j] = (1 / p_ref) * tb.d_air[j];
    dd.dnu[j + dd.ks] = 0.0;
    dd.dgamma_d[j] = 0.0;
    dd.dgamma_d[j + dd.ks] = dg_T;
    dd.dy[j] = sqrt(cLn2) * dgl_p * (1 / g);
    dd.dy[j + dd.ks] = sqrt(cLn2) * dgl_T * (1 / g) + dg_T * (-(ynum / (g * g)));
    dd.dS[j] = 0.0;
    dd.dS[j + dd.ks] = dS_T;
    dd.dgamma_l[j] = dgl_p;
    dd.dgamma_l[j + dd.ks] = dgl_T;
  }
  const int a = (int)rint(interp_index(grid, nGrid, v - wing, 1.0)), b = (int)rint(interp_index(grid, nGrid, v + wing, (double)nGrid));
  out.i0[j] = a;
  out.i1[j] = b;
  if (j > 0) {  // does the Voigt kernel's bisection apply?  (window starts and stops non-decreasing in the line index)
    const double vp = tb.nu0[j - 1] + p / p_ref * tb.d_air[j - 1];
    const int ap = (int)rint(interp_index(grid, nGrid, vp - wing, 1.0)), bp = (int)rint(interp_index(grid, nGrid, vp + wing, (double)nGrid));
    if (a < ap || b < bp) atomicOr(unsorted, 1);
  }
}
__global__ void k_line_prefactors(MomLineTable tb, int nGrid, const double *grid, double p, double T, double vmr, double wing,
                                  double cgd, MomLineOut out, int *unsorted) {
  line_prefactors_one<false>(blockIdx.x * blockDim.x + threadIdx.x, tb, nGrid, grid, p, T, vmr, wing, cgd, out, unsorted, MomLinePartialsOut{},
                             0.0);
}
// blockIdx.y = layer; prm = [p | T | cgd | factor][nz], Dual run: | d cgd / dT and the partials into dpf
template <bool DUAL>
__global__ void k_line_prefactors_profile(MomLineTable tb, MomLineBlock pf, MomLinePartialBlock dpf, int nGrid, const double *grid,
                                          const double *prm, double vmr, double wing, int *unsorted) {
  const int z = blockIdx.y, Nz = pf.nz;
  line_prefactors_one<DUAL>(blockIdx.x * blockDim.x + threadIdx.x, tb, nGrid, grid, prm[z], prm[Nz + z], vmr, wing, prm[2 * Nz + z], pf.layer(z),
                            unsorted + z, DUAL ? dpf.layer(z) : MomLinePartialsOut{}, DUAL ? prm[4 * Nz + z] : 0.0);
}
hipError_t mom_voigt_profile_launch(hipStream_t st, int shape, const MomLineTable &tb, const MomLineBlock &pf, const MomLinePartialBlock *dpf,
                                    int nGrid, const double *grid, const double *prm, double vmr, double wing, int *unsorted,
                                    double *tau_abs, double *dtau_abs, const double *factor) {
  if (tb.nLines <= 0 || pf.nz <= 0) return hipSuccess;
  hipLaunchKernelGGL(dpf ? k_line_prefactors_profile<true> : k_line_prefactors_profile<false>, dim3((tb.nLines + 255) / 256, pf.nz), dim3(256),
                     0, st, tb, pf, dpf ? *dpf : MomLinePartialBlock{}, nGrid, grid, prm, vmr, wing, unsorted);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 blocks((nGrid + kBlock - 1) / kBlock, pf.nz);
  if (dpf)
    hipLaunchKernelGGL(kProfileDualKernel[shape], blocks, dim3(kBlock), 0, st, tb.nLines, pf, *dpf, nGrid, grid, tau_abs, dtau_abs, factor,
                       unsorted);
  else
    hipLaunchKernelGGL(kProfileKernel[shape], blocks, dim3(kBlock), 0, st, tb.nLines, pf, nGrid, grid, tau_abs, factor, unsorted);
  return hipGetLastError();
}
hipError_t mom_line_prefactors_launch(hipStream_t st, const MomLineTable &tb, int nGrid, const double *grid, double p, double T,
                                      double vmr, double wing, double cgd, const MomLineOut &out, int *unsorted) {
  if (tb.nLines <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_line_prefactors, dim3((tb.nLines + 255) / 256), dim3(256), 0, st, tb, nGrid, grid, p, T, vmr, wing, cgd, out, unsorted);
  return hipGetLastError();
}

// one launch for all lines on `st` (device pointers); used by mom_voigt_xsec below and by the handle-level
// mom_voigt_tau_abs (mom_optics.hip), which accumulates straight into the resident tau_abs table
hipError_t mom_voigt_launch(hipStream_t st, int shape, int nLines, const MomLineView &ln, const MomLinePartials *dln, int nGrid,
                            const double *grid, double *out, double *dout, size_t os, double factor, int accumulate, int sorted) {
  const dim3 blocks((nGrid + kBlock - 1) / kBlock);
  if (dln)
    hipLaunchKernelGGL(kDualKernel[shape], blocks, dim3(kBlock), 0, st, nLines, ln, *dln, nGrid, grid, out, dout, os, factor, accumulate, sorted);
  else
    hipLaunchKernelGGL(kValueKernel[shape], blocks, dim3(kBlock), 0, st, nLines, ln, nGrid, grid, out, factor, accumulate, sorted);
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
  // one device allocation (a one-layer line block | grid | sigma; Dual run: | its partial block | dsigma) and one pinned-free
  // staging copy per array on a private stream; callers that evaluate many layers should use the handle-level mom_voigt_tau_abs,
  // which keeps all of this resident
  MomLineBlock blk = {nullptr, (size_t)(nLines > 0 ? nLines : 1), 1};
  MomLinePartialBlock dblk = blk.partials(nullptr);
  const size_t bytes = (blk.doubles() + 2 * (size_t)nGrid + (dual ? dblk.doubles() + 2 * (size_t)nGrid : 0)) * sizeof(double);
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
    blk.base = (double *)base;
    double *d_grid = blk.base + blk.doubles(), *d_sig = d_grid + nGrid;
    dblk.base = d_sig + nGrid;
    double *d_dsig = dual ? dblk.base + dblk.doubles() : nullptr;   // [nGrid, 2]
    MomLineOut ln = blk.layer(0);
    MomLinePartialsOut dln = dblk.layer(0);
    for (int k = 0; k < 5; ++k)   // an array the shape does not read stays as allocated: the kernel never loads it
      if (nLines && line[k] && mom_shape_reads(shape, k))
        VCHK(hipMemcpyAsync(ln.prefactor(k), line[k], (size_t)nLines * sizeof(double), hipMemcpyHostToDevice, st));
    if (nLines) {
      VCHK(hipMemcpyAsync(ln.i0, ind_start, (size_t)nLines * sizeof(int), hipMemcpyHostToDevice, st));
      VCHK(hipMemcpyAsync(ln.i1, ind_stop, (size_t)nLines * sizeof(int), hipMemcpyHostToDevice, st));
    }
    VCHK(hipMemcpyAsync(d_grid, grid, (size_t)nGrid * sizeof(double), hipMemcpyHostToDevice, st));
    for (int q = 0; q < 5 && dual; ++q) {
      if (!nLines || !dpart[q] || !mom_shape_reads(shape, q)) { dln.partial(q) = nullptr; continue; }   // null: zeros
      for (int k = 0; k < 2; ++k)   // host [nLines, 2] column-major
        VCHK(hipMemcpyAsync(dln.partial(q) + dln.ks * k, dpart[q] + (size_t)nLines * k, (size_t)nLines * sizeof(double),
                            hipMemcpyHostToDevice, st));
    }
    const MomLinePartials dread = dln;
    VCHK(hipEventCreate(&e0));
    VCHK(hipEventCreate(&e1));
    VCHK(hipEventRecord(e0, st));
    VCHK(mom_voigt_launch(st, shape, nLines, ln, dual ? &dread : nullptr, nGrid, d_grid, d_sig, d_dsig, (size_t)nGrid, 1.0, 0, sorted));
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
