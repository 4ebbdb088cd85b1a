// mom_reduce.hpp -- the m = 0 reduction (include/momcore.h, MOM_OPT_M0_REDUCTION) as plain host functions on double arrays: the
// test on the data, the cut of streams and phase-matrix bases to the (I,Q) sub-problem, the cut of the m = 0 BRDF matrix.
// Both host drivers call it; the options and kernel routes in front of the data test and the edge N0 >= N0r of the sub-problem's
// kernels stay with the caller.  No HIP, nothing of MOM_NS / MOM_REAL: a host compiler can include it alone (tests/host/).
#pragma once
#include <cstddef>
#include <vector>

#pragma GCC visibility push(hidden)  // internal to the library that includes it: no exported symbol
constexpr int kMomM0Stokes = 2;  // Stokes components of the sub-problem: (I,Q)

// entry i0 of the sub-problem is entry full(i0) of the full problem: the first two components of stream i0 / 2
inline int mom_m0_full(int i0, int nS) { return (i0 / kMomM0Stokes) * nS + (i0 % kMomM0Stokes); }
// real entries of the sub-problem of an edge N = nS Nq
inline int mom_m0_edge(int N, int nS) { return kMomM0Stokes * (N / nS); }

// Moment 0 decouples into (I,Q) and (U,V) when the source has no U, V (I0[k] == 0 for k >= 2; I0 holds 4 entries) and no basis
// of Zpp / Zmp [N,N,K,M] has an (I,Q) <-> (U,V) entry in its moment-0 block; checked on the data, bitwise
// (mom_m0_source: the source's half alone, for bases whose entries are tested where they are formed, mom_zmom.hip)
inline bool mom_m0_source(const double *I0, int nS) {
  for (int k = 2; k < nS; ++k)
    if (I0[k] != 0.0) return false;
  return true;
}
inline bool mom_m0_reducible(const double *I0, int N, int nS, int K, const double *Zpp, const double *Zmp) {
  if (!mom_m0_source(I0, nS)) return false;
  for (int kb = 0; kb < K; ++kb)
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < N; ++i) {
        if (((i % nS) < 2) == ((j % nS) < 2)) continue;
        const size_t o = i + (size_t)N * (j + (size_t)N * kb);  // moment 0 block
        if (Zpp[o] != 0.0 || Zmp[o] != 0.0) return false;
      }
  return true;
}

// The sub-problem on an edge N0 >= N0r = mom_m0_edge(N, nS): streams [N0] and the moment-0 blocks [N0,N0,K]; the entries behind
// N0r are dummy entries (mu = 1, weight 0, sigma = 1, Z = 0: the pad rule of mom_host.hpp)
struct MomM0Cut {
  std::vector<double> mu, wt, sg, Zpp, Zmp;
};
// the streams alone (Zpp, Zmp empty): for bases that are cut on the device (mom_zmom.hip)
inline MomM0Cut mom_m0_cut_streams(const double *mu, const double *wt, int N, int nS, int N0) {
  const int N0r = mom_m0_edge(N, nS);
  MomM0Cut c{std::vector<double>(N0, 1.0), std::vector<double>(N0, 0.0), std::vector<double>(N0, 1.0), {}, {}};
  for (int i = 0; i < N0r; ++i) { c.mu[i] = mu[mom_m0_full(i, nS)]; c.wt[i] = wt[mom_m0_full(i, nS)]; }
  return c;
}
inline MomM0Cut mom_m0_cut(const double *mu, const double *wt, int N, int nS, int K, int N0, const double *Zpp, const double *Zmp) {
  const int N0r = mom_m0_edge(N, nS);
  MomM0Cut c = mom_m0_cut_streams(mu, wt, N, nS, N0);
  c.Zpp.assign((size_t)N0 * N0 * K, 0.0);
  c.Zmp = c.Zpp;
  for (int kb = 0; kb < K; ++kb)
    for (int j = 0; j < N0r; ++j)
      for (int i = 0; i < N0r; ++i) {
        const size_t src = mom_m0_full(i, nS) + (size_t)N * (mom_m0_full(j, nS) + (size_t)N * kb);
        c.Zpp[i + (size_t)N0 * (j + (size_t)N0 * kb)] = Zpp[src];
        c.Zmp[i + (size_t)N0 * (j + (size_t)N0 * kb)] = Zmp[src];
      }
  return c;
}

// The m = 0 BRDF matrix Rsurf [N,N] cut to r0 [N0,N0] (zero behind the real entries); false when it couples (I,Q) with (U,V)
constexpr const char *kMomM0BrdfCouples =
    "mom_scene_set_surface: the m = 0 BRDF matrix couples (I,Q) with (U,V); set MOM_OPT_M0_REDUCTION = 0 before "
    "mom_scene_set for this surface";
inline bool mom_m0_cut_brdf(const double *Rsurf, int N, int nS, int N0, std::vector<double> &r0) {
  const int nS0 = kMomM0Stokes;
  r0 = std::vector<double>((size_t)N0 * N0, 0.0);
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      const bool iq_i = (i % nS) < nS0, iq_j = (j % nS) < nS0;
      const double v = Rsurf[i + (size_t)N * j];
      if (iq_i != iq_j && v != 0.0) return false;
      if (iq_i && iq_j) r0[(i / nS) * nS0 + (i % nS) + (size_t)N0 * ((j / nS) * nS0 + (j % nS))] = v;
    }
  return true;
}

#pragma GCC visibility pop
