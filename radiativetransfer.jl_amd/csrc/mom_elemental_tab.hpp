// mom_elemental_tab.hpp -- the second form of the elemental layer (MOM_OPT_ELEMENTAL), for the two first-stage images of the
// headline: the two-buffer strip image (mom_strip2.hpp, HOLDT) and the quad-block image (mom_q4.hpp).  It writes what
// elemental_build (mom_kernels.hpp) writes -- c.r, c.t, c.jp, c.jm, the sun-block columns -- bit for bit, and differs in how:
//   * the layer-independent stream-pair tables SI = 1/mu_i + 1/mu_j, F1 = mu_j/(mu_i + mu_j), F2 = mu_j/(mu_i - mu_j) come from a
//     device table built once per handle (mom_scene.hip k_stream_tables: the expressions of elemental_build on the same operands;
//     FP64 division and addition are correctly rounded, so the values are those the per-layer pass computed).  A layer's table pass
//     is E = 1 - exp(-dtau SI) on the Nq (Nq + 1) / 2 pairs iq <= jq, stored to both positions (a + b == b + a: E is symmetric bit
//     for bit); F1 and F2 are read from the global table together with the phase-matrix bases, one batch ahead;
//   * what is uniform for the launch is decided before it: the host launches this form only for regular streams, tables that apply,
//     two phase-matrix bases and an edge that is a whole number of streams (mom_elemental_tab_applies), and the kernel without it
//     otherwise; N, the pitch and the workgroup size are compile-time, the coordinates advance by kThreads = DJ N + DI without a division;
//   * a batch of B elements requests all its LDS operands together, waits once, forms r and every alternative of t with the
//     expressions of elemental_build in the same association and picks by select.  An alternative that is not picked may be Inf or
//     NaN (F2 of an equal-mu pair is); nd >= 1 is the multiplier sg_i or 1.0; the sun-block column stores stay predicated;
//   * the source pass takes mu_s/(mu_i -+ mu_s) from the same tables, entry (iq, sq), and dtau/mu_i from c.v2.
// Signed zeros: none differs -- every output is the product or the constant elemental_build forms.
#pragma once
#include "mom_kernels.hpp"

namespace MOM_NS {

// May a launch with the stream set q (its tables in stab) and K bases take the table form?  The host decides it once per launch
// (mom_scene.hip launch_first_stage) and picks the kernel: regular streams, an edge of whole streams, two bases, and the per-layer
// tables of elemental_build apply (its `tab`; mat_elems is the same number in every build at the edges of the two images)
__host__ __device__ inline bool mom_elemental_tab_applies(const DevStreams &q, int K, const real *stab) {
  if (stab == nullptr || !q.regular || K != 2 || q.nS < 1 || q.N % q.nS != 0) return false;
  const int Nq = q.N / q.nS;
  return 3 * Nq * Nq <= (int)mat_elems(q.N);
}

// B: elements per batch (a divisor of 8).  The quad-block image takes four; the two-buffer strip image two -- with four in flight and
// four in the works on top of the eight held t entries it would not stay free of scratch at two waves per SIMD
template <bool HOLDT, int B, int N, int LD, class FZ>
__device__ __forceinline__ void elemental_build_tab(const Ctx &c, const DevStreams &q, const real *stab, int m, int nd,
                                                    real tau_sum, real dtau, real varpi, FZ Zpp, FZ Zmp) {
  constexpr int T = kThreads, NN = N * N, SLOTS = (NN + T - 1) / T, NB = (SLOTS + B - 1) / B;
  constexpr int DI = T % N, DJ = T / N;  // one slot further: e + T = (i + DI) + (j + DJ) N
  constexpr int HELD = HOLDT ? 8 / B : 0;  // batches whose t entries wait in registers (the first eight slots, as elemental_build)
  static_assert(N <= T, "one row per thread in the source pass");
  static_assert(8 % B == 0 && (!HOLDT || NB > HELD), "HOLDT: whole batches in the first eight slots, and more than eight slots");
  const real winv = (m == 0) ? 0.5 : 0.25;
  const real wct02 = (m == 0) ? 0.5 : 0.25;
  const int n = q.nS, Nq = N / n, NQ2 = Nq * Nq;
  FastDiv fs;
  fs.init(n);
  real *E = c.tabE, *ZS = c.tabZS;
  const gdouble *SI = as_global(stab), *F1 = SI + NQ2, *F2 = SI + 2 * NQ2;
  const int tid = wg_tid();
  const int i_start = n * (q.imu0 - 1), i_end = n * q.imu0;
  const int sq = q.imu0 - 1;
  // a batch in flight: the four bases and the two table entries of each element, requested one batch ahead of their use
  struct Batch {
    real bp0[B], bm0[B], bp1[B], bm1[B], f1[B], f2[B];
    int ij[B];  // i | j << 8; j = N: past the last element (the loads then take element (0, 0), nothing is stored)
  };
  static_assert(N < 256, "packed coordinates");
  int ni = tid % N, nj = tid / N;  // the next slot to request
  auto issue = [&](Batch &b) {
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const bool ok = nj < N;
      const int i = ok ? ni : 0, j = ok ? nj : 0;
      b.ij[u] = i | ((ok ? nj : N) << 8);
      int iq, jq, dummy;
      fs.split(i, dummy, iq);
      fs.split(j, dummy, jq);
      const int pq = iq + jq * Nq;
      b.bp0[u] = Zpp.basis(0, i, j);
      b.bm0[u] = Zmp.basis(0, i, j);
      b.bp1[u] = Zpp.basis(1, i, j);
      b.bm1[u] = Zmp.basis(1, i, j);
      b.f1[u] = F1[pq];
      b.f2[u] = F2[pq];
      ni += DI;
      nj += DJ;
      if (ni >= N) {
        ni -= N;
        ++nj;
      }
    }
  };
  Batch cur, nxt;
  issue(cur);
  // the source pass's table entries (iq, sq) of this thread's row travel under the whole element loop
  const int srow = tid < N ? tid : 0;
  int siq, sdummy;
  fs.split(srow, sdummy, siq);
  const real sf1 = F1[siq + sq * Nq], sf2 = F2[siq + sq * Nq];
  for (int i = tid; i < N; i += T) {
    c.ei[i] = exp(-dtau / c.mu[i]);
    c.v1[i] = c.wt[i] * winv;   // wct
    c.v2[i] = dtau / c.mu[i];
  }
  // E on the pairs iq <= jq, e = jq (jq + 1) / 2 + iq
  for (int e = tid; e < (Nq * (Nq + 1)) / 2; e += T) {
    int jq = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    if ((jq * (jq + 1)) / 2 > e) --jq;
    else if (((jq + 1) * (jq + 2)) / 2 <= e) ++jq;
    const int iq = e - (jq * (jq + 1)) / 2;
    const real v = 1 - exp(-dtau * SI[iq + jq * Nq]);
    E[iq + jq * Nq] = v;
    E[jq + iq * Nq] = v;
  }
  __syncthreads();
  MOM_STAMP(46);
  const real wp0 = Zpp.weight(0), wm0 = Zmp.weight(0), wp1 = Zpp.weight(1), wm1 = Zmp.weight(1);
  const bool dsign = nd >= 1;  // apply_D_elemental!, elemental.jl:265-269
  real th[HOLDT ? 8 : 1];
  auto element_math = [&](const Batch &b, const int H) {  // H >= 0 (a constant once unrolled): the t entries go to th[H ..]
    real wj[B], eii[B], eij[B], v2i[B], sgi[B], Epq[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int i = b.ij[u] & 255, jr = b.ij[u] >> 8, j = jr < N ? jr : 0;
      int iq, jq, dummy;
      fs.split(i, dummy, iq);
      fs.split(j, dummy, jq);
      wj[u] = c.v1[j];
      eii[u] = c.ei[i];
      eij[u] = c.ei[j];
      v2i[u] = c.v2[i];
      sgi[u] = c.sg[i];
      Epq[u] = E[iq + jq * Nq];
    }
    MOM_STAMP(49);
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int i = b.ij[u] & 255, j = b.ij[u] >> 8;
      const bool ok = j < N;
      // Z = sum_k w_k Z_k, accumulated in k order
      real zp = 0.0, zm = 0.0;
      zp += wp0 * b.bp0[u];
      zm += wm0 * b.bm0[u];
      zp += wp1 * b.bp1[u];
      zm += wm1 * b.bm1[u];
      if (ok && j >= i_start && j < i_end) {
        ZS[i + (j - i_start) * N] = zp;
        ZS[i + (n + j - i_start) * N] = zm;
      }
      const bool live = wj[u] > 1.e-8, diag = (i == j);
      const real rl = varpi * zm * b.f1[u] * wj[u] * Epq[u];
      const real td = eii[u] * (1 + varpi * zp * v2i[u] * wj[u]);  // (i == j: wj is c.v1[i])
      const real to = varpi * zp * b.f2[u] * wj[u] * (eii[u] - eij[u]);
      // mu_i == mu_j, read off the table: F2 = mu_j / (mu_i - mu_j) is infinite for exactly those pairs (mu_j > 0, and a difference
      // of two unequal stream values is no smaller than an ulp of them: the quotient stays finite)
      const real tl = __builtin_isinf(b.f2[u]) ? (diag ? td : 0.0) : to;
      real rr = live ? rl : 0.0;
      const real tt = live ? tl : (diag ? eii[u] : 0.0);
      rr *= dsign ? sgi[u] : 1.0;
      if (ok) c.r[i + j * LD] = rr;
      if constexpr (HOLDT) {
        if (H >= 0) th[(H >= 0 ? H : 0) + u] = tt;
        else if (ok) c.t[i + j * LD] = tt;
      } else if (ok) {
        c.t[i + j * LD] = tt;
      }
    }
    MOM_STAMP(57);
  };
  auto copy_next = [&]() {
#pragma unroll
    for (int u = 0; u < B; ++u) {
      cur.bp0[u] = nxt.bp0[u]; cur.bm0[u] = nxt.bm0[u]; cur.bp1[u] = nxt.bp1[u]; cur.bm1[u] = nxt.bm1[u];
      cur.f1[u] = nxt.f1[u]; cur.f2[u] = nxt.f2[u];
      cur.ij[u] = nxt.ij[u];
    }
  };
#pragma unroll
  for (int hb = 0; hb < HELD; ++hb) {  // (NB > HELD: there is a batch behind each of these)
    issue(nxt);
    element_math(cur, hb * B);
    copy_next();
  }
#pragma nounroll
  for (int b = HELD; b < NB; ++b) {
    const bool more = b + 1 < NB;
    if (more) issue(nxt);
    element_math(cur, -1);
    if (more) copy_next();
  }
  __syncthreads();
  MOM_STAMP(47);
  const real mus = c.mu[i_start];
  const real att = exp(-tau_sum / mus);
  for (int i = tid; i < N; i += T) {  // (N <= T: i is this thread's row srow)
    real zp = 0.0, zm = 0.0;
    for (int k = 0; k < n; ++k) {
      zp += ZS[i + k * N] * q.I0[k];
      zm += ZS[i + (n + k) * N] * q.I0[k];
    }
    const bool sun = i >= i_start && i < i_end;
    const real jps = wct02 * varpi * zp * c.v2[i] * c.ei[i];
    const real jpo = wct02 * varpi * zp * sf2 * (c.ei[i] - c.ei[i_start]);
    real jp = sun ? jps : jpo;
    real jm = wct02 * varpi * zm * sf1 * E[siq + sq * Nq];
    jp *= att;
    jm *= att;
    const int kd = i - siq * n;  // i % n
    const real Dk = kd == 0 ? q.D[0] : kd == 1 ? q.D[1] : kd == 2 ? q.D[2] : q.D[3];
    if (nd >= 1) jm = Dk * jm;  // elemental.jl:249-251
    c.jp[i] = jp;
    c.jm[i] = jm;
  }
  __syncthreads();
  if constexpr (HOLDT) {  // the tables are read: the held t entries go home
    int hi = tid % N, hj = tid / N;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (hj < N) c.t[hi + hj * LD] = th[u];
      hi += DI;
      hj += DJ;
      if (hi >= N) {
        hi -= N;
        ++hj;
      }
    }
    __syncthreads();
  }
  MOM_STAMP(48);
}

}  // namespace MOM_NS
