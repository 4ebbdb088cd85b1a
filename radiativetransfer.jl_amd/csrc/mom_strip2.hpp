// mom_strip2.hpp -- the TWO-BUFFER 4-wave strip image (r7): Float64, N = 52, 56, 60 (KS = 13 .. 15), TWO workgroups per CU.
//
// Why (profiles/r05_phase_stamps_n60.txt): the 8-wave N = 60 image holds r, t, P, Q (4 x 32.7 KB) + vectors + the
// stream-pair tables, 149 KB: one workgroup per CU.  72 % of its time is inside the strip chains, where one wave per SIMD keeps
// the matrix pipe saturated; the other 28 % (elemental layer, composite loads, the B product, write-backs, barriers) leave the
// pipe idle, and in the doubling steps (56 % of the kernel) waves 4 .. 7 only wait at the barriers.  Only a second independent
// unit on the CU can fill those gaps.  This image:
//   * buffers r and t only (2 x 32.7 KB at N = 60) + vectors with `part` cut to its 16 norm slots + a 128-real layer tail:
//     74.8 KB, two workgroups per CU;
//   * four waves, one column strip each (N = 52 .. 60: four 16-row tiles);
//   * elemental layer: its tables (E, F1, F2 and the sun-block columns) in t's buffer; elemental_build<true> keeps the t entries
//     of its first batch -- the only ones whose addresses can meet the tables -- in registers and stores them after the tables
//     are done (s2_applies checks that the tables end below the first directly stored entry);
//   * doubling: P = r r overwrites t's buffer (each wave its own strip, whose t^T strip it holds in registers for the Horner loop
//     anyway); after the series and (A r)^T, t is restored from those registers (two barriers more per step);
//   * interaction (interface 11): R+- staged in r's buffer (r's strip held in registers), B over it, the two Horner chains, r
//     restored, the products with r and t, then T++ staged in t's buffer for the last two products;
//   * anything else -- a series beyond kStripMaxP terms, a forced pivoted inverse -- is not computed here: the workgroup records
//     the layer in resume[unit] and leaves the unit; nothing of that layer has reached the composite state in global memory, so
//     the 8-wave image's launch behind it (LayerArgs::resume) redoes the layer and carries the unit to the end.
// Every product is the one of the 8-wave image's strip path (mom_strip.hpp) on the same operands in the same order: the results
// are bitwise those of the 8-wave image.
// Scope: Float64, 4-wave build, sweep mode, single composite (no multi-target), interface 11 on every layer after the first.
//
// Sources only (MOM_OPT_SOURCES_ONLY, k_layer_s2<.., SRC = true>; the quad-block image has the same form, mom_q4.hpp).  Of the four
// composite operators R+- and T-- feed the next layer's B, W0, the two series and the sources; R-+ += (T01 r-+) T++ and
// T++ = T21 T++ feed only themselves.  The sources take ONE ROW from each of those two products, the riding row:
// J0- += T01 (r-+ J0+ + j0-) takes J0+^T V, J0+ = j0+ + T21 (J0+ + R+- j0-) takes J0+^T T21^T.  Everything mom_rt_run hands out
// (R, T, hdr, the BHRs) comes from J0+-, and mom_download returns moment 0 of the full problem only (MOM_ESTATE when moment 0 ran on
// the sub-problem).  So in a launch of mom_rt_run that holds no observable moment -- the (I,Q) sub-problem's, or a full-problem launch
// with m_first >= 1 -- the host asks for SRC, and section (d) of the interaction neither loads R-+, nor stages T++ in t's buffer,
// nor stores either: J0+ goes to column N of t's buffer and strip_ride (mom_strip.hpp) forms the two riding rows with the matrix
// instructions the full products would have issued for them, in the same order: J0+- keep their bits.
// What the two arrays hold afterwards: store_added_as_composite is unchanged, so the FIRST layer's r-+ and t++ -- finite, rewritten
// by every run, meaningless.  Who reads them: the 8-wave image where it finishes a unit (interaction_strip / interaction_core) and
// k_surface, which go on updating the two operators from there.  In all three R-+ is read only as the addend of its own update and
// T++ only as the multiplier of the two products above, whose riding rows come from the riding column J0+, not from T++: nothing of
// the two arrays enters a J0+-, a Frobenius sum (those are taken over B = r-+ R+- alone) or, through it, a series length or a resume
// decision.  mom_rt_run_multisensor (k_combine, k_interlayer read all four operators), the Dual and RRS runs and the operator-level
// calls never launch SRC; nor do the scheduling modes 0, 2, 3, which keep the recorded forms of their experiments.
#pragma once
#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_elemental_tab.hpp"

namespace MOM_NS {

// MOM_OPT_STRIP2_SCHED (LayerArgs::sched, MomLaunchForm::sched_mode): how the workgroups share the units and the two of a CU its matrix pipe.
//   * Bit 0 (default on), a shared unit queue: the units are handed out by an atomic ticket instead of pt += gridDim.x, so no
//     workgroup idles through a partial last round; resume[] stays indexed by unit.  Units are independent: the order does not
//     change a result.  C2: full layers 272.7 -> 263.0 ms, N = 52 / 56 -2 % (profiles/r08_C2_ab.txt).
//   * Bit 1 (default off), asymmetric chain priority: the workgroup that arrives SECOND on its CU (a ticket per CU, keyed by the
//     XCC / SE / SH / CU ids of the hardware registers -- blockIdx says nothing about residency) runs every strip chain at wave
//     priority 1 and everything else at 0.  Meant against two units running in lock-step; the timelines
//     (profiles/r08_phase_stamps_s2.txt) show that they do not (both outside a chain: 5 % of the time), and the priority only moves
//     time from the favoured unit's chains to its non-chain sections: 1.5 ms gained alone, 1.6 ms lost on top of the queue.
// The kernel is instantiated per value of the mask (k_layer_s2<KS, MODE>): 0 is the kernel as it was before the option, and the
// default carries nothing of the priority.
constexpr int kS2CuKeys = 2048;     // XCC id (3 bits) x HW_ID bits 15:8 (CU, SH, SE)
constexpr int kS2SchedInts = 1 + kS2CuKeys;
#define MOM_S2_GETREG(id, off, size) ((((size)-1) << 11) | ((off) << 6) | (id))
__device__ __forceinline__ int s2_cu_key() {
  const unsigned cu = __builtin_amdgcn_s_getreg(MOM_S2_GETREG(4, 8, 8));    // HW_REG_HW_ID: cu_id 11:8, sh_id 12, se_id 15:13
  const unsigned xcc = __builtin_amdgcn_s_getreg(MOM_S2_GETREG(20, 0, 4));  // HW_REG_XCC_ID
  return (int)(((xcc & 7u) << 8) | cu);
}
#ifndef MOM_S2_PRIO
#define MOM_S2_PRIO 1
#endif
// the boundary of a strip chain: the favoured workgroup raises / drops its priority (the flag is kept in the LDS int c.ipiv[1], not
// in a scalar register: the kernel has none to spare); sec = the timeline id (diagnostic builds) of the section that ends here
// PRIO = false (every instantiation without bit 1 of the mode): nothing is emitted
__device__ __forceinline__ int s2_favoured(const Ctx &c) { return __builtin_amdgcn_readfirstlane(c.ipiv[1]) & 1; }
template <bool ON, bool PRIO>
__device__ __forceinline__ void s2_chain(const Ctx &c, int sec, int fav) {
#ifndef MOM_DIAG_TIMELINE
  if constexpr (PRIO)
#endif
  {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PRIO)
      if (fav) __builtin_amdgcn_s_setprio(ON ? MOM_S2_PRIO : 0);
    MOM_TL(c, sec);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// the unit a QUEUE workgroup is on: its ticket, from LDS into a scalar register
#define S2_UNIT(c) ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((c).ipiv[0]))
// timeline sections (diagnostic builds): what a workgroup was in until the event
enum { S2_SEC_TOP = 0, S2_SEC_ELEM = 1, S2_SEC_DBL = 2, S2_SEC_DEND = 3, S2_SEC_ICOPY = 4, S2_SEC_ICH1 = 5, S2_SEC_ICOPY2 = 6,
       S2_SEC_ICH2 = 7, S2_SEC_IEND = 8, S2_SEC_FIRST = 9 };

constexpr int kS2Lay = 128;  // reals of the layer-scalar tail
__host__ __device__ inline size_t s2_vec_reals(int N) { return part_offset_doubles(N) + 16; }
__host__ __device__ inline size_t s2_lds_bytes(int N) { return (2 * mat_elems(N) + s2_vec_reals(N) + kS2Lay) * sizeof(real); }
// the elemental layer's table space at the front of t's buffer: E | F1 | F2 per stream pair (when they fit a buffer, as in
// elemental_build) and the sun-block columns, 2 nS columns of N
__host__ __device__ inline int s2_table_reals(int N, int ns, int nS) {
  const int Nq = N / (ns > 0 ? ns : 1);
  const bool tab = 3 * Nq * Nq <= (int)mat_elems(N);
  return (tab ? 3 * Nq * Nq : 0) + 2 * nS * N;
}
// t-buffer offset of the first element that elemental_build<true> stores directly: element 8 kThreads (slot 8 of the linear order)
__host__ __device__ inline int s2_direct_offset(int N) {
  const int e = 8 * kThreads;
  return (e % N) + (e / N) * ld_for(N);
}
// does the image apply to operators of edge N with ns Stokes components per stream (nS per stream-pair table row)?
__host__ __device__ inline bool s2_applies(int N, int ns, int nS) {
  return kF64 && kWaves == 4 && (N == 52 || N == 56 || N == 60) && N * N > 8 * kThreads &&
         s2_table_reals(N, ns, nS) <= s2_direct_offset(N) && 2 * (s2_lds_bytes(N) + 1024) <= kLdsPerCU;
}

__device__ __forceinline__ void make_ctx_s2(Ctx &c, int N, int inv_mode, int ns, real *smem) {
  c.N = N;
  c.Np = np_for(N);
  c.nc = cols_for(N);
  c.ld = ld_for(N);
  c.ldv = c.Np;
  c.fd.init(N);
  c.inv_mode = inv_mode;
  c.qpre = 0;
  c.slot = 0;
  c.ptab = nullptr;
  const size_t msz = mat_elems(N);
  c.r = smem; c.t = smem + msz; c.P = nullptr; c.Q = nullptr; c.X = nullptr;
  real *p = smem + 2 * msz;
  const int lv = c.ldv;
  c.jp = p; c.jm = p + lv; c.j1p = p + 2 * lv; c.j1m = p + 3 * lv; c.v1 = p + 4 * lv; c.v2 = p + 5 * lv;
  c.Jp = p + 6 * lv; c.Jm = p + 7 * lv; c.prow = p + 8 * lv; c.pcol = p + 9 * lv; c.rowk = p + 10 * lv;
  c.ei = p + 11 * lv; c.mu = p + 12 * lv; c.wt = p + 13 * lv; c.sg = p + 14 * lv;
  c.thr = p + 15 * lv;
  int *ip = reinterpret_cast<int *>(c.thr + 32);
  c.ipiv = ip; c.sh = ip + lv; c.bad = ip + lv + 1;
  c.part = p + part_offset_doubles(N);
  const int Nq = N / (ns > 0 ? ns : 1);
  c.tabE = c.t;
  c.tabZS = c.t + ((3 * Nq * Nq <= (int)msz) ? 3 * Nq * Nq : 0);
}

// One doubling step (doubling.jl:44-67) in two buffers; returns false, before anything of the step is stored, if it needs the
// general path.  In: c.r (riding columns N, N + 1 = j0+, j0-), c.t, c.jp, c.jm; out: the same, as doubling_step_strip.
template <int KS, int KW, bool RB>
__device__ __forceinline__ bool doubling_step_s2(Ctx &c, real expk) {
  using G = StripGeom<KS>;
  constexpr int N = G::N, NT = G::NT, LD = G::LD;
  static_assert(NT == kWaves, "two-buffer image: one column strip per wave");
  const int lane = wg_lane(), wave = wg_wave(), lr = lane & 15, lq = lane >> 4;
  const int c0 = 16 * wave, col = c0 + lr;
  const bool colok = col < N;
  real *r = c.r, *t = c.t;
  real *P = c.t;  // P = r r lives in t's buffer until t is restored
  r4 T0[NT];
  strip_load_lds<KS>(t, lr, lq, c0, T0);
  // ---- P = r r (+ riding columns r j0+, r j0-) and ||r r||_F^2 (doubling_rr_strip); this wave's strip of P goes to exactly
  // the addresses its T0 load has just read, and the riding columns N, N + 1 of t are read by no product that is stored
  real ss = 0.0;
  {
    r4 W[NT], B[NT];
    strip_load_lds<KS>(r, lr, lq, c0, W);
    strip_zero(B);
    strip_mul<KS, KW, RB>(r, lr, lq, W, B, wave);
    strip_store_lds<KS>(P, lr, lq, c0, colok, B);
    if (colok) {
      if (lq == G::LQ0) P[col + N * LD] = B[G::RT][G::RR0];        // (r j0+)[col]
      if (lq == G::LQ1) P[col + (N + 1) * LD] = B[G::RT][G::RR1];  // (r j0-)[col]
#pragma unroll
      for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if (strip_rowok<KS>(rt, rr, lq)) ss += B[rt][rr] * B[rt][rr];
    }
  }
  wg_sumsq_put(c, ss);
  __syncthreads();
  const real beta2 = wg_sumsq_get(c);
  const int p = __builtin_amdgcn_readfirstlane(neumann_terms_12(beta2));
  if (p > kStripMaxP || c.inv_mode != 0) return false;
  // riding rows of the multiplier r^T: w1 = j1- + r j0+, w2 = j0+ + r j1-  (doubling.jl:51-60); every wave writes the same values
  if (lane < N) {
    r[lane + N * LD] = c.jm[lane] * expk + P[lane + N * LD];
    r[lane + (N + 1) * LD] = c.jp[lane] + expk * P[lane + (N + 1) * LD];
  }
  r4 Y[NT];
  strip_copy(Y, T0);
  // Y = A^T = (t (I - r r)^-1)^T by Horner: Y <- t^T + (r r)^T Y
#pragma nounroll
  for (int k = 1; k < p; ++k) {
    r4 acc[NT];
    strip_copy(acc, T0);
    strip_mul<KS, KW, RB>(P, lr, lq, Y, acc, wave);
    strip_copy(Y, acc);
  }
  r4 Zt[NT];
  strip_zero(Zt);
  strip_mul<KS, KW, RB>(r, lr, lq, Y, Zt, wave);  // (A r)^T ; rows N, N+1: (A w1)^T, (A w2)^T
  const real aw = Zt[G::RT][G::RR0], aw2 = Zt[G::RT][G::RR1];
  __syncthreads();  // every wave is done with P
  strip_store_lds<KS>(t, lr, lq, c0, colok, T0);  // t back
  __syncthreads();
  r4 Rn[NT], Tn[NT];
  strip_load_lds<KS>(r, lr, lq, c0, Rn);
  strip_mul<KS, KW, RB>(t, lr, lq, Zt, Rn, wave);  // r^T + t^T (A r)^T      (:64)
  strip_zero(Tn);
  strip_mul<KS, KW, RB>(t, lr, lq, Y, Tn, wave);   // t^T A^T                (:67)
  __syncthreads();  // every wave is done reading r and t of this step
  strip_store_lds<KS>(r, lr, lq, c0, colok, Rn);
  strip_store_lds<KS>(t, lr, lq, c0, colok, Tn);
  if (colok && lq == G::LQ0) {  // j0- += A w1 (:57)
    const real jm = c.jm[col] + aw;
    c.jm[col] = jm;
    r[col + (N + 1) * LD] = jm;
  }
  if (colok && lq == G::LQ1) {  // j0+ = j1+ + A w2 (:60)
    const real jp = c.jp[col] * expk + aw2;
    c.jp[col] = jp;
    r[col + N * LD] = jp;
  }
  __syncthreads();
  return true;
}

// nd doubling steps; bail = true (nothing of the layer has left the workgroup) if a step needs the general path
template <int KS, bool PRIO, int KW, bool RB>
__device__ __forceinline__ real doubling_run_s2(Ctx &c, int nd, real expk, bool &bail) {
  const int N = c.N, ld = c.ld;
  bail = false;
  if (nd == 0) return expk;
  for (int i = wg_tid(); i < N; i += kThreads) {
    c.r[i + N * ld] = c.jp[i];
    c.r[i + (N + 1) * ld] = c.jm[i];
  }
  __syncthreads();
  const int fav = PRIO ? s2_favoured(c) : 0;
  s2_chain<true, PRIO>(c, S2_SEC_ELEM, fav);  // a doubling step is products and barriers throughout
  for (int it = 0; it < nd; ++it) {
    if (!doubling_step_s2<KS, KW, RB>(c, expk)) {
      s2_chain<false, PRIO>(c, S2_SEC_DBL, fav);
      bail = true;
      return expk;
    }
    expk = expk * expk;
  }
  s2_chain<false, PRIO>(c, S2_SEC_DBL, fav);
  // apply_D! (doubling.jl:93-110) and apply_D_SFI! (:112-118): r-+ rows and j0- scaled by sg
  real *r = c.r;
  for (int e = wg_tid(); e < N * N; e += kThreads) {
    int i, j;
    c.fd.split(e, i, j);
    r[i + j * ld] *= c.sg[i];
  }
  for (int i = wg_tid(); i < N; i += kThreads) {
    c.jm[i] *= c.sg[i];
    r[i + N * ld] = 0.0; r[i + (N + 1) * ld] = 0.0;
  }
  __syncthreads();
  MOM_TL(c, S2_SEC_DEND);
  return expk;
}

// ScatteringInterface_11 in two buffers (see interaction_strip for the algebra; same products, same order).  Returns false,
// nothing stored, if the series is too long.  Ends with a barrier.  SRC: the sources-only form (the header of this file).
template <int KS, bool PRIO, int KW, bool RB, bool SRC = false>
__device__ __forceinline__ bool interaction_strip_s2(Ctx &c, const CompPtrs &g) {
  using G = StripGeom<KS>;
  constexpr int N = G::N, NT = G::NT, LD = G::LD, NN = N * N, U = (NN + kThreads - 1) / kThreads;
  static_assert(NT == kWaves, "two-buffer image: one column strip per wave");
  const int lane = wg_lane(), wave = wg_wave(), lr = lane & 15, lq = lane >> 4;
  const int c0 = 16 * wave, col = c0 + lr;
  const bool colok = col < N;
  real *r = c.r, *t = c.t;
  // ---- (a) r's strip into registers, R+- into r's buffer; B = r-+ R+- and W0 = R+-^T t++^T on strips
  r4 rT[NT];
  {
    real vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = wg_tid() + u * kThreads;
      if (e < NN) {
        int i, j;
        c.fd.split(e, i, j);
        vr[u] = MOM_NT_LOAD(g.R_pm + i + j * G::CP);
      }
    }
    strip_load_lds<KS>(r, lr, lq, c0, rT);
    __syncthreads();  // every wave holds its strip of r
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = wg_tid() + u * kThreads;
      if (e < NN) {
        int i, j;
        c.fd.split(e, i, j);
        r[i + j * LD] = vr[u];
      }
    }
  }
  __syncthreads();
  const int fav = PRIO ? s2_favoured(c) : 0;  // (read once per interaction: the later boundaries have no vector register to spare)
  s2_chain<true, PRIO>(c, S2_SEC_ICOPY, fav);
  const real *Rpm = r;
  r4 Bs[NT], W0[NT];
  real ss = 0.0;
  strip_zero(Bs);
  strip_mul<KS, KW, RB>(Rpm, lr, lq, rT, Bs, wave);
  if (colok) {
#pragma unroll
    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        if (strip_rowok<KS>(rt, rr, lq)) ss += Bs[rt][rr] * Bs[rt][rr];
  }
  {
    r4 tT[NT];
    strip_load_lds<KS>(t, lr, lq, c0, tT);
    strip_zero(W0);
    strip_mul<KS, KW, RB>(Rpm, lr, lq, tT, W0, wave);
  }
  __syncthreads();  // every wave is done with R+-
  real *B = r;      // B replaces R+-
  strip_store_lds<KS>(B, lr, lq, c0, colok, Bs);
  wg_sumsq_put(c, ss);
  __syncthreads();
  const real beta2 = wg_sumsq_get(c);
  const int p = __builtin_amdgcn_readfirstlane(neumann_terms_12(beta2));
  if (p > kStripMaxP) {
    s2_chain<false, PRIO>(c, S2_SEC_ICH1, fav);
    return false;
  }
  const unsigned mask = strip_sign_mask(c.sg, lq, N);
  // ---- (b) the two Horner loops, multiplier B^T
  r4 Y1[NT], Y2[NT];
  strip_copy(Y2, W0);
#pragma nounroll
  for (int k = 1; k < p; ++k) {  // Y2 <- W0 + B^T Y2 : X^T
    r4 acc[NT];
    strip_copy(acc, W0);
    strip_mul<KS, KW, RB>(B, lr, lq, Y2, acc, wave);
    strip_copy(Y2, acc);
  }
  {
    r4 T1[NT];
    strip_load_glb<KS>(g.T_mm, lr, lq, c0, colok, T1);
    strip_copy(Y1, T1);
#pragma nounroll
    for (int k = 1; k < p; ++k) {  // Y1 <- T--^T + B^T Y1 : T01^T
      r4 acc[NT];
      strip_copy(acc, T1);
      strip_mul<KS, KW, RB>(B, lr, lq, Y1, acc, wave);
      strip_copy(Y1, acc);
    }
  }
  __syncthreads();  // every wave is done with B
  // ---- (c) r back (riding column N = j0-); the products with r and t
  strip_store_lds<KS>(r, lr, lq, c0, colok, rT);
  for (int i = wg_tid(); i < N; i += kThreads) r[i + N * LD] = c.jm[i];
  __syncthreads();
  {  // T-- = T01 t--  ->  (t--)^T T01^T = D t^T D Y1                                   (:96)
    r4 Yf[NT], o[NT];
    strip_copy(Yf, Y1);
    strip_flip(Yf, mask);
    strip_zero(o);
    strip_mul<KS, KW, RB>(t, lr, lq, Yf, o, wave);
    strip_flip(o, mask);
    strip_store_glb<KS>(g.T_mm, lr, lq, c0, colok, o);
  }
  // V = (T01 r-+)^T = r-+^T Y1 ; row N: (T01 j0-)^T
  r4 V[NT];
  strip_zero(V);
  strip_mul<KS, KW, RB>(r, lr, lq, Y1, V, wave);
  // T21^T = t++^T + r-+^T X^T ; row N: (X j0-)^T
  r4 T21[NT];
  strip_load_lds<KS>(t, lr, lq, c0, T21);
  strip_mul<KS, KW, RB>(r, lr, lq, Y2, T21, wave);
  {  // R+- = r+- + X t--  ->  D (D r+-^T + t^T D X^T), D r+-^T[row][col] = sg[col] r-+[col][row]   (:116)
    r4 acc[NT];
    const real sc = colok ? c.sg[col] : 1.0;
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) acc[rt] = rT[rt] * sc;
    strip_flip(Y2, mask);
    strip_mul<KS, KW, RB>(t, lr, lq, Y2, acc, wave);
    strip_flip(acc, mask);
    strip_store_glb<KS>(g.R_pm, lr, lq, c0, colok, acc);
  }
  s2_chain<false, PRIO>(c, S2_SEC_ICH1, fav);
  if constexpr (SRC) {
    // ---- (d), sources only: neither R-+ nor T++ is loaded, staged or stored.  J0+ alone goes to column N of t's buffer, and the
    // two riding rows the sources take from the products with T++ -- J0+^T V and J0+^T T21^T -- are formed on their own
    const real j0m = (colok && lq == G::LQ0) ? g.J0m[col] : 0.0;
    const real vj = (wg_tid() < N) ? g.J0p[wg_tid()] : 0.0;
    __syncthreads();  // every wave is done with t
    if (wg_tid() < N) t[wg_tid() + N * LD] = vj;
    __syncthreads();
    s2_chain<true, PRIO>(c, S2_SEC_ICOPY2, fav);
    real ride1 = 0.0, ride2 = 0.0;
    strip_ride<KS, KW>(t, lr, lq, V, ride1, wave);    // row N: (T01 r-+ J0+)^T
    // J0- = J0- + T01 (r-+ J0+ + j0-)                                                (:90)
    if (colok && lq == G::LQ0) g.J0m[col] = j0m + (ride1 + V[G::RT][G::RR0]);
    strip_ride<KS, KW>(t, lr, lq, T21, ride2, wave);  // row N: (T21 J0+)^T
    // J0+ = j0+ + T21 (J0+ + R+- j0-)                                                (:110)
    if (colok && lq == G::LQ0) g.J0p[col] = c.jp[col] + (ride2 + T21[G::RT][G::RR0]);
    s2_chain<false, PRIO>(c, S2_SEC_ICH2, fav);
    __syncthreads();
    MOM_TL(c, S2_SEC_IEND);
    return true;
  }
  // ---- (d) T++ (+ J0+ as its riding column N) into t's buffer; the products with T++
  r4 Radd[NT];
  strip_load_glb<KS>(g.R_mp, lr, lq, c0, colok, Radd);
  const real j0m = (colok && lq == G::LQ0) ? g.J0m[col] : 0.0;
  {
    real vt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = wg_tid() + u * kThreads;
      if (e < NN) {
        int i, j;
        c.fd.split(e, i, j);
        vt[u] = MOM_NT_LOAD(g.T_pp + i + j * G::CP);
      }
    }
    const real vj = (wg_tid() < N) ? g.J0p[wg_tid()] : 0.0;
    __syncthreads();  // every wave is done with t
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = wg_tid() + u * kThreads;
      if (e < NN) {
        int i, j;
        c.fd.split(e, i, j);
        t[i + j * LD] = vt[u];
      }
    }
    if (wg_tid() < N) t[wg_tid() + N * LD] = vj;
  }
  __syncthreads();
  s2_chain<true, PRIO>(c, S2_SEC_ICOPY2, fav);
  const real *Tpp = t;
  // R-+ = R-+ + (T01 r-+) T++  ->  R-+^T + T++^T V ; row N: (T01 r-+ J0+)^T        (:93)
  strip_mul<KS, KW, RB>(Tpp, lr, lq, V, Radd, wave);
  strip_store_glb<KS>(g.R_mp, lr, lq, c0, colok, Radd);
  // J0- = J0- + T01 (r-+ J0+ + j0-)                                                (:90)
  if (colok && lq == G::LQ0) g.J0m[col] = j0m + (Radd[G::RT][G::RR0] + V[G::RT][G::RR0]);
  // T++ = T21 T++  ->  T++^T T21^T ; row N: (T21 J0+)^T                            (:113)
  {
    r4 o[NT];
    strip_zero(o);
    strip_mul<KS, KW, RB>(Tpp, lr, lq, T21, o, wave);
    strip_store_glb<KS>(g.T_pp, lr, lq, c0, colok, o);
    // J0+ = j0+ + T21 (J0+ + R+- j0-)                                                (:110)
    if (colok && lq == G::LQ0) g.J0p[col] = c.jp[col] + (o[G::RT][G::RR0] + T21[G::RT][G::RR0]);
  }
  s2_chain<false, PRIO>(c, S2_SEC_ICH2, fav);
  __syncthreads();
  MOM_TL(c, S2_SEC_IEND);
  return true;
}

// One launch walks all layers of every unit (sweep mode only); see the header of this file for what it does not do.
// MODE = the bits of MomLaunchForm::sched_mode, one instantiation each: without bit 0 the unit loop is the fixed stride, without bit 1
// no chain boundary emits anything, so MODE 0 is the kernel as it was before the option existed.
// KW < KS (MOM_OPT_ZERO_SKIP bit 1; the host picks it from MomLaunchForm::nbw, mom_image_variants.hpp): every strip product of the
// image runs KW k-steps and the diagonal fix-up (mom_strip.hpp strip_diag_fixup), strip index = wave.  Only the products change:
// Frobenius sums, series lengths, resume decisions, stores and the elemental layer are those of KW = KS.
// RB (MOM_OPT_ZERO_SKIP bit 2; default mode only): every strip product follows the row-block rule of mom_strip.hpp strip_mul -- the
// row tiles that hold rows of zero-weight streams or rows past the riding rows run v_mfma_f64_4x4x4_4b on their live blocks of four
// rows.  The strip rows that keep their incoming value under it are read by nothing: the stores and the Frobenius sums are guarded
// by strip_rowok (rows < N), strip_flip only changes signs, the riding rows N, N + 1 lie in a live block, and a strip's rows >= N
// never are a B operand (KS k-steps at most).
// SRC (MOM_OPT_SOURCES_ONLY; default mode only; MomLaunchForm::sources_only): the sources-only form of the
// interaction, see the header of this file.  SRC = false is the kernel as it was before the option existed.
// EL (MOM_OPT_ELEMENTAL; default mode only; MomLaunchForm::elemental_tab): the table form of the elemental layer
// (mom_elemental_tab.hpp).  The host asks for it only where the form applies to the launch (mom_elemental_tab_applies: regular
// streams, their tables, two bases); any other launch takes EL = false, the kernel as it was before the option existed.
template <int KS, int MODE, int KW = KS, bool RB = false, bool SRC = false, bool EL = false>
__global__ void __launch_bounds__(kThreads, 2) k_layer_s2(const LayerArgs a) {
  // (the argument block is never written: see k_layer_lean)
  constexpr int N = 4 * KS;
  constexpr bool QUEUE = (MODE & 1) != 0, PRIO = (MODE & 2) != 0;
  const size_t total = (size_t)a.S * a.M;
  Ctx c;
  make_ctx_s2(c, N, a.q.inv_mode, a.q.regular ? a.q.nS : 1, mom_smem);
  zero_padding<true>(c);
  __syncthreads();
  load_streams(c, a.q);
  __syncthreads();
  real *lay = mom_smem + 2 * mat_elems(N) + s2_vec_reals(N);
  const int nz = a.Nz_sweep;
  const int LW = 3 + a.K, LZ = kS2Lay / LW;
  // (c.ipiv, c.sh serve the pivoted inverse, which this image never runs: c.ipiv[0], [1] carry the tickets to the other waves)
  if (PRIO && wg_tid() == 0) c.ipiv[1] = atomicAdd(a.sched + 1 + s2_cu_key(), 1);  // odd: the favoured workgroup
#ifdef MOM_DIAG_TIMELINE
  if (!PRIO && wg_tid() == 0) c.ipiv[1] = 0;
  if (wg_tid() == 0) c.ipiv[2] = -1;
  int tl_units = 0;
#endif
  for (size_t pt = blockIdx.x;; pt += gridDim.x) {
    if constexpr (QUEUE) {  // the next unit nobody has taken: thread 0 draws the ticket and hands it to the other waves through LDS
      if (wg_tid() == 0) c.ipiv[0] = atomicAdd(a.sched, 1);
      __syncthreads();
      pt = S2_UNIT(c);
    }
    if (pt >= total) break;
#ifdef MOM_DIAG_TIMELINE
    if (wg_tid() == 0 && tl_units == 1) c.ipiv[2] = 0;
    ++tl_units;
    MOM_TL(c, S2_SEC_TOP);
#endif
    const size_t NNs = (size_t)N * N;
    int done = nz;
    for (int z = 0; z < nz; ++z) {
      // QUEUE: the unit index is read from LDS again wherever a layer needs it.  Held in scalar registers across the layer loop,
      // it and what derives from it (n, the moment, six composite pointers) cost the register allocator the room it needs to
      // keep the kernel free of scratch; the fixed stride does not, there the compiler re-derives them from blockIdx.
      if constexpr (QUEUE) pt = S2_UNIT(c);
      const int n = (int)(pt % a.S), mrel = (int)(pt / a.S), m = a.m_first + mrel;
      const int zl = z % LZ;
      if (zl == 0) {
        const int cnt = ((nz - z < LZ) ? nz - z : LZ) * LW;
        for (int i = wg_tid(); i < cnt; i += kThreads) {
          const int zz = i / LW, k = i - zz * LW;
          const size_t o = (size_t)n + (size_t)a.S * (z + zz);
          lay[i] = (k == 0) ? as_global(a.tau)[o] : (k == 1) ? as_global(a.varpi)[o] : (k == 2) ? as_global(a.tau_sum)[o]
                                                                                                : as_global(a.zw)[(size_t)a.K * o + (k - 3)];
        }
        __syncthreads();
      }
      const int nd = a.nd_z[z];
      const bool first = (z == 0) && (a.first != 0);
      const real *ls = lay + zl * LW;
      const real tau = ls[0], varpi = ls[1], tau_sum = ls[2];
      const real dtau = ldexp(tau, -nd);         // τ ./ 2^ndoubl   (rt_kernel.jl:244)
      real expk = exp(-dtau / a.q.mu0);          // init_layer      (rt_kernel.jl:273)
      ZMix zpp{as_global(a.Zpp) + NNs * a.K * mrel, ls + 3, a.K, N};
      ZMix zmp{as_global(a.Zmp) + NNs * a.K * mrel, ls + 3, a.K, N};
      if constexpr (EL) elemental_build_tab<true, 2, N, StripGeom<KS>::LD>(c, a.q, a.etab, m, nd, tau_sum, dtau, varpi, zpp, zmp);
      else elemental_build<true>(c, a.q, m, nd, tau_sum, dtau, varpi, zpp, zmp);
      bool bail;
      expk = doubling_run_s2<KS, PRIO, KW, RB>(c, nd, expk, bail);
      if (!bail) {
        if constexpr (QUEUE) pt = S2_UNIT(c);
        const CompPtrs g = comp_ptrs(a.comp, N, comp_pitch(N), pt);
        if (first) {
          store_added_as_composite(c, g);
          __syncthreads();
          MOM_TL(c, S2_SEC_FIRST);
        } else {
          bail = !interaction_strip_s2<KS, PRIO, KW, RB, SRC>(c, g);
        }
      }
      if (bail) {  // workgroup-uniform: the 8-wave image redoes this layer and finishes the unit
        done = z;
        __syncthreads();
        break;
      }
    }
    if constexpr (QUEUE) pt = S2_UNIT(c);
    if (wg_tid() == 0) a.resume[pt] = done;
    if constexpr (QUEUE) __syncthreads();  // every wave has read this unit's ticket before thread 0 draws the next one
  }
  if (wg_tid() == 0 && *c.bad) atomicMax(a.info, *c.bad);
#ifdef MOM_DIAG_TIMELINE
  if (wg_tid() == 0 && blockIdx.x < kTlWgs) {
    unsigned *hd = mom_tl_hdr + 4 * blockIdx.x;
    hd[0] = (unsigned)s2_cu_key();
    hd[1] = (unsigned)c.ipiv[1];
    hd[2] = (unsigned)(c.ipiv[1] & 1);
    hd[3] = (unsigned)(c.ipiv[2] < 0 ? 0 : c.ipiv[2]);
  }
#endif
}

}  // namespace MOM_NS
