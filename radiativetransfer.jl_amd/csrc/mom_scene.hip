// mom_scene.hip -- the scene-level part of the C ABI (include/momcore.h): mom_scene_set and the surface, the single-launch
// runs, the layer-launch policy over the image table, rt_run_core, mom_rt_run, mom_rt_run_multisensor, the Dual run's entry
// points, the getters.  Handle and shared helpers: mom_handle.hpp.
#include "mom_handle.hpp"
#include "mom_elemental_tab.hpp"
#include "mom_images.hpp"
#include "mom_reduce.hpp"

using namespace mom;

// postprocessing_vza! (postprocessing_vza.jl:9-60, SFI branch) and postprocessing_vza_hdrf! (:63-93), all
// moments in m order.  With the m = 0 reduction (see mom_scene_set) the m = 0 sources live in their own
// arrays with N0 = nS0 * Nquad rows; Stokes components >= nS0 get no m = 0 contribution (it is exactly 0).
struct PostArgs {
  int N, nS, S, M, nVza, red0, N0, nS0;
  int hdr_all;   // BRDF surfaces: hdr_J0- exists for every moment (hdrJm), not only m = 0
  int zeroT_hi;  // LambertianSurfaceLegendre: t++ = t-- = 0 for m > 0 (lambertian_surface.jl:131-132) -> J0+ = 0 there
  const int *node;
  const double *cos_mphi, *sin_mphi;
  const double *J0p, *J0m;    // [N,S,M] (moment 0 slice unused when red0)
  const double *J0p0, *J0m0;  // [N0,S] when red0
  const double *hdrJ;         // m = 0: [N,S] or [N0,S] when red0
  const double *hdrJm;        // hdr_all: [N,S,M] (slot 0 unused)
  double *R, *T, *hdr;
};
__global__ void k_postprocess(PostArgs a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)a.nVza * a.nS * a.S;
  if (idx >= total) return;
  const int v = (int)(idx % a.nVza);
  const int k = (int)((idx / a.nVza) % a.nS);
  const size_t s = idx / ((size_t)a.nVza * a.nS);
  const int row = (a.node[v] - 1) * a.nS + k;
  double r = 0.0, t = 0.0, h = 0.0;
  for (int m = 0; m < a.M; ++m) {
    const double weight = (m == 0) ? 0.5 : 1.0;
    const double cs = weight * ((k < 2) ? a.cos_mphi[v + (size_t)a.nVza * m] : a.sin_mphi[v + (size_t)a.nVza * m]);
    if (m == 0 && a.red0) {
      if (k < a.nS0) {
        const size_t o = (size_t)(a.node[v] - 1) * a.nS0 + k + (size_t)a.N0 * s;
        r += cs * a.J0m0[o];
        t += cs * a.J0p0[o];
        h += cs * a.hdrJ[o];
      }
    } else {
      const size_t o = row + (size_t)a.N * (s + (size_t)a.S * m);
      r += cs * a.J0m[o];
      if (!(a.zeroT_hi && m > 0)) t += cs * a.J0p[o];
      if (m == 0) h += cs * a.hdrJ[row + (size_t)a.N * s];
      else if (a.hdr_all) h += cs * a.hdrJm[o];
    }
  }
  a.R[idx] = r;
  a.T[idx] = t;
  a.hdr[idx] = h;  // Lambertian surfaces: only m = 0 contributes (r-+ = 0, j0- = 0 for m > 0)
}

// MOM_OPT_ELEMENTAL: the layer-independent stream-pair tables of the elemental layer, once per stream set instead of once per layer
// and unit: out = SI | F1 | F2, [3][Nq][Nq], entry iq + jq Nq, with the very expressions of elemental_build (mom_kernels.hpp) on the
// stream values mu[iq ns] it reads -- on the device, so that they are the same instructions
__global__ void k_stream_tables(const double *mu, int ns, int Nq, double *out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Nq * Nq) return;
  const int jq = e / Nq, iq = e - jq * Nq;
  const double mui = mu[iq * ns], muj = mu[jq * ns];
  out[e] = (1 / mui) + (1 / muj);
  out[Nq * Nq + e] = muj / (mui + muj);
  out[2 * Nq * Nq + e] = muj / (mui - muj);
}
// the tables of stream set q into `buf`, where the table form can apply to it (regular streams, an edge of whole streams); else none
static int stream_tables(mom_t *h, const DevStreams &q, MomDevBuf<double> &buf) {
  buf.reset();
  if (!q.regular || q.nS < 1 || q.N % q.nS != 0) return MOM_OK;
  const int Nq = q.N / q.nS;
  HIPCHK(h, buf.renew(3 * (size_t)Nq * Nq));
  hipLaunchKernelGGL(k_stream_tables, dim3((Nq * Nq + 255) / 256), dim3(256), 0, h->stream, q.mu, q.nS, Nq, buf.get());
  HIPCHK(h, hipGetLastError());
  return MOM_OK;
}

// the edges that have a strip-chained finisher, of the 4-wave or the 8-wave build (the pad rule: mom_host.hpp)
static bool strip_size(int N) { return mom_find_image(MOM_IMG_STRIP4, N) || mom_find_image(MOM_IMG_STRIP8, N); }
static int strip_pad(int N) { return mom_strip_pad(strip_size, N); }

// ---- Greek coefficients staged on the handle: the Z bases are formed where the kernels read them (mom_zmom.hip) -------------
// one mu per stream of the handle's quadrature (mom_set_streams): entry i nS of h_mu
static std::vector<double> stream_mu(const mom_t *h) {
  std::vector<double> mu((size_t)(h->N / h->nS));
  for (size_t i = 0; i < mu.size(); ++i) mu[i] = h->h_mu[i * h->nS];
  return mu;
}
// what both staging calls check and copy: the handle's state, the Greek sets against the handle's streams (mom_z_moments' checks)
static int stage_greeks(mom_t *h, const char *fn, MomGreekStage &st, int nG, int l_pad, const int *l_max, const double *greek, int M) {
  const std::string f(fn);
  if (h->dtype != 0) return fail(h, MOM_EUNSUPPORTED, (f + ": Greek coefficients are staged on Float64 handles only").c_str());
  if (!h->streams_set) return fail(h, MOM_ESTATE, (f + ": call mom_set_streams first").c_str());
  if (h->N % h->nS != 0) return fail(h, MOM_EINVAL, (f + ": the operator edge is not a whole number of streams").c_str());
  if (M > h->M) return fail(h, MOM_EINVAL, (f + ": more moments than the handle was created for").c_str());
  const std::vector<double> mu = stream_mu(h);
  if (const char *bad = mom_zmom_check(h->nS, (int)mu.size(), mu.data(), nG, l_pad, l_max, greek, 0, M))
    return fail(h, MOM_EINVAL, (f + ": " + bad).c_str());
  st.drop();
  st.nG = nG; st.l_pad = l_pad; st.M = M;
  st.l_max.assign(l_max, l_max + nG);
  st.greek.assign(greek, greek + (size_t)nG * 6 * l_pad);
  st.live = true;
  return MOM_OK;
}

extern "C" int mom_scene_stage_greeks(mom_t *h, int which, int nG, int l_pad, const int *l_max, const double *greek, int M) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (which != 0 && which != 1) return fail(h, MOM_EINVAL, "mom_scene_stage_greeks: which must be 0 (elastic bases) or 1 (the Raman set)");
  if (which == 0 && nG > 64) return fail(h, MOM_EINVAL, "mom_scene_stage_greeks: at most 64 phase-matrix bases");
  if (which == 1 && nG != 1) return fail(h, MOM_EINVAL, "mom_scene_stage_greeks: the Raman stage is one Greek set (nG = 1)");
  return stage_greeks(h, "mom_scene_stage_greeks", which ? h->stage_r : h->stage_z, nG, l_pad, l_max, greek, M);
}

extern "C" int mom_scene_stage_greek_partials(mom_t *h, int P, int nD, const int *basis, const int *partial, int l_pad,
                                              const int *l_max, const double *dgreek) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const char *fn = "mom_scene_stage_greek_partials";
  if (P < 1 || P > 64 || nD < 1 || !basis || !partial) return fail(h, MOM_EINVAL, "mom_scene_stage_greek_partials: 1 <= P <= 64, nD >= 1, basis and partial given");
  for (int d = 0; d < nD; ++d) {
    if (basis[d] < 0 || basis[d] >= 64 || partial[d] < 0 || partial[d] >= P)
      return fail(h, MOM_EINVAL, "mom_scene_stage_greek_partials: basis within 0..63 and partial within 0..P-1");
    for (int e = 0; e < d; ++e)
      if (basis[e] == basis[d] && partial[e] == partial[d]) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: the pair (basis %d, partial %d) is named twice", fn, basis[d], partial[d]);
        return fail(h, MOM_EINVAL, buf);
      }
  }
  MomGreekStage st;
  const int rc = stage_greeks(h, fn, st, nD, l_pad, l_max, dgreek, 1);  // the moments are the scene's, known at the setter
  if (rc) return rc;
  st.P = P;
  st.basis.assign(basis, basis + nD);
  st.partial.assign(partial, partial + nD);
  h->stage_d = std::move(st);
  return MOM_OK;
}

int mom_stage_claim(mom_t *h, const char *fn, int K, int M) {
  const MomGreekStage &st = h->stage_z;
  char buf[256];
  if (!st.live) {
    snprintf(buf, sizeof buf, "%s: bad argument", fn);
    return fail(h, MOM_EINVAL, buf);
  }
  if (st.nG == K && st.M == M) return MOM_OK;
  snprintf(buf, sizeof buf, "%s: K = %d, M = %d, but the staged Greek sets (mom_scene_stage_greeks) are K = %d, M = %d", fn, K, M, st.nG, st.M);
  return fail(h, MOM_EINVAL, buf);
}

// scene_common's staged case: d_Zpp / d_Zmp [Nk, Nk, K, M] and, for N0 > 0 (the host half of the m = 0 condition holds), d_Zpp0 /
// d_Zmp0 [N0, N0, K], zeroed and written on the handle's stream; *red_ok ends up false when a moment-0 block couples (I,Q) with (U,V)
static int stage_bases(mom_t *h, int K, int M, int Nk, int N0, bool *red_ok) {
  MomGreekStage st = std::move(h->stage_z);
  h->stage_z.drop();
  if (!st.live || st.nG != K || st.M != M) return fail(h, MOM_EINVAL, "the scene's setter: no staged Greek sets of this K and M");
  const std::vector<double> mu = stream_mu(h);
  std::vector<int> slot((size_t)K * M);
  for (size_t e = 0; e < slot.size(); ++e) slot[e] = (int)e;  // [Nk, Nk, K, M]: block k + K m
  const size_t nZ = (size_t)Nk * Nk * K * M, nZ0 = (size_t)N0 * N0 * K;
  MomZmomPlan pl;
  HIPCHK(h, mom_zmom_plan(pl, h->nS, (int)mu.size(), mu.data(), K, st.l_pad, st.l_max.data(), st.greek.data(), 0, M, slot.data(), h->stream));
  HIPCHK(h, h->d_Zpp.renew(nZ));
  HIPCHK(h, h->d_Zmp.renew(nZ));
  if (Nk != h->N) {  // strip_pad's dummy entries: exact zeros
    HIPCHK(h, hipMemsetAsync(h->d_Zpp, 0, nZ * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_Zmp, 0, nZ * sizeof(double), h->stream));
  }
  if (N0 > 0) {
    HIPCHK(h, h->d_Zpp0.renew(nZ0));
    HIPCHK(h, h->d_Zmp0.renew(nZ0));
    HIPCHK(h, hipMemsetAsync(h->d_Zpp0, 0, nZ0 * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_Zmp0, 0, nZ0 * sizeof(double), h->stream));
  }
  HIPCHK(h, mom_zmom_launch(pl, h->stream, h->d_Zpp, h->d_Zmp, Nk, N0 > 0 ? h->d_Zpp0.get() : nullptr, N0 > 0 ? h->d_Zmp0.get() : nullptr, N0));
  int coupled = 0;
  if (N0 > 0) HIPCHK(h, mom_zmom_couples(pl, h->stream, K, h->d_Zpp, h->d_Zmp, Nk, &coupled));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the plan and the stage go out of scope
  if (coupled) {
    *red_ok = false;
    h->d_Zpp0.reset(); h->d_Zmp0.reset();
  }
  return MOM_OK;
}

extern "C" int mom_scene_set(mom_t *h, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                             const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface,
                             const double *tau_sum, double albedo, int nVza, const int *node_1based,
                             const double *cos_mphi, const double *sin_mphi) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_scene_set: call mom_set_streams first");
  if (Nz <= 0 || K <= 0 || M <= 0 || M > h->M || nVza <= 0 || !tau || !varpi || !zw || (Zpp == nullptr) != (Zmp == nullptr) || !ndoubl ||
      !iface || !tau_sum || !node_1based || !cos_mphi || !sin_mphi)
    return fail(h, MOM_EINVAL, "mom_scene_set: bad argument");
  if (!Zpp) {  // the staged bases (mom_scene_stage_greeks), if any
    const int rc = mom_stage_claim(h, "mom_scene_set", K, M);
    if (rc) return rc;
  }
  if (K > 64) return fail(h, MOM_EINVAL, "mom_scene_set: at most 64 phase-matrix bases (Rayleigh + aerosol types)");
  for (int z = 0; z < Nz; ++z)
    if (ndoubl[z] < 0 || ndoubl[z] > 60 || iface[z] < 0 || iface[z] > 3)
      return fail(h, MOM_EINVAL, "mom_scene_set: ndoubl/iface out of range");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = h->S;
  h->scene_set = false;
  h->optics_scene = false;  // host optics: no ingredients for mom_scene_set_optics_partials
  int rc;
  if (h->f32) {
    for (int v = 0; v < nVza; ++v)
      if (node_1based[v] < 1 || node_1based[v] * h->nS > h->N) return fail(h, MOM_EINVAL, "mom_scene_set: bad view node");
    if ((rc = momf_scene_set(h->f32, Nz, K, M, tau, varpi, zw, Zpp, Zmp, ndoubl, iface, tau_sum, albedo, nVza, node_1based,
                             cos_mphi, sin_mphi)))
      return fail(h, rc, momf_error(h->f32));
    h->Nz = Nz; h->K = K; h->scene_M = M; h->nVza = nVza; h->albedo = albedo; h->surf_kind = 0;
    h->nd.assign(ndoubl, ndoubl + Nz);
    h->iface.assign(iface, iface + Nz);
    h->scene_set = true;
    return MOM_OK;
  }
  HIPCHK(h, mom_upload(h->d_tau, tau, S * Nz, h->stream));
  HIPCHK(h, mom_upload(h->d_varpi, varpi, S * Nz, h->stream));
  HIPCHK(h, mom_upload(h->d_zw, zw, (size_t)K * S * Nz, h->stream));
  HIPCHK(h, mom_upload(h->d_tau_sum, tau_sum, S * (Nz + 1), h->stream));
  if ((rc = scene_common(h, Nz, K, M, Zpp, Zmp, albedo, nVza, node_1based, cos_mphi, sin_mphi))) return rc;
  h->nd.assign(ndoubl, ndoubl + Nz);
  h->iface.assign(iface, iface + Nz);
  h->scene_set = true;
  return MOM_OK;
}

int scene_common(mom_t *h, int Nz, int K, int M, const double *Zpp, const double *Zmp, double albedo, int nVza,
                 const int *node_1based, const double *cos_mphi, const double *sin_mphi) {
  for (int v = 0; v < nVza; ++v)
    if (node_1based[v] < 1 || node_1based[v] * h->nS > h->N) return fail(h, MOM_EINVAL, "mom_scene_set: bad view node");
  const size_t S = h->S, NN = (size_t)h->N * h->N;
  // a new scene: the partials of the previous one (mom_scene_set_partials) do not belong to it, nor does a staged partial set
  for (auto &b : h->d_dual_in) b.reset();
  h->dual_P = 0; h->dual_ran = false;
  h->stage_d.drop();
  // (edges up to 32 belong to the wave-per-point kernel, which takes the operators as they are)
  const int Nk = (h->opt_pad && !(h->N <= 32 && h->opt_small)) ? strip_pad(h->N) : h->N;
  h->Nk = Nk;
  h->qk = h->q;
  h->qk.N = Nk;
  h->nbw_0 = 0;
  // ---- m = 0 reduction (include/momcore.h): conditions checked on the data, bitwise.  The options, the source and the N <= 4 route
  // are decided here; the data are the host's arrays, or for staged bases (Zpp == nullptr) what the device formed (stage_bases)
  const bool staged = !Zpp;
  bool red_ok = h->opt_m0 && h->nS >= 3 && h->q.regular && !(h->N <= 4 && h->opt_small && nVza <= 4 && K <= 4) &&
                (staged ? mom_m0_source(h->q.I0, h->nS) : mom_m0_reducible(h->q.I0, h->N, h->nS, K, Zpp, Zmp));
  int N0 = 0;
  if (red_ok) {
    // N0r real entries; the kernels run on N0 >= N0r (dummy entries of strip_pad at the end: mu = 1, weight 0, Z = 0)
    const int N0r = mom_m0_edge(h->N, h->nS);
    N0 = h->opt_pad ? strip_pad(N0r) : N0r;
    // r6: sub-problems of edge 18 .. 30 that are not a multiple of 4 take ONE dummy stream (two entries) to reach a quad-block
    // size (20, 24, 28, 32: mom_q4.hpp; IQUV scenes of 9 .. 15 streams)
    if (h->opt_pad && h->opt_lean >= 3 && N0 == N0r && N0r > 16 && N0r < 32 && (N0r % 4) != 0) N0 = N0r + 2;
  }
  for (MomDevBuf<double> *b : {&h->d_mu0, &h->d_wt0, &h->d_sg0, &h->d_Zpp0, &h->d_Zmp0, &h->d_hdrJ0, &h->d_scratch0}) b->reset();
  if (staged) {
    const int rc = stage_bases(h, K, M, Nk, N0, &red_ok);
    if (rc) return rc;
  } else if (Nk == h->N) {
    HIPCHK(h, mom_upload(h->d_Zpp, Zpp, NN * K * M, h->stream));
    HIPCHK(h, mom_upload(h->d_Zmp, Zmp, NN * K * M, h->stream));
  } else {
    const std::vector<double> zp = mom_pad_blocks(Zpp, h->N, Nk, (size_t)K * M), zm = mom_pad_blocks(Zmp, h->N, Nk, (size_t)K * M);
    HIPCHK(h, mom_upload(h->d_Zpp, zp.data(), zp.size(), h->stream));
    HIPCHK(h, mom_upload(h->d_Zmp, zm.data(), zm.size(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the padded host copies go out of scope
  }
  HIPCHK(h, mom_upload(h->d_node, node_1based, (size_t)nVza, h->stream));
  HIPCHK(h, mom_upload(h->d_cos, cos_mphi, (size_t)nVza * M, h->stream));
  HIPCHK(h, mom_upload(h->d_sin, sin_mphi, (size_t)nVza * M, h->stream));
  h->d_R.reset(); h->d_hdr.reset(); h->d_T = nullptr;
  // R_SFI || T_SFI in ONE buffer: it is the send buffer of the all-gather (mom_allgather_RT) as it stands
  HIPCHK(h, h->d_R.renew(2 * (size_t)nVza * h->nS * S));
  h->d_T = h->d_R + (size_t)nVza * h->nS * S;
  HIPCHK(h, h->d_hdr.renew((size_t)nVza * h->nS * S));
  if (!h->d_hdrJ) {
    HIPCHK(h, h->d_hdrJ.renew((size_t)(h->N + kMomPadMax) * S));
    HIPCHK(h, h->d_bhr_uw.renew((size_t)h->nS * S));
    HIPCHK(h, h->d_bhr_dw.renew((size_t)h->nS * S));
  }
  {  // the (I,Q) sub-problem of a reducible scene: its streams, composite state and scratch (its bases: above)
    const int N = h->N, nS = h->nS;
    const bool ok = red_ok;
    for (auto &b : h->comp0) b.reset();
    h->red0 = ok;
    if (ok) {
      const int nS0 = kMomM0Stokes;
      h->N0 = N0; h->nS0 = nS0;
      const MomM0Cut cut = staged ? mom_m0_cut_streams(h->h_mu.data(), h->h_wt.data(), N, nS, N0)
                                  : mom_m0_cut(h->h_mu.data(), h->h_wt.data(), N, nS, K, N0, Zpp, Zmp);
      h->nbw_0 = mom_q4_nbw(cut.wt.data(), N0);  // after the reduction to (I,Q) and the padding
      HIPCHK(h, mom_upload(h->d_mu0, cut.mu.data(), (size_t)N0, h->stream));
      HIPCHK(h, mom_upload(h->d_wt0, cut.wt.data(), (size_t)N0, h->stream));
      HIPCHK(h, mom_upload(h->d_sg0, cut.sg.data(), (size_t)N0, h->stream));
      if (!staged) {
        HIPCHK(h, mom_upload(h->d_Zpp0, cut.Zpp.data(), cut.Zpp.size(), h->stream));
        HIPCHK(h, mom_upload(h->d_Zmp0, cut.Zmp.data(), cut.Zmp.size(), h->stream));
      }
      for (int k = 0; k < 6; ++k) {
        const size_t cnt = ((k < 4) ? (size_t)comp_pitch(N0) * N0 : (size_t)N0) * S;
        HIPCHK(h, h->comp0[k].renew(cnt));
        HIPCHK(h, hipMemsetAsync(h->comp0[k], 0, cnt * sizeof(double), h->stream));
      }
      HIPCHK(h, h->d_hdrJ0.renew((size_t)N0 * S));
      const size_t scr = (size_t)h->G * kGenericBufs * mat_elems(N0) + (size_t)ld_for(N0) * np_for(N0);
      HIPCHK(h, h->d_scratch0.renew(scr));
      HIPCHK(h, hipMemsetAsync(h->d_scratch0, 0, scr * sizeof(double), h->stream));
      HIPCHK(h, hipMemsetAsync(h->d_bhr_uw, 0, (size_t)h->nS * S * sizeof(double), h->stream));
      HIPCHK(h, hipMemsetAsync(h->d_bhr_dw, 0, (size_t)h->nS * S * sizeof(double), h->stream));
      DevStreams &q0 = h->q0;
      q0 = h->q;
      q0.mu = h->d_mu0; q0.wt = h->d_wt0; q0.sg = h->d_sg0;
      q0.N = N0; q0.nS = nS0;
      for (int k = nS0; k < 4; ++k) { q0.I0[k] = 0.0; q0.D[k] = 1.0; }
    }
  }
  {  // MOM_OPT_ELEMENTAL: the stream-pair tables of both stream sets, behind the uploads of their stream values on the same stream
    int rc;
    if ((rc = stream_tables(h, h->qk, h->d_etab))) return rc;
    h->d_etab0.reset();
    if (h->red0 && (rc = stream_tables(h, h->q0, h->d_etab0))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->Nz = Nz; h->K = K; h->scene_M = M; h->nVza = nVza; h->albedo = albedo;
  h->surf_kind = 0;  // LambertianSurfaceScalar(albedo) until mom_scene_set_surface says otherwise
  return MOM_OK;
}

extern "C" int mom_scene_set_surface(mom_t *h, int kind, int M, const double *Rsurf, const double *albedo_spec) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_scene_set_surface: call mom_scene_set first");
  if (kind < 0 || kind > 2 || (kind == 1 && (!Rsurf || M != h->scene_M)) || (kind == 2 && !albedo_spec))
    return fail(h, MOM_EINVAL, "mom_scene_set_surface: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  const int N = h->N, nS = h->nS;
  const size_t NN = (size_t)N * N, S = h->S;
  int rc;
  if (h->f32) {
    if ((rc = momf_scene_set_surface(h->f32, kind, M, Rsurf, albedo_spec))) return fail(h, rc, momf_error(h->f32));
    h->surf_kind = kind;
    return MOM_OK;
  }
  if (kind == 1) {
    if (h->Nk == N) {
      HIPCHK(h, mom_upload(h->d_Rsurf, Rsurf, NN * M, h->stream));
    } else {
      const std::vector<double> rp = mom_pad_blocks(Rsurf, N, h->Nk, (size_t)M);
      HIPCHK(h, mom_upload(h->d_Rsurf, rp.data(), rp.size(), h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, h->d_hdrJm.renew((size_t)h->Nk * S * M));
    if (h->red0) {
      // moment 0 runs on the (I,Q) sub-problem: its surface matrix must not couple (I,Q) with (U,V) either
      std::vector<double> r0;
      if (!mom_m0_cut_brdf(Rsurf, N, nS, h->N0, r0)) return fail(h, MOM_EINVAL, kMomM0BrdfCouples);
      HIPCHK(h, mom_upload(h->d_Rsurf0, r0.data(), r0.size(), h->stream));
    }
  } else if (kind == 2) {
    HIPCHK(h, mom_upload(h->d_albedo_spec, albedo_spec, S, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->surf_kind = kind;
  return MOM_OK;
}

// The runs that are ONE launch (rt_run_small, rt_run_wave) between the handle's timing events: the launch is the whole "full
// layers" stage, the surface and post-processing stages are empty
static int single_launch_begin(mom_t *h) {
  while (h->ev_full.size() < 2) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev_full.push_back(e); }
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  HIPCHK(h, hipEventRecord(h->ev_full[0], h->stream));
  return MOM_OK;
}
static int single_launch_end(mom_t *h) {
  HIPCHK(h, hipEventRecord(h->ev_full[1], h->stream));
  for (int k = 1; k < 4; ++k) HIPCHK(h, hipEventRecord(h->ev[k], h->stream));
  h->launches = 1; h->launches_full = 1; h->launches_red = 0;
  return MOM_OK;
}

// N <= 4: one spectral point per lane, all moments / layers / surface / post-processing in ONE launch (arguments: mom_host.hpp)
static int rt_run_small(mom_t *h) {
  const int Nz = h->Nz;
  if (!h->d_smtab) HIPCHK(h, h->d_smtab.renew(3 * 16));
  double tab[48];
  mom_small_tables(h->h_mu.data(), h->N, tab);
  HIPCHK(h, hipMemcpyAsync(h->d_smtab, tab, sizeof tab, hipMemcpyHostToDevice, h->stream));
  {
    HIPCHK(h, h->d_ndif.reserve(2 * (size_t)Nz, h->stream));
    std::vector<int> v(h->nd);
    v.insert(v.end(), h->iface.begin(), h->iface.end());
    HIPCHK(h, hipMemcpyAsync(h->d_ndif, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host arrays above go out of scope
  }
  if (h->K > 4) return fail(h, MOM_EINVAL, "mom_rt_run: the N <= 4 sweep kernel handles at most 4 phase-matrix bases");
  MomSmallSweepArgs a{};
  HIPCHK(h, mom_fill_small_args(a, *h, h->q, h->S, h->d_info, h->opt_small != 2, h->stream));
  int rc = single_launch_begin(h);
  if (rc) return rc;
  HIPCHK(h, momsm_launch_sweep(&a, h->N, h->stream));
  return single_launch_end(h);
}

// 4 < N <= 32: one spectral point per wavefront, operators in MFMA-layout registers, ONE launch
static bool wave_sweep_applies(const mom_t *h) { return mom_wave_sweep_applies(*h, h->N, h->nS, h->opt_small, h->opt_force_generic); }
static int rt_run_wave(mom_t *h) {
  const int Nz = h->Nz;
  HIPCHK(h, h->d_ndif.reserve(2 * (size_t)Nz, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_ndif, h->nd.data(), (size_t)Nz * sizeof(int), hipMemcpyHostToDevice, h->stream));
  MomWaveSweepArgs a{};
  mom_fill_wave_args(a, *h, h->q, h->S, h->d_info, h->opt_small == 1);
  int rc = single_launch_begin(h);
  if (rc) return rc;
  HIPCHK(h, momw_launch_sweep(&a, h->stream));
  if ((rc = single_launch_end(h))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));  // h->nd may be rewritten by the next scene_set
  return MOM_OK;
}

// ---- one layer launch (rt_run_core's launch_layer) as a policy over the image table (mom_images.hpp) ----------------------
// the kernel that runs every layer no first-stage image has completed
enum Finisher { kFinStrip4, kFinStrip8, kFinGen4, kFinGen8 };  // strip-chained image / general k_layer, 4-wave / 8-wave build

static Finisher choose_finisher(const mom_t *h, const DevStreams &q, int ns_tab, bool lds) {
  // small operators: 4-wave workgroups, two per CU (momcore_w4.hip; the strip-chained images of that build where the edge has
  // one), when two LDS images fit
  const MomLayerImage *s4 = mom_find_image(MOM_IMG_STRIP4, q.N);
  if (lds && h->opt_w4 && np_for(q.N) <= 48 &&
      2 * (s4 ? s4->lds_bytes(ns_tab, q.nS, h->K) : mom4_lds_bytes(q.N, true)) + 2048 <= 160 * 1024)
    return s4 ? kFinStrip4 : kFinGen4;
  return (lds && mom_find_image(MOM_IMG_STRIP8, q.N)) ? kFinStrip8 : kFinGen8;
}

// At most one first-stage image in front of the finisher, or {nullptr}.  Behind each of them the finisher resumes what it left:
//   * general 4-wave image (operator edges 20 .. 32, multiples of 4): the quad-block image (mom_q4.hpp), MOM_OPT_LEAN >= 3;
//   * 4-wave strip image: MOM_OPT_LEAN = 3 the quad-block image, 2 the six-wave lean image, 1 (and wherever the chosen one does
//     not apply) the lean image (three workgroups per CU; mom_lean.hpp) -- the route exists only where the lean image applies;
//   * 8-wave strip image: the two-buffer 4-wave image (two workgroups per CU; mom_strip2.hpp), MOM_OPT_STRIP2 (C2: it leaves
//     nothing -- the finisher's launch reads the resume table and ends).
struct FirstStage {
  const MomLayerImage *image;
  MomImageFamily family;
};
static FirstStage choose_first_stage(const mom_t *h, Finisher fin, const DevStreams &q, int ns_tab) {
  auto applying = [&](MomImageFamily f) {
    const MomLayerImage *im = mom_find_image(f, q.N);
    return FirstStage{(im && im->lds_bytes(ns_tab, q.nS, h->K) > 0) ? im : nullptr, f};
  };
  if (fin == kFinGen4 && h->opt_lean >= 3) return applying(MOM_IMG_QUAD);
  if (fin == kFinStrip8 && h->opt_strip2) return applying(MOM_IMG_STRIP2);
  if (fin == kFinStrip4 && h->opt_lean) {
    const FirstStage lean = applying(MOM_IMG_LEAN);
    if (lean.image && h->opt_lean >= 2) {
      const FirstStage alt = applying(h->opt_lean >= 3 ? MOM_IMG_QUAD : MOM_IMG_LEAN6);
      if (alt.image) return alt;
    }
    return lean;
  }
  return FirstStage{nullptr, MOM_IMG_LEAN};
}

// The first-stage launch of `fs` for the sweep described by `a`, if it applies: a whole-slab sweep of a single-target run, no
// forced pivoted inverse, interface code 3 on every layer that interacts (the images handle no other).  On return a.resume (and
// a.sched) are set for the finisher as well.
// nbw: the blocks of four entries with a weighted one of a.q (mom_q4_nbw).  sources_only (MOM_OPT_SOURCES_ONLY): no caller can
// observe a moment of this launch -- the two-buffer strip image and the quad-block image leave the composite R-+ and T++ out of it.
static int launch_first_stage(mom_t *h, const FirstStage &fs, LayerArgs &a, int nbw, bool multi_target, bool sources_only, hipStream_t st) {
  const int nzr = a.Nz_sweep;  // 0: a per-layer launch
  bool ok = fs.image && nzr > 0 && !multi_target && a.q.inv_mode == 0;
  for (int k = 1; k < nzr && ok; ++k) ok = (a.iface_z[k] == 3);
  if (ok && !a.first) ok = (a.iface_z[0] == 3);
  if (!ok) return MOM_OK;
  const size_t units = (size_t)a.S * a.M;
  // resume[unit]: the two-buffer image has a table of its own -- under MOM_OPT_OVERLAP the m = 0 sub-problem's first stage and
  // the full problem's two-buffer launch can be in flight at once
  const bool two_buffer = (fs.family == MOM_IMG_STRIP2);
  MomDevBuf<int> &table = two_buffer ? h->d_resume2 : h->d_resume;
  HIPCHK(h, table.reserve(units, st));
  a.resume = table;
  int per_cu = fs.image->per_cu();
  // which instantiation the image launches (mom_image_variants.hpp); the lean images have one
  const bool quad = (fs.family == MOM_IMG_QUAD);
  MomLaunchForm form;
  // MOM_OPT_ZERO_SKIP: bit 0 the quad-block image, bit 1 the two-buffer strip image, bit 2 the row-block rule of the latter
  if (h->opt_zero_skip & (quad ? 1 : two_buffer ? 2 : 0)) form.nbw = nbw;
  form.row_blocks = two_buffer && (h->opt_zero_skip & 4);
  form.sources_only = sources_only && (two_buffer || quad);
  // MOM_OPT_ELEMENTAL: the same two images, where the stream set of the launch has its tables (launch_layer sets a.etab)
  form.elemental_tab = (two_buffer || quad) && mom_elemental_tab_applies(a.q, a.K, a.etab);
  if (two_buffer) {
    h->resume2_units = units; h->resume2_nz = nzr;  // (mom_strip2_resumed)
    if (h->opt_strip2_sched) {  // the queue counter (and, for the chain priority, the per-CU tickets) start at zero: a memset ON
                                // THE STREAM, so that an asynchronous step (or a captured one) resets them in order with its launches
      const size_t ints = kMomStrip2SchedInts;
      if (!h->d_sched2) HIPCHK(h, h->d_sched2.renew(ints));
      HIPCHK(h, hipMemsetAsync(h->d_sched2, 0, ((h->opt_strip2_sched & 2) ? ints : 1) * sizeof(int), st));
      a.sched = h->d_sched2;
      form.sched_mode = h->opt_strip2_sched;
    }
  }
#ifdef MOM_EXPERIMENTS
  if (fs.family == MOM_IMG_LEAN || fs.family == MOM_IMG_LEAN6) {
    static const int lean_per_cu = getenv("MOM_LEAN_PER_CU") ? atoi(getenv("MOM_LEAN_PER_CU")) : 0;
    if (lean_per_cu > 0) per_cu = lean_per_cu;
  }
#endif
  const int grid = (int)std::min<size_t>(units, (size_t)per_cu * h->num_cu);  // persistent workgroups
  HIPCHK(h, fs.image->launch(&a, form, grid, st));
  h->launches++;
  return MOM_OK;
}

// One k_layer launch (plus the first-stage launch in front of it, if any) of the argument block `a` on stream `st`
static int launch_layer_images(mom_t *h, LayerArgs &a, int nbw, bool multi_target, bool sources_only, hipStream_t st) {
  const DevStreams &q = a.q;
  const size_t units = (size_t)a.S * a.M;
  const bool lds = (q.N <= 64) && !h->opt_force_generic;
  const int ns_tab = q.regular ? q.nS : 1;  // Stokes components per stream of the elemental layer's stream-pair tables
  const Finisher fin = choose_finisher(h, q, ns_tab, lds);
  const int rc = launch_first_stage(h, choose_first_stage(h, fin, q, ns_tab), a, nbw, multi_target, sources_only, st);
  if (rc) return rc;
  if (fin == kFinStrip4 || fin == kFinStrip8) {  // strip-chained kernels (momcore_strip.hip), one image per N
    const MomLayerImage *im = mom_find_image(fin == kFinStrip4 ? MOM_IMG_STRIP4 : MOM_IMG_STRIP8, q.N);
    // 8-wave build: persistent workgroups, one per CU (only one 135 KB LDS image fits a CU): the prologue is paid once;
    // their start is staggered over about one unit time (~ (44 + 17 nd) us at N = 60)
    // (not behind the two-buffer image: its units are done, a staggered start would only delay the empty resume launch)
    if (fin == kFinStrip8 && units >= 8 * (size_t)h->num_cu && h->opt_stagger && a.resume == nullptr) {
      const double f = (double)q.N / 60.0, unit_us = f * f * f * (44.0 + 17.0 * a.nd);
      a.stagger = (int)(unit_us * 100.0 / 32.0);
    }
    const int grid = (int)std::min<size_t>(units, (size_t)im->per_cu() * h->num_cu);  // persistent: two per CU (4-wave), one (8-wave)
    HIPCHK(h, im->launch(&a, MomLaunchForm{}, grid, st));
  } else if (fin == kFinGen4) {
    HIPCHK(h, mom4_launch_layer(&a, a.iface, true, (int)((a.S >= 2048) ? a.S : units), mom4_lds_bytes(q.N, true), st));
  } else {
    const int grid = lds ? (int)((a.S >= 2048) ? a.S : units) : (int)std::min<size_t>(units, (size_t)h->G);
    HIPCHK(h, mom_gen_launch_layer(&a, a.iface, lds, grid, lds_bytes(q.N, lds), st));
  }
  h->launches++;
  return MOM_OK;
}

// The general path of mom_rt_run for the layers [za, zb) of the column into the composite state `compF` (full problem;
// the m = 0 sub-problem keeps its own arrays and is used only when allow_red): layer kernels, then (do_surface) the
// surface layer with its closing interaction, then (do_post) the azimuthal post-processing into d_R / d_T / d_hdr.
// mom_rt_run: the whole column; mom_rt_run_multisensor: the slabs above and below a sensor.
// multi-target sweep (mom_rt_run_multisensor): composite targets and the per-layer action table of LayerArgs
struct TargetSpec {
  int ntgt = 0;
  double *tgt[kMaxTargets][6] = {};
  std::vector<signed char> act;  // [zb - za][kMaxTargets]
};

template <class Comp6>  // compF[6]: the handle's buffers or raw pointers
static int rt_run_core(mom_t *h, int za, int zb, bool allow_red, const Comp6 &compF, bool do_surface, bool do_post,
                       bool cont = false, const TargetSpec *tg = nullptr) {
  const size_t S = h->S;
  const int M = h->scene_M;
  const bool red0 = h->red0 && allow_red;
  const int nzr = zb - za;
  while (h->ev_full.size() < 2 * (size_t)h->Nz + 2) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev_full.push_back(e); }
  while (h->ev_red.size() < 2 * (size_t)h->Nz + 2) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev_red.push_back(e); }
  const int Nk = h->Nk;  // kernel-side edge of the full problem (strip_pad)
  const size_t NN = (size_t)Nk * Nk;
  // one k_layer launch over `Mcount` moments starting at `m_first` with stream set `q` (full or reduced)
  // sweep mode: every layer of a unit inside one launch (z < 0 selects it); needs one interface code for all z >= 1
  // (the code is a template argument of the kernel images) -- always the case once scattering has set in
  // cont: the slab continues the composite state already in compF (its first layer interacts like the others)
  bool can_sweep = h->opt_sweep && nzr <= kMaxSweepLayers && nzr > 1;
  for (int z = za + 2; z < zb && can_sweep; ++z) can_sweep = (h->iface[z] == h->iface[za + 1]);
  if (cont && can_sweep) can_sweep = (h->iface[za] == h->iface[za + 1]);
  for (int z = za; z < zb && can_sweep; ++z) can_sweep = (h->nd[z] <= 127);
  hipStream_t cur = h->stream;  // the stream launch_layer issues to (MOM_OPT_OVERLAP switches it for the m = 0 sub-problem)
  // nbw: MomLaunchForm::nbw of the stream set q (launch_first_stage leaves it 0 where MOM_OPT_ZERO_SKIP has the image's bit off).  Full
  // problem: from the weights mom_set_streams
  // uploaded (the dummy entries behind the N real ones only lengthen the run of zero weights); sub-problem: scene_common's count
  const int nbw_k = mom_q4_nbw(h->h_wt.data(), h->N);
  auto launch_layer = [&](int z, const DevStreams &q, int nbw, int m_first, int Mcount, const double *Zpp, const double *Zmp,
                          const auto &comp, double *scratch) -> int {  // comp[6]: buffers or raw pointers
    LayerArgs a{};
    a.q = q; a.S = h->S; a.M = Mcount; a.K = h->K; a.m_first = m_first;
    const bool sweep = z < 0;
    if (sweep) {
      z = za;
      a.Nz_sweep = nzr;
      int ndsum = 0;
      for (int k = 0; k < nzr; ++k) { a.nd_z[k] = (signed char)h->nd[za + k]; a.iface_z[k] = (signed char)h->iface[za + k]; ndsum += h->nd[za + k]; }
      a.nd = ndsum / nzr; a.iface = h->iface[za + 1]; a.first = cont ? 0 : 1;
    } else {
      a.nd = h->nd[z]; a.iface = h->iface[z]; a.first = (z == za) && !cont;
    }
    a.tau = h->d_tau + S * z; a.varpi = h->d_varpi + S * z; a.zw = h->d_zw + (size_t)h->K * S * z;
    a.tau_sum = h->d_tau_sum + S * z;
    a.Zpp = Zpp; a.Zmp = Zmp;
    for (int k = 0; k < 6; ++k) a.comp[k] = comp[k];
    if (tg) {  // every moment of a target lies m_first moments into its arrays, like comp
      a.ntgt = tg->ntgt;
      for (int t = 0; t < tg->ntgt; ++t)
        for (int k = 0; k < 6; ++k) a.tgt[t][k] = tg->tgt[t][k];
      const int rows = sweep ? nzr : 1, r0 = sweep ? 0 : (z - za);
      for (int r = 0; r < rows; ++r)
        for (int t = 0; t < kMaxTargets; ++t) a.act_z[r][t] = tg->act[(size_t)(r0 + r) * kMaxTargets + t];
    }
    a.scratch = scratch; a.info = h->d_info;
    // MOM_OPT_ELEMENTAL: the stream-pair tables of the stream set this launch runs with
    if (h->opt_elemental) a.etab = (&q == &h->q0) ? h->d_etab0.get() : h->d_etab.get();
    // MOM_OPT_SOURCES_ONLY: mom_rt_run alone (allow_red and no targets: mom_rt_run_multisensor has neither), and only a launch
    // that holds no observable moment -- the (I,Q) sub-problem's (mom_download: MOM_ESTATE) or one that starts behind moment 0
    const bool unobserved = h->opt_sources_only && allow_red && !tg && (&q == &h->q0 || m_first >= 1);
    return launch_layer_images(h, a, nbw, tg != nullptr, unobserved, cur);
  };
  // MOM_OPT_OVERLAP: the two launches of a sweep -- moments 1..M-1 on the full problem, moment 0 on the (I,Q) sub-problem --
  // are independent.  What runs at the edges 52 / 56 / 60 (C2: N = 60, sub-problem N = 40): the sub-problem on the quad-block image
  // (one wavefront per unit, four per CU, 10 000 units), the full problem on the two-buffer strip image (two 4-wave workgroups per
  // CU, persistent, 20 000 units handed out by its shared queue, MOM_OPT_STRIP2_SCHED) and behind it the 8-wave image's resume
  // launch, which finds nothing left in C2.  The sub-problem (with its surface interaction) goes first, on the handle's second,
  // high-priority stream; the full problem's workgroups take the CUs as the sub-problem's tail frees them, and a quad-block
  // workgroup can share a CU with ONE two-buffer workgroup (75 + 2 x 40 KB of LDS), not with two.
  // Where two such kernels share CUs for long they contend for the matrix pipes and LDS bandwidth and the sweep takes longer
  // than the two launches in sequence (profiles/r06_C2_ab.txt (b'): N = 36 .. 44 with the m = 0 problem on the wave-per-point
  // kernel 28 -> 45 ms, C4 -5 %), so the overlap is reserved for the edges below, where only the tails meet; measured there it
  // gained about 2 ms of 330 (profiles/r07_C2_ab.txt).  With the shared unit queue the full problem has no partial last round left
  // to fill: re-measured at the default, 322.6 ms with the overlap and 322.7 without (profiles/r08_C2_ab.txt).  It costs nothing,
  // so the gate stays
  const bool two = red0 && can_sweep && h->opt_overlap && M > 1 && !tg && h->stream2 && !h->opt_force_generic &&
                   mom_find_image(MOM_IMG_STRIP2, Nk) != nullptr;  // ("the edges below": those of the two-buffer image)
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  for (int z = (can_sweep ? -1 : za); z < (can_sweep ? 0 : zb); ++z) {
    int rc;
    const int e = can_sweep ? 0 : z - za;  // event slot
    if (red0) {
      if (two) {  // the m = 0 sub-problem first, on the high-priority stream: see the comment at `two`
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        cur = h->stream2;
        // the full problem's launch is released only when the second stream has passed its own wait and stands right before
        // the sub-problem's launch: otherwise the main stream (no wait packet in front of its kernel) always dispatches first
        HIPCHK(h, hipEventRecord(h->ev_go, cur));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_go, 0));
        HIPCHK(h, hipEventRecord(h->ev_red[2 * e], cur));
        if ((rc = launch_layer(z, h->q0, h->nbw_0, 0, 1, h->d_Zpp0, h->d_Zmp0, h->comp0, h->d_scratch0))) return rc;
        HIPCHK(h, hipEventRecord(h->ev_red[2 * e + 1], cur));
        h->launches_red++;
        cur = h->stream;
      }
      if (M > 1) {  // moments 1..M-1 on the full problem
        double *comp1[6];
        for (int k = 0; k < 6; ++k) comp1[k] = compF[k] + ((k < 4) ? (size_t)comp_pitch(Nk) * Nk : (size_t)Nk) * S;
        HIPCHK(h, hipEventRecord(h->ev_full[2 * e], h->stream));
        if ((rc = launch_layer(z, h->qk, nbw_k, 1, M - 1, h->d_Zpp + NN * h->K, h->d_Zmp + NN * h->K, comp1, h->d_scratch))) return rc;
        HIPCHK(h, hipEventRecord(h->ev_full[2 * e + 1], h->stream));
        h->launches_full++;
      }
      if (!two) {
        HIPCHK(h, hipEventRecord(h->ev_red[2 * e], h->stream));
        if ((rc = launch_layer(z, h->q0, h->nbw_0, 0, 1, h->d_Zpp0, h->d_Zmp0, h->comp0, h->d_scratch0))) return rc;
        HIPCHK(h, hipEventRecord(h->ev_red[2 * e + 1], h->stream));
        h->launches_red++;
      }
    } else {
      HIPCHK(h, hipEventRecord(h->ev_full[2 * e], h->stream));
      if ((rc = launch_layer(z, h->qk, nbw_k, 0, M, h->d_Zpp, h->d_Zmp, compF, h->d_scratch))) return rc;
      HIPCHK(h, hipEventRecord(h->ev_full[2 * e + 1], h->stream));
      h->launches_full++;
    }
  }
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  // surface layer + closing interaction: m = 0 always; every moment for a BRDF surface (kind 1)
  for (int m = 0; do_surface && m < ((h->surf_kind == 1) ? M : 1); ++m) {
    SurfArgs a{};
    const bool red = red0 && m == 0;
    const DevStreams &q = red ? h->q0 : h->qk;
    a.q = q; a.S = h->S; a.iface = h->iface[h->Nz - 1];  // Q6: last layer's interface code (rt_run.jl:181)
    a.albedo = h->albedo; a.tau_tot = h->d_tau_sum + S * h->Nz;
    a.kind = h->surf_kind; a.m = m; a.albedo_spec = h->d_albedo_spec;
    a.Rsurf = (h->surf_kind == 1) ? (red ? h->d_Rsurf0 : h->d_Rsurf + NN * m) : nullptr;
    for (int k = 0; k < 6; ++k)
      a.comp[k] = red ? h->comp0[k] : compF[k] + ((k < 4) ? (size_t)comp_pitch(Nk) * Nk : (size_t)Nk) * S * m;
    a.hdrJ = red ? h->d_hdrJ0 : (m == 0 ? h->d_hdrJ : h->d_hdrJm + (size_t)Nk * S * m);
    a.bhr_uw = h->d_bhr_uw; a.bhr_dw = h->d_bhr_dw; a.nS_out = h->nS;
    a.scratch = red ? h->d_scratch0 : h->d_scratch; a.info = h->d_info;
    const bool lds = (q.N <= 64) && !h->opt_force_generic;
    const size_t sm = lds_bytes(q.N, lds);
    const int grid = lds ? (int)S : (int)std::min<size_t>(S, (size_t)h->G);
    const hipStream_t sst = (two && red) ? h->stream2 : h->stream;  // the sub-problem's surface follows its layers
    if (lds && h->opt_w4 && np_for(q.N) <= 48 && 2 * mom4_lds_bytes(q.N, true) + 2048 <= 160 * 1024) {
      HIPCHK(h, mom4_launch_surface(&a, true, (int)S, mom4_lds_bytes(q.N, true), sst));
    } else {
      HIPCHK(h, mom_launch_ldsm(MOM_LDSM(k_surface), lds, grid, kThreads, sm, sst, a));
    }
  }
  if (two) {  // join: everything below (post-processing, the caller's downloads) is ordered behind both streams
    HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  if (do_post) {
    const size_t total = (size_t)h->nVza * h->nS * S;
    PostArgs pa{};
    pa.N = Nk; pa.nS = h->nS; pa.S = h->S; pa.M = M; pa.nVza = h->nVza; pa.red0 = red0 ? 1 : 0;
    pa.N0 = h->N0; pa.nS0 = h->nS0;
    pa.node = h->d_node; pa.cos_mphi = h->d_cos; pa.sin_mphi = h->d_sin;
    pa.J0p = compF[4]; pa.J0m = compF[5]; pa.J0p0 = h->comp0[4]; pa.J0m0 = h->comp0[5];
    pa.hdrJ = red0 ? h->d_hdrJ0 : h->d_hdrJ;
    pa.hdr_all = (h->surf_kind == 1) ? 1 : 0; pa.zeroT_hi = (h->surf_kind == 2) ? 1 : 0; pa.hdrJm = h->d_hdrJm;
    pa.R = h->d_R; pa.T = h->d_T; pa.hdr = h->d_hdr;
    hipLaunchKernelGGL(k_postprocess, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, pa);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  return MOM_OK;
}

extern "C" int mom_rt_run(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_rt_run: call mom_scene_set first");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->f32) {
    const int rc = momf_rt_run(h->f32);
    return rc ? fail(h, rc, momf_error(h->f32)) : MOM_OK;
  }
  h->launches = 0; h->launches_full = 0; h->launches_red = 0;
  h->comp_pitched = true;
  h->comp_on_chip = true;
  if (h->N <= 4 && h->opt_small && !h->opt_force_generic && h->nVza <= 4 && h->surf_kind == 0 && h->K <= 4) return rt_run_small(h);
  if (wave_sweep_applies(h)) return rt_run_wave(h);
  h->comp_on_chip = false;
  return rt_run_core(h, 0, h->Nz, true, h->comp, true, true);
}

// rt_run_test_ms(::noRS, sensor_levels, model, iBand) (rt_run_multisensor.jl:14-191).  Sensors are processed one after
// the other (in order of depth) with two composite states: the slab above the sensor (layers 1..L) and the slab below it (layers L+1..Nz and
// the surface), each built by the same fused layer kernels as mom_rt_run (sweep mode, strip chains, padded edges), then
// k_interlayer and the azimuthal post-processing of the interface fields.  The m = 0 (I,Q) reduction is not used here
// (the interface fields couple two states of the full problem); level 0 is mom_rt_run itself.
extern "C" int mom_rt_run_multisensor(mom_t *h, int nSensors, const int *sensor_levels, double *uwJ, double *dwJ) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_rt_run_multisensor");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_rt_run_multisensor: call mom_scene_set first");
  if (nSensors <= 0 || !sensor_levels || !uwJ || !dwJ) return fail(h, MOM_EINVAL, "mom_rt_run_multisensor: bad argument");
  for (int i = 0; i < nSensors; ++i)
    if (sensor_levels[i] < 0 || sensor_levels[i] >= h->Nz)
      return fail(h, MOM_EINVAL, "mom_rt_run_multisensor: sensor level must be in 0..Nz-1 (0 = TOA/BOA, L = below layer L)");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = h->S;
  const int M = h->scene_M, Nk = h->Nk;
  const size_t out1 = (size_t)h->nVza * h->nS * S;
  h->launches = 0; h->launches_full = 0; h->launches_red = 0;
  h->comp_pitched = true;
  h->comp_on_chip = false;
  if (!h->comp_top[0]) {
    const int Na = h->N + kMomPadMax;
    for (int k = 0; k < 6; ++k) {
      const size_t perc = (k < 4) ? (size_t)comp_pitch(Na) * Na : (size_t)Na;
      HIPCHK(h, h->comp_top[k].renew(perc * S * h->M));
    }
    for (int k = 0; k < 2; ++k) HIPCHK(h, h->d_msJ[k].renew((size_t)Na * S * h->M));
  }
  HIPCHK(h, h->d_ms_out.reserve(2 * out1 * nSensors, h->stream));
  double *d_uw = h->d_ms_out, *d_dw = h->d_ms_out + out1 * nSensors;
  // rt_kernel_multisensor! (rt_kernel_multisensor.jl:51-112): ONE sweep over the layers builds every layer's added operators
  // once and feeds all composites -- the running slab above the sensors (target 0, frozen into a per-sensor snapshot when
  // the sweep passes the sensor's level) and the slab below each sensor -- then per sensor the surface interaction, the
  // interface solve and the post-processing.  Sensors are processed in chunks of what one kernel's target table holds.
  const int Na = h->N + kMomPadMax;
  const size_t blk[6] = {(size_t)comp_pitch(Na) * Na, (size_t)comp_pitch(Na) * Na, (size_t)comp_pitch(Na) * Na,
                         (size_t)comp_pitch(Na) * Na, (size_t)Na, (size_t)Na};
  const int per_chunk = (kMaxTargets - 1) / 2;  // top + (snapshot + bottom) per sensor
  for (int c0 = 0; c0 < nSensors; c0 += per_chunk) {
    const int nc = std::min(per_chunk, nSensors - c0);
    const size_t need = (size_t)2 * nc;  // composite sets beyond h->comp_top: nc snapshots + nc bottoms
    if (h->ms_comp.size() < 6 * need) h->ms_comp.resize(6 * need);
    for (size_t sidx = 0; sidx < need; ++sidx)
      for (int k = 0; k < 6; ++k) HIPCHK(h, h->ms_comp[6 * sidx + k].reserve(blk[k] * S * h->M, h->stream));
    // sensors of this chunk in order of depth: the slab below sensor i is the SEGMENT of layers [L_i, L_i+1) -- built in the
    // shared sweep, so every layer feeds the running top slab and exactly one segment whatever the number of sensors --
    // joined afterwards to the slab below sensor i + 1 (k_combine); the deepest sensor's segment runs to the last layer
    std::vector<int> ord(nc);
    for (int i = 0; i < nc; ++i) ord[i] = c0 + i;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sensor_levels[x] < sensor_levels[y]; });
    TargetSpec tg;
    tg.act.assign((size_t)h->Nz * kMaxTargets, 0);
    int maxL = 0;
    for (int i = 0; i < nc; ++i) maxL = std::max(maxL, sensor_levels[c0 + i]);
    int nt = 0;
    for (int k = 0; k < 6; ++k) tg.tgt[0][k] = h->comp_top[k];
    nt = 1;
    for (int z = 0; z < maxL; ++z) tg.act[(size_t)z * kMaxTargets + 0] = (z == 0) ? 1 : 2;
    std::vector<int> snap_t(nc, -1), bot_t(nc, -1);
    for (int i = 0; i < nc; ++i) {
      const int L = sensor_levels[ord[i]], Lnext = (i + 1 < nc) ? sensor_levels[ord[i + 1]] : h->Nz;
      if (L > 0) {
        snap_t[i] = nt;
        for (int k = 0; k < 6; ++k) tg.tgt[nt][k] = h->ms_comp[(size_t)(2 * i) * 6 + k];
        tg.act[(size_t)(L - 1) * kMaxTargets + nt] = 3;
        ++nt;
      }
      bot_t[i] = nt;
      for (int k = 0; k < 6; ++k) tg.tgt[nt][k] = h->ms_comp[(size_t)(2 * i + 1) * 6 + k];
      for (int z = L; z < Lnext; ++z) tg.act[(size_t)z * kMaxTargets + nt] = (z == L) ? 1 : 2;
      ++nt;
    }
    tg.ntgt = nt;
    int rc;
    if ((rc = rt_run_core(h, 0, h->Nz, false, h->comp, false, false, false, &tg))) return rc;
    for (int i = nc - 2; i >= 0; --i) {  // slab below sensor i = its segment (+) the slab below sensor i + 1
      const int L = sensor_levels[ord[i]], Lnext = sensor_levels[ord[i + 1]];
      if (L == Lnext) {  // same level: same slab
        for (int k = 0; k < 6; ++k)
          HIPCHK(h, hipMemcpyAsync(tg.tgt[bot_t[i]][k], tg.tgt[bot_t[i + 1]][k], blk[k] * S * h->M * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        continue;
      }
      InterArgs a{};
      a.q = h->qk; a.S = h->S; a.M = M;
      for (int k = 0; k < 6; ++k) { a.top[k] = tg.tgt[bot_t[i]][k]; a.bot[k] = tg.tgt[bot_t[i + 1]][k]; }
      a.scratch = h->d_scratch; a.info = h->d_info;
      const bool lds = (Nk <= 64) && !h->opt_force_generic;
      const size_t sm = lds_bytes(Nk, lds);
      const size_t units = S * M;
      const int grid = (int)(lds ? units : std::min<size_t>(units, (size_t)h->G));
      HIPCHK(h, mom_launch_combine(a, lds, grid, sm, h->stream));  // (momcore.hip)
    }
    for (int i = 0; i < nc; ++i) {
      const int ims = ord[i], L = sensor_levels[ims];
      double *bot[6], *top[6];
      for (int k = 0; k < 6; ++k) { bot[k] = tg.tgt[bot_t[i]][k]; top[k] = (L > 0) ? tg.tgt[snap_t[i]][k] : nullptr; }
      // surface interaction with the slab below the sensor (rt_run_multisensor.jl:150-159); L = 0: + post-processing of the
      // whole column (uwJ = R_SFI, dwJ = T_SFI, postprocessing_vza_ms.jl:34-36)
      if ((rc = rt_run_core(h, h->Nz, h->Nz, false, bot, true, L == 0))) return rc;
      if (L > 0) {
        InterArgs a{};
        a.q = h->qk; a.S = h->S; a.M = M;
        for (int k = 0; k < 6; ++k) { a.top[k] = top[k]; a.bot[k] = bot[k]; }
        a.dwJ = h->d_msJ[0]; a.uwJ = h->d_msJ[1]; a.scratch = h->d_scratch; a.info = h->d_info;
        const bool lds = (Nk <= 64) && !h->opt_force_generic;
        const size_t sm = lds_bytes(Nk, lds);
        const size_t units = S * M;
        const int grid = (int)(lds ? units : std::min<size_t>(units, (size_t)h->G));
        HIPCHK(h, mom_launch_ldsm(MOM_LDSM(k_interlayer), lds, grid, kThreads, sm, h->stream, a));
        PostArgs pa{};
        pa.N = Nk; pa.nS = h->nS; pa.S = h->S; pa.M = M; pa.nVza = h->nVza; pa.red0 = 0;
        pa.node = h->d_node; pa.cos_mphi = h->d_cos; pa.sin_mphi = h->d_sin;
        pa.J0p = h->d_msJ[0]; pa.J0m = h->d_msJ[1];
        pa.hdrJ = h->d_hdrJ; pa.hdr_all = 0; pa.zeroT_hi = 0; pa.hdrJm = nullptr;
        pa.R = h->d_R; pa.T = h->d_T; pa.hdr = h->d_hdr;
        hipLaunchKernelGGL(k_postprocess, dim3((unsigned)((out1 + 255) / 256)), dim3(256), 0, h->stream, pa);
        HIPCHK(h, hipGetLastError());
      }
      HIPCHK(h, hipMemcpyAsync(d_uw + out1 * ims, h->d_R, out1 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(d_dw + out1 * ims, h->d_T, out1 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
  }
  HIPCHK(h, hipMemcpyAsync(uwJ, d_uw, out1 * nSensors * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dwJ, d_dw, out1 * nSensors * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return check_info(h);
}

// ---- ForwardDiff.Dual through rt_run (mom_dual.hip) ---------------------------------------------------------------
// What mom_scene_set_partials and mom_scene_set_optics_partials (mom_optics.hip) share: mom_host.hpp
int mom_partials_check(mom_t *h, const char *fn, int P, const double *dZpp, const double *dZmp) {
  char buf[200];
  if (!(P >= 0 && P <= 64 && ((dZpp == nullptr) == (dZmp == nullptr)))) {
    snprintf(buf, sizeof buf, "%s: 0 <= P <= 64; dZpp and dZmp come together", fn);
    return fail(h, MOM_EINVAL, buf);
  }
  // dZpp == dZmp == NULL with a staged partial set (mom_scene_stage_greek_partials): mom_partials_rest forms it, for this P
  const MomGreekStage &st = h->stage_d;
  if (dZpp || !st.live) return MOM_OK;
  if (st.P != P) {
    snprintf(buf, sizeof buf, "%s: P = %d, but the staged Greek partials (mom_scene_stage_greek_partials) are P = %d", fn, P, st.P);
    return fail(h, MOM_EINVAL, buf);
  }
  for (int b : st.basis)
    if (b >= h->K) {
      snprintf(buf, sizeof buf, "%s: the staged Greek partials name basis %d, the scene has K = %d", fn, b, h->K);
      return fail(h, MOM_EINVAL, buf);
    }
  return MOM_OK;
}
// mom_partials_rest's staged case: d_dual_in[3] / [4] [Nk, Nk, K, M, P], zero but for the blocks of the staged (basis, partial) pairs
static int stage_partials(mom_t *h) {
  MomGreekStage st = std::move(h->stage_d);
  h->stage_d.drop();
  const int K = h->K, M = h->scene_M, Nk = h->Nk, nD = st.nG;
  const size_t nZ = (size_t)Nk * Nk * K * M * h->dual_P;
  const std::vector<double> mu = stream_mu(h);
  std::vector<int> slot((size_t)nD * M);
  for (int mi = 0; mi < M; ++mi)
    for (int d = 0; d < nD; ++d) slot[d + (size_t)nD * mi] = st.basis[d] + K * (mi + M * st.partial[d]);
  MomZmomPlan pl;
  HIPCHK(h, mom_zmom_plan(pl, h->nS, (int)mu.size(), mu.data(), nD, st.l_pad, st.l_max.data(), st.greek.data(), 0, M, slot.data(), h->stream));
  HIPCHK(h, h->d_dual_in[3].renew(nZ));
  HIPCHK(h, h->d_dual_in[4].renew(nZ));
  HIPCHK(h, hipMemsetAsync(h->d_dual_in[3], 0, nZ * sizeof(double), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_dual_in[4], 0, nZ * sizeof(double), h->stream));
  HIPCHK(h, mom_zmom_launch(pl, h->stream, h->d_dual_in[3], h->d_dual_in[4], Nk, nullptr, nullptr, 0));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the plan and the stage go out of scope
  return MOM_OK;
}
void mom_partials_reset(mom_t *h, int P) {
  for (auto &b : h->d_dual_in) b.reset();
  h->d_dual_out.reset(); h->d_dual_ts.reset();
  h->dual_P = P;
  h->dual_ran = false;
}
int mom_partials_rest(mom_t *h, const double *dZpp, const double *dZmp, const double *dalbedo, const double *dRsurf,
                      const double *dalbedo_spec) {
  const size_t S = h->S, Nz = h->Nz, K = h->K, M = h->scene_M, N = h->N, Nk = h->Nk, P = h->dual_P;
  if (dZpp) {
    if (Nk == N) {
      HIPCHK(h, mom_upload(h->d_dual_in[3], dZpp, N * N * K * M * P, h->stream));
      HIPCHK(h, mom_upload(h->d_dual_in[4], dZmp, N * N * K * M * P, h->stream));
    } else {  // the scene's operators carry strip_pad's dummy entries (Z = 0): so do the partials
      const std::vector<double> zp = mom_pad_blocks(dZpp, (int)N, (int)Nk, K * M * P), zm = mom_pad_blocks(dZmp, (int)N, (int)Nk, K * M * P);
      HIPCHK(h, mom_upload(h->d_dual_in[3], zp.data(), zp.size(), h->stream));
      HIPCHK(h, mom_upload(h->d_dual_in[4], zm.data(), zm.size(), h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  } else if (h->stage_d.live) {  // (mom_partials_check has compared P and the bases with the scene)
    const int rc = stage_partials(h);
    if (rc) return rc;
  }
  if (dalbedo) HIPCHK(h, mom_upload(h->d_dual_in[5], dalbedo, (size_t)P, h->stream));
  if (dRsurf && h->surf_kind == 1) {
    const std::vector<double> rp = mom_pad_blocks(dRsurf, (int)N, (int)Nk, M * P);
    HIPCHK(h, mom_upload(h->d_dual_in[6], rp.data(), rp.size(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (dalbedo_spec && h->surf_kind == 2) HIPCHK(h, mom_upload(h->d_dual_in[7], dalbedo_spec, S * P, h->stream));
  HIPCHK(h, h->d_dual_out.renew((3 * (size_t)h->nVza + 2) * h->nS * S * P));   // dR | dT | dhdr | dbhr_uw | dbhr_dw
  HIPCHK(h, h->d_dual_ts.renew(S * (Nz + 1) * P));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// The partials of everything mom_scene_set / mom_scene_set_surface uploaded, in the layout of the value arrays with the
// partial index as the slowest axis; NULL = that input does not depend on the parameters.
extern "C" int mom_scene_set_partials(mom_t *h, int P, const double *dtau, const double *dvarpi, const double *dzw,
                                      const double *dZpp, const double *dZmp, const double *dalbedo, const double *dRsurf,
                                      const double *dalbedo_spec) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_scene_set_partials");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_scene_set_partials: call mom_scene_set first");
  const int rc = mom_partials_check(h, "mom_scene_set_partials", P, dZpp, dZmp);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  mom_partials_reset(h, P);
  if (P == 0) return MOM_OK;
  const size_t S = h->S, Nz = h->Nz, K = h->K;
  if (dtau) HIPCHK(h, mom_upload(h->d_dual_in[0], dtau, S * Nz * P, h->stream));
  if (dvarpi) HIPCHK(h, mom_upload(h->d_dual_in[1], dvarpi, S * Nz * P, h->stream));
  if (dzw) HIPCHK(h, mom_upload(h->d_dual_in[2], dzw, K * S * Nz * P, h->stream));
  return mom_partials_rest(h, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec);
}

// rt_run on Dual numbers for the resident scene: R_SFI / T_SFI (read with mom_get_RT) and their partials
// (mom_get_RT_partials).  Asynchronous on the handle's stream like mom_rt_run.
extern "C" int mom_rt_run_dual(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_rt_run_dual");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_rt_run_dual: call mom_scene_set first");
  HIPCHK(h, hipSetDevice(h->device));
  MomDualScene sc{};
  sc.N = h->Nk; sc.nS = h->nS; sc.S = h->S; sc.Nz = h->Nz; sc.K = h->K; sc.M = h->scene_M; sc.P = h->dual_P; sc.nVza = h->nVza;
  sc.imu0 = h->q.imu0; sc.strict = h->strict; sc.surf_kind = h->surf_kind; sc.mu0 = h->q.mu0; sc.albedo = h->albedo;
  for (int k = 0; k < 4; ++k) { sc.I0[k] = h->q.I0[k]; sc.D[k] = h->q.D[k]; }
  sc.mu = h->d_mu; sc.wt = h->d_wt;
  sc.tau = h->d_tau; sc.varpi = h->d_varpi; sc.zw = h->d_zw; sc.Zpp = h->d_Zpp; sc.Zmp = h->d_Zmp; sc.tau_sum = h->d_tau_sum;
  sc.dtau = h->d_dual_in[0]; sc.dvarpi = h->d_dual_in[1]; sc.dzw = h->d_dual_in[2]; sc.dZpp = h->d_dual_in[3];
  sc.dZmp = h->d_dual_in[4]; sc.dalbedo = h->d_dual_in[5]; sc.dRsurf = h->d_dual_in[6]; sc.dalbedo_spec = h->d_dual_in[7];
  sc.Rsurf = h->d_Rsurf; sc.albedo_spec = h->d_albedo_spec;
  sc.nd = h->nd.data(); sc.iface = h->iface.data(); sc.node = h->d_node; sc.cos_mphi = h->d_cos; sc.sin_mphi = h->d_sin;
  const size_t out = (size_t)h->nVza * h->nS * h->S;
  sc.R = h->d_R; sc.T = h->d_T; sc.dR = h->d_dual_out; sc.dT = h->d_dual_out ? h->d_dual_out + out * h->dual_P : nullptr;
  sc.hdr = h->d_hdr; sc.bhr_uw = h->d_bhr_uw; sc.bhr_dw = h->d_bhr_dw;
  sc.dhdr = h->d_dual_out ? h->d_dual_out + 2 * out * h->dual_P : nullptr;
  sc.dbhr_uw = h->d_dual_out ? h->d_dual_out + 3 * out * h->dual_P : nullptr;
  sc.dbhr_dw = sc.dbhr_uw ? sc.dbhr_uw + (size_t)h->nS * h->S * h->dual_P : nullptr;
  sc.dtau_sum_buf = h->d_dual_ts; sc.info = h->d_info; sc.stream = h->stream;
  sc.work = &h->dual_work;
  size_t budget = h->opt_dual_budget;
  if (!budget) {
    size_t fr = 0, tot = 0;
    HIPCHK(h, hipMemGetInfo(&fr, &tot));
    budget = (size_t)(0.6 * (double)(fr + h->dual_work.capacity()));
  }
  sc.work_budget = budget;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  std::string err;
  const int rc = momd_run(sc, &err);
  if (rc == 1) return fail(h, MOM_EUNSUPPORTED, err.c_str());
  if (rc) return fail(h, MOM_EHIP, err.c_str());
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  h->dual_ran = true;
  h->comp_on_chip = true;  // no composite layer of this run is left in the handle's operator-level state
  return MOM_OK;
}

extern "C" int mom_get_RT_partials(mom_t *h, double *dR_SFI, double *dT_SFI) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->dual_ran || h->dual_P == 0 || !dR_SFI || !dT_SFI)
    return fail(h, MOM_ESTATE, "mom_get_RT_partials: no Dual run with P > 0 / null output");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)h->nVza * h->nS * h->S * h->dual_P * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(dR_SFI, h->d_dual_out, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dT_SFI, h->d_dual_out + bytes / sizeof(double), bytes, hipMemcpyDeviceToHost, h->stream));
  return check_info(h);
}

extern "C" int mom_get_hdr_partials(mom_t *h, double *dhdr, double *dbhr_uw, double *dbhr_dw) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->dual_ran || h->dual_P == 0 || !dhdr || !dbhr_uw || !dbhr_dw)
    return fail(h, MOM_ESTATE, "mom_get_hdr_partials: no Dual run with P > 0 / null output");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t out = (size_t)h->nVza * h->nS * h->S * h->dual_P, fl = (size_t)h->nS * h->S * h->dual_P;
  HIPCHK(h, hipMemcpyAsync(dhdr, h->d_dual_out + 2 * out, out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dbhr_uw, h->d_dual_out + 3 * out, fl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dbhr_dw, h->d_dual_out + 3 * out + fl, fl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return check_info(h);
}

extern "C" int mom_get_RT(mom_t *h, double *R_SFI, double *T_SFI) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set || !R_SFI || !T_SFI) return fail(h, MOM_ESTATE, "mom_get_RT: no scene / null output");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->f32) {
    const int rc = momf_get_RT(h->f32, R_SFI, T_SFI);
    return rc ? fail(h, rc, momf_error(h->f32)) : check_info(h);
  }
  HIPCHK(h, mom_download_RT(*h, h->nS, h->S, R_SFI, T_SFI, h->stream));
  return check_info(h);
}

extern "C" int mom_get_hdr(mom_t *h, double *hdr, double *bhr_uw, double *bhr_dw) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set || !hdr || !bhr_uw || !bhr_dw) return fail(h, MOM_ESTATE, "mom_get_hdr: no scene / null output");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->f32) {
    const int rc = momf_get_hdr(h->f32, hdr, bhr_uw, bhr_dw);
    return rc ? fail(h, rc, momf_error(h->f32)) : check_info(h);
  }
  HIPCHK(h, mom_download_hdr(*h, h->nS, h->S, hdr, bhr_uw, bhr_dw, h->stream));
  return check_info(h);
}

extern "C" int mom_get_RT_device(mom_t *h, void *dR, void *dT) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_get_RT_device");
  if (!h->scene_set || !dR || !dT) return fail(h, MOM_ESTATE, "mom_get_RT_device: no scene / null output");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)h->nVza * h->nS * h->S * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(dR, h->d_R, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dT, h->d_T, bytes, hipMemcpyDeviceToDevice, h->stream));
  return MOM_OK;  // asynchronous: a singular-operator report surfaces at mom_get_RT / mom_check
}

// The resident phase-matrix arrays as the kernels read them (include/momcore.h), whichever route put them there
extern "C" int mom_scene_get_bases(mom_t *h, int which, int *edge, int *blocks, double *Zpp, double *Zmp) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_scene_get_bases");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_scene_get_bases: no scene");
  if (which < 0 || which > 3 || (Zpp == nullptr) != (Zmp == nullptr))
    return fail(h, MOM_EINVAL, "mom_scene_get_bases: which within 0..3; Zpp and Zmp come together");
  if (which == 3 && !h->rrs_scene) return fail(h, MOM_ESTATE, "mom_scene_get_bases: no Raman set (mom_scene_set_rrs)");
  int e = 0, b = 0;
  const double *src[2] = {nullptr, nullptr};
  if (which == 0) { e = h->Nk; b = h->K * h->scene_M; src[0] = h->d_Zpp; src[1] = h->d_Zmp; }
  else if (which == 1 && h->red0) { e = h->N0; b = h->K; src[0] = h->d_Zpp0; src[1] = h->d_Zmp0; }
  else if (which == 2 && h->d_dual_in[3]) { e = h->Nk; b = h->K * h->scene_M * h->dual_P; src[0] = h->d_dual_in[3]; src[1] = h->d_dual_in[4]; }
  else if (which == 3) { e = h->N; b = h->scene_M; src[0] = h->d_Zr[0]; src[1] = h->d_Zr[1]; }
  if (edge) *edge = e;
  if (blocks) *blocks = b;
  if (!Zpp || e == 0 || b == 0) return MOM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)e * e * b * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(Zpp, src[0], bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(Zmp, src[1], bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}
