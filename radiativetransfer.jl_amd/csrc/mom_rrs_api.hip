// mom_rrs_api.hip -- the rotational-Raman part of the C ABI (include/momcore.h): mom_elemental_inelastic_rrs with its kernel,
// and rt_run(::RRS) on the persistent layers of mom_rrs.hip (interface: mom_rrs.hpp).
#include "mom_handle.hpp"
#include "mom_rrs.hpp"

using namespace mom;

// elemental_inelastic!(RS_type::RRS, ...) (CoreKernel/elemental_inelastic.jl:23-91): the single-scattering layer of the
// rotational-Raman source operators, one thread per element (i, j, n1, dn) of the 4-D arrays -- get_elem_rt_RRS! (:93-160),
// get_elem_rt_SFI_RRS! (:320-382), apply_D_elemental_RRS! (:384-402; the SFI D kernel :404-412 / :478-490 changes nothing
// for any ndoubl).  n0 = n1 + i_l1l0[dn] is the incident-wavelength index (0-based here), dtau the elemental optical
// thickness per spectral point.  Entries whose n0 falls off the grid are written as zeros (the reference leaves the
// freshly allocated zeros in place).  HBM-write bound: 4 N^2 + 2 N doubles per (n1, dn).
struct RrsArgs {
  DevStreams q;
  int S, nR, m, nd, strict;
  const int *i_l1l0;                                                     // [nR]
  const double *varpi_l1l0, *fscatt, *tau_sum, *dtau, *varpi, *Zpp, *Zmp;  // [nR], [S] x4, [N,N] x2
  double *ier_mp, *iet_pp, *ier_pm, *iet_mm, *ieJ0p, *ieJ0m;              // [N,N,S,nR] x4, [N,S,nR] x2
};

__global__ void __launch_bounds__(256) k_elemental_rrs(RrsArgs a) {
#pragma clang fp contract(off)
  const int N = a.q.N, n = a.q.nS;
  const size_t NN = (size_t)N * N, total = NN * a.S * a.nR;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % N), j = (int)((e / N) % N);
  const size_t u = e / NN;                       // n1 + S dn
  const int n1 = (int)(u % a.S), dn = (int)(u / a.S);
  const int n0 = n1 + a.i_l1l0[dn];
  const double wdiv = (a.m == 0) ? 2.0 : 4.0, wct02 = (a.m == 0) ? 0.5 : 0.25;
  const double mui = a.q.mu[i], muj = a.q.mu[j], wj = a.q.wt[j] / wdiv;
  double r = 0.0, t = 0.0;
  const bool in = (n0 >= 0) && (n0 < a.S);
  if (in && wj > 1.e-8) {
    const double d1 = a.dtau[n1], d0 = a.dtau[n0];
    const double pre = a.varpi_l1l0[dn] * a.varpi[n0] * a.fscatt[n0];
    // :118-120
    r = a.fscatt[n0] * a.varpi_l1l0[dn] * a.varpi[n0] * a.Zmp[i + (size_t)N * j] * (1 / ((mui / muj) + (d1 / d0))) *
        (1 - exp(-((d1 / mui) + (d0 / muj)))) * wj;
    if (mui == muj) {
      if (i == j) {
        const double wi = a.q.wt[i] / wdiv;
        if (fabs(d0 - d1) > 1.e-6)   // :130-134
          t = pre * a.Zpp[i + (size_t)N * i] * wi * (exp(-d0 / mui) - exp(-d1 / mui)) / (1 - (d1 / d0));
        else                          // :136-138
          t = pre * a.Zpp[i + (size_t)N * i] * wi * (1 - exp(-d0 / muj));
      }
    } else {                          // :147-151
      t = pre * a.Zpp[i + (size_t)N * j] * (1 / ((mui / muj) - (d1 / d0))) * wj * (exp(-d1 / mui) - exp(-d0 / muj));
    }
  }
  // apply_D_elemental_RRS! (:384-402), component rule of SURVEY Q1
  const int ci = a.strict ? ((i + 1) % n) : (i % n) + 1, cj = a.strict ? ((j + 1) % n) : (j % n) + 1;
  if (a.nd < 1) {
    const double s = (((ci <= 2) && (cj <= 2)) || ((ci > 2) && (cj > 2))) ? 1.0 : -1.0;
    a.ier_pm[e] = s * r;
    a.iet_mm[e] = s * t;
  } else {
    if (ci > 2) r = -r;
    a.ier_pm[e] = 0.0;  // left untouched by the reference for ndoubl >= 1 (apply_D_matrix_IE! fills them after doubling)
    a.iet_mm[e] = 0.0;
  }
  a.ier_mp[e] = r;
  a.iet_pp[e] = t;
  if (j == 0) {  // source vectors: one thread per (i, n1, dn)                                   (:320-382)
    const int i_start = n * (a.q.imu0 - 1), i_end = n * a.q.imu0;  // 0-based [i_start, i_end)
    double jp = 0.0, jm = 0.0;
    if (in) {
      const double d1 = a.dtau[n1], d0 = a.dtau[n0], mus = a.q.mu[i_start];
      double zpI = 0.0, zmI = 0.0;
      for (int ii = i_start; ii < i_end; ++ii) {
        zpI += a.Zpp[i + (size_t)N * ii] * a.q.I0[ii - i_start];
        zmI += a.Zmp[i + (size_t)N * ii] * a.q.I0[ii - i_start];
      }
      const double pre = a.varpi_l1l0[dn] * a.varpi[n0] * a.fscatt[n0];
      if (i >= i_start && i < i_end) {
        if (fabs(d0 - d1) > 1.e-6) jp = (exp(-d0 / mui) - exp(-d1 / mui)) / ((d1 / d0) - 1) * pre * zpI * wct02;  // :350-353
        else jp = wct02 * pre * zpI * (1 - exp(-d0 / mus));                                                        // :355-357
      } else {                                                                                                     // :361-364
        jp = wct02 * pre * zpI * (1 / ((mui / mus) - (d1 / d0))) * (exp(-d1 / mui) - exp(-d0 / mus));
      }
      jm = wct02 * pre * zmI * (1 / ((mui / mus) + (d1 / d0))) * (1 - exp(-((d1 / mui) + (d0 / mus))));            // :368-370
      const double att = exp(-a.tau_sum[n0] / mus);                                                               // :371-372
      jp *= att;
      jm *= att;
    }
    if (a.nd >= 1) jm = a.q.D[i % n] * jm;  // :374-376
    const size_t o = i + (size_t)N * u;
    a.ieJ0p[o] = jp;
    a.ieJ0m[o] = jm;
  }
}

extern "C" int mom_elemental_inelastic_rrs(mom_t *h, int m, int ndoubl, int nRaman, const int *i_l1l0, const double *varpi_l1l0,
                                           const double *fscattRayl, const double *tau_sum, const double *dtau,
                                           const double *varpi, const double *Zpp_l1l0, const double *Zmp_l1l0,
                                           double *ier_mp, double *iet_pp, double *ier_pm, double *iet_mm, double *ieJ0p,
                                           double *ieJ0m) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_elemental_inelastic_rrs");
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_elemental_inelastic_rrs: call mom_set_streams first");
  if (m < 0 || ndoubl < 0 || nRaman <= 0 || !i_l1l0 || !varpi_l1l0 || !fscattRayl || !tau_sum || !dtau || !varpi ||
      !Zpp_l1l0 || !Zmp_l1l0 || !ier_mp || !iet_pp || !ier_pm || !iet_mm || !ieJ0p || !ieJ0m)
    return fail(h, MOM_EINVAL, "mom_elemental_inelastic_rrs: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  const int N = h->N;
  const size_t S = h->S, NN = (size_t)N * N, big = NN * S * nRaman, vec = (size_t)N * S * nRaman;
  double *buf = nullptr;
  int *dI = nullptr;
  HIPCHK(h, h->ws[0].reserve((4 * big + 2 * vec + nRaman + 4 * S + 2 * NN) * sizeof(double), h->stream));
  buf = reinterpret_cast<double *>(h->ws[0].get());
  HIPCHK(h, h->ws[1].reserve((size_t)nRaman * sizeof(int), h->stream));
  dI = reinterpret_cast<int *>(h->ws[1].get());
  double *d_out = buf, *d_vp = buf + 4 * big + 2 * vec, *d_fs = d_vp + nRaman, *d_ts = d_fs + S, *d_dt = d_ts + S,
         *d_w = d_dt + S, *d_zp = d_w + S, *d_zm = d_zp + NN;
  HIPCHK(h, hipMemcpyAsync(dI, i_l1l0, nRaman * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_vp, varpi_l1l0, nRaman * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_fs, fscattRayl, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_ts, tau_sum, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_dt, dtau, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_w, varpi, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_zp, Zpp_l1l0, NN * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_zm, Zmp_l1l0, NN * sizeof(double), hipMemcpyHostToDevice, h->stream));
  RrsArgs a{};
  a.q = h->q; a.S = h->S; a.nR = nRaman; a.m = m; a.nd = ndoubl; a.strict = h->strict;
  a.i_l1l0 = dI; a.varpi_l1l0 = d_vp; a.fscatt = d_fs; a.tau_sum = d_ts; a.dtau = d_dt; a.varpi = d_w; a.Zpp = d_zp; a.Zmp = d_zm;
  a.ier_mp = d_out; a.iet_pp = d_out + big; a.ier_pm = d_out + 2 * big; a.iet_mm = d_out + 3 * big;
  a.ieJ0p = d_out + 4 * big; a.ieJ0m = d_out + 4 * big + vec;
  hipLaunchKernelGGL(k_elemental_rrs, dim3((unsigned)((big + 255) / 256)), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  double *dst[6] = {ier_mp, iet_pp, ier_pm, iet_mm, ieJ0p, ieJ0m};
  for (int k = 0; k < 4; ++k) HIPCHK(h, hipMemcpyAsync(dst[k], d_out + k * big, big * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dst[4], a.ieJ0p, vec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(dst[5], a.ieJ0m, vec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// =========================================================================================
// rotational-Raman path (BASELINE config 5): rt_run(::RRS) -- kernels in mom_rrs.hip
// =========================================================================================
#define RRSCHK(h, call)                                                                                        \
  do {                                                                                                         \
    hipError_t e__ = (call);                                                                                   \
    if (e__ != hipSuccess) {                                                                                   \
      if ((h)->rrs && !(h)->rrs->err.empty()) {                                                                \
        const std::string m__ = (h)->rrs->err;                                                                 \
        (h)->rrs->err.clear();                                                                                 \
        return fail(h, MOM_EUNSUPPORTED, m__.c_str());                                                         \
      }                                                                                                        \
      char buf__[512];                                                                                         \
      snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      return fail(h, MOM_EHIP, buf__);                                                                         \
    }                                                                                                          \
  } while (0)

static momr::Streams rrs_streams(const mom_t *h) {
  momr::Streams q{};
  q.mu = h->d_mu; q.wt = h->d_wt;
  for (int k = 0; k < 4; ++k) { q.I0[k] = h->q.I0[k]; q.D[k] = h->q.D[k]; }
  q.N = h->N; q.nS = h->nS; q.imu0 = h->q.imu0; q.strict_idx = h->strict; q.mu0 = h->q.mu0;
  return q;
}
static int rrs_ready(mom_t *h, const char *who) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (h->dtype != 0) return fail(h, MOM_EINVAL, "the RRS path is Float64 only");
  if (!h->rrs) { static thread_local char b[128]; snprintf(b, sizeof b, "%s: call mom_rrs_set first", who); return fail(h, MOM_ESTATE, b); }
  if (!h->streams_set) return fail(h, MOM_ESTATE, "mom_set_streams must be called first");
  HIPCHK(h, hipSetDevice(h->device));
  h->rrs->fast = false;  // only mom_rt_run_rrs switches the deferred / derived mode on, for its own duration
  return MOM_OK;
}

extern "C" int mom_rrs_set(mom_t *h, int nRaman, const int *i_l1l0, const double *varpi_l1l0, int rrs_strict_reference) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_rrs_set");
  if (nRaman <= 0 || !i_l1l0 || !varpi_l1l0) return fail(h, MOM_EINVAL, "mom_rrs_set: bad argument");
  if (h->N > 64) return fail(h, MOM_EUNSUPPORTED, "mom_rrs_set: the RRS kernels cover operator edges N <= 64 (the reference's RRS shape is N = 15)");
  for (int k = 0; k < nRaman; ++k)
    if (std::abs(i_l1l0[k]) >= h->S) return fail(h, MOM_EINVAL, "mom_rrs_set: |i_l1l0| must be < nSpec (get_n0_n1 fails in the reference)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  momr::destroy(h->rrs);
  h->rrs = nullptr;
  h->rrs_scene = false;
  const hipError_t e = momr::create(&h->rrs, h->stream, h->N, h->nS, h->S, nRaman, i_l1l0, varpi_l1l0, rrs_strict_reference ? 1 : 0);
  if (e != hipSuccess) {
    momr::destroy(h->rrs);
    h->rrs = nullptr;
    char buf[256];
    snprintf(buf, sizeof buf, "mom_rrs_set: allocating the RRS layers failed: %s", hipGetErrorString(e));
    return fail(h, MOM_EHIP, buf);
  }
  if (h->opt_rrs_kernels >= 0) h->rrs->kopt = h->opt_rrs_kernels;
  return MOM_OK;
}

extern "C" int mom_rrs_set_shard(mom_t *h, int nSpec_global, int n_glob0, int n1_lo, int n1_hi) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->rrs) return fail(h, MOM_ESTATE, "mom_rrs_set_shard: call mom_rrs_set first");
  if (n_glob0 < 0 || n_glob0 + h->S > nSpec_global || n1_lo < 0 || n1_lo > n1_hi || n1_hi > h->S)
    return fail(h, MOM_EINVAL, "mom_rrs_set_shard: need 0 <= n_glob0, n_glob0 + nSpec <= nSpec_global, 0 <= n1_lo <= n1_hi <= nSpec");
  if (n1_hi > n1_lo) {
    // every source index n1 + i_l1l0 of an owned point must be local or off the GLOBAL grid
    const int H = h->rrs->max_off;
    if ((n_glob0 > 0 && n1_lo < H) || (n_glob0 + h->S < nSpec_global && h->S - n1_hi < H))
      return fail(h, MOM_EINVAL, "mom_rrs_set_shard: the halo is shorter than max |i_l1l0| on an interior edge");
  }
  h->rrs->n_glob0 = n_glob0;
  h->rrs->n1_lo = n1_lo;
  h->rrs->n1_hi = n1_hi;
  return MOM_OK;
}

static int rrs_check(mom_t *h) {
  int info = 0;
  HIPCHK(h, hipMemcpyAsync(&info, h->rrs->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (info) {
    HIPCHK(h, hipMemsetAsync(h->rrs->d_info, 0, sizeof(int), h->stream));
    char buf[128];
    snprintf(buf, sizeof buf, "zero pivot at elimination step %d while inverting (I - R r) (RRS path)", info);
    return fail(h, MOM_ESINGULAR, buf);
  }
  return MOM_OK;
}

static double *rrs_which(mom_t *h, int which, bool *matrix, size_t *nblk) {
  momr::State *s = h->rrs;
  if (which < 0 || which >= 30) return nullptr;
  const int grp = which / 6, k = which % 6;
  *matrix = k < 4;
  *nblk = (size_t)s->S * (grp >= 3 ? (size_t)s->nR : 1);
  switch (grp) {
    case 0: return s->added[(k == momr::R_PM || k == momr::T_MM) ? 0 : s->cur][k];
    case 1: return s->comp[s->ccur][k];
    case 2: return s->surf[k];
    case 3: return s->ie_added[k];
    default: return s->ie_comp[k];
  }
}
extern "C" int mom_rrs_upload(mom_t *h, int which, const double *src) {
  int rc = rrs_ready(h, "mom_rrs_upload");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  bool matrix = false;
  size_t nblk = 0;
  double *p = rrs_which(h, which, &matrix, &nblk);
  if (!p || !src) return fail(h, MOM_EINVAL, "mom_rrs_upload: bad argument");
  if (which >= 18 && which < 24) {
    RRSCHK(h, momr::ensure_pm(h->rrs, rrs_streams(h)));
    momr::mark_uploaded(h->rrs);
  }
  HIPCHK(h, momr::upload(h->rrs, p, src, matrix, nblk));  // ABI memory order -> padded device blocks
  return MOM_OK;
}
extern "C" int mom_rrs_download(mom_t *h, int which, double *dst) {
  int rc = rrs_ready(h, "mom_rrs_download");
  if (rc) return rc;
  bool matrix = false;
  size_t nblk = 0;
  double *p = rrs_which(h, which, &matrix, &nblk);
  if (!p || !dst) return fail(h, MOM_EINVAL, "mom_rrs_download: bad argument");
  if (which >= 18 && which < 24) RRSCHK(h, momr::ensure_pm(h->rrs, rrs_streams(h)));
  HIPCHK(h, momr::download(h->rrs, dst, p, matrix, nblk));
  return MOM_OK;
}

extern "C" int mom_rrs_elemental(mom_t *h, int m, int ndoubl, const double *tau_sum, const double *dtau, const double *varpi,
                                 const double *Zpp, const double *Zmp, const double *fscattRayl, const double *Zpp_l1l0,
                                 const double *Zmp_l1l0) {
  int rc = rrs_ready(h, "mom_rrs_elemental");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  if (!tau_sum || !dtau || !varpi || !Zpp || !Zmp || !fscattRayl || !Zpp_l1l0 || !Zmp_l1l0 || ndoubl < 0 || ndoubl > 62)
    return fail(h, MOM_EINVAL, "mom_rrs_elemental: bad argument");
  const size_t S = h->S, NN = (size_t)h->N * h->N;
  const double *src[8] = {tau_sum, dtau, varpi, fscattRayl, Zpp, Zmp, Zpp_l1l0, Zmp_l1l0};
  for (int k = 0; k < 8; ++k) {
    const size_t cnt = (k < 4) ? S : NN;
    if (!h->d_rrs_op[k]) HIPCHK(h, h->d_rrs_op[k].renew(cnt));
    HIPCHK(h, hipMemcpyAsync(h->d_rrs_op[k], src[k], cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  const MomDevBuf<double> *d = h->d_rrs_op;
  RRSCHK(h, momr::elemental(h->rrs, rrs_streams(h), m, ndoubl, 0, d[0], d[1], d[2], d[4], d[5], 1, nullptr, d[3], d[6], d[7], true, true));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_rrs_doubling(mom_t *h, int ndoubl, double *expk) {
  int rc = rrs_ready(h, "mom_rrs_doubling");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  if (ndoubl < 0 || !expk) return fail(h, MOM_EINVAL, "mom_rrs_doubling: bad argument");
  momr::State *s = h->rrs;
  HIPCHK(h, hipMemcpyAsync(s->expk[s->cur], expk, (size_t)h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  RRSCHK(h, momr::doubling(s, rrs_streams(h), ndoubl));
  HIPCHK(h, hipMemcpyAsync(expk, s->expk[s->cur], (size_t)h->S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return rrs_check(h);
}

extern "C" int mom_rrs_interaction(mom_t *h, int iface, int with_surface_layer) {
  int rc = rrs_ready(h, "mom_rrs_interaction");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  if (iface < 0 || iface > 3) return fail(h, MOM_EINVAL, "mom_rrs_interaction: iface must be 0..3");
  RRSCHK(h, momr::interaction(h->rrs, rrs_streams(h), iface, with_surface_layer != 0));
  return rrs_check(h);
}

extern "C" int mom_rrs_copy_added_to_composite(mom_t *h) {
  int rc = rrs_ready(h, "mom_rrs_copy_added_to_composite");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  RRSCHK(h, momr::copy_added_to_composite(h->rrs, rrs_streams(h)));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_rrs_surface_lambertian(mom_t *h, int m, double albedo, const double *tau_tot) {
  int rc = rrs_ready(h, "mom_rrs_surface_lambertian");
  if (rc) return rc;
  h->rrs->dirty = true;  // operator-level write: the next scene-level run starts from zeroed layers again
  if (!tau_tot) return fail(h, MOM_EINVAL, "mom_rrs_surface_lambertian: bad argument");
  HIPCHK(h, hipMemcpyAsync(h->d_vec[0], tau_tot, (size_t)h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
  RRSCHK(h, momr::surface(h->rrs, rrs_streams(h), m, 0, albedo, h->d_vec[0], nullptr, nullptr));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_scene_set_rrs(mom_t *h, const double *fscattRayl, const double *Zpp_l1l0, const double *Zmp_l1l0) {
  int rc = rrs_ready(h, "mom_scene_set_rrs");
  if (rc) return rc;
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_scene_set_rrs: call mom_scene_set / mom_scene_set_optics first");
  // Zpp_l1l0 == Zmp_l1l0 == NULL: the staged Raman set (mom_scene_stage_greeks, which = 1), if any
  const bool staged = !Zpp_l1l0 && !Zmp_l1l0 && h->stage_r.live;
  if (!fscattRayl || (!staged && (!Zpp_l1l0 || !Zmp_l1l0))) return fail(h, MOM_EINVAL, "mom_scene_set_rrs: bad argument");
  if (staged && h->stage_r.M != h->scene_M) {
    char buf[200];
    snprintf(buf, sizeof buf, "mom_scene_set_rrs: the scene has M = %d, but the staged Raman set (mom_scene_stage_greeks) is M = %d",
             h->scene_M, h->stage_r.M);
    return fail(h, MOM_EINVAL, buf);
  }
  if (h->Nk != h->N) return fail(h, MOM_ESTATE, "mom_scene_set_rrs: the scene was set with a padded operator edge (MOM_OPT_STRIP_PAD)");
  const size_t NN = (size_t)h->N * h->N;
  HIPCHK(h, mom_upload(h->d_fscatt, fscattRayl, (size_t)h->S * h->Nz, h->stream));
  if (staged) {  // [N, N, M] formed in d_Zr on the handle's stream: one set, block m
    MomGreekStage st = std::move(h->stage_r);
    h->stage_r.drop();
    const int M = h->scene_M, n_mu = h->N / h->nS;
    std::vector<double> mu((size_t)n_mu);
    for (int i = 0; i < n_mu; ++i) mu[i] = h->h_mu[(size_t)i * h->nS];
    std::vector<int> slot((size_t)M);
    for (int m = 0; m < M; ++m) slot[m] = m;
    MomZmomPlan pl;
    HIPCHK(h, mom_zmom_plan(pl, h->nS, n_mu, mu.data(), 1, st.l_pad, st.l_max.data(), st.greek.data(), 0, M, slot.data(), h->stream));
    HIPCHK(h, h->d_Zr[0].renew(NN * M));
    HIPCHK(h, h->d_Zr[1].renew(NN * M));
    HIPCHK(h, mom_zmom_launch(pl, h->stream, h->d_Zr[0], h->d_Zr[1], h->N, nullptr, nullptr, 0));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the plan and the stage go out of scope
    h->rrs_scene = true;
    return MOM_OK;
  }
  HIPCHK(h, mom_upload(h->d_Zr[0], Zpp_l1l0, NN * h->scene_M, h->stream));
  HIPCHK(h, mom_upload(h->d_Zr[1], Zmp_l1l0, NN * h->scene_M, h->stream));
  h->rrs_scene = true;
  return MOM_OK;
}

extern "C" int mom_rt_run_rrs(mom_t *h) {
  int rc = rrs_ready(h, "mom_rt_run_rrs");
  if (rc) return rc;
  if (!h->scene_set || !h->rrs_scene) return fail(h, MOM_ESTATE, "mom_rt_run_rrs: call mom_scene_set and mom_scene_set_rrs first");
  momr::State *s = h->rrs;
  const momr::Streams q = rrs_streams(h);
  const size_t S = h->S, NN = (size_t)h->N * h->N;
  const int Nz = h->Nz, K = h->K, M = h->scene_M;
  momr::timing_reset(s, true);
  s->fast = true;   // deferred inelastic elemental, derived ier+- / iet-- (corrected position)
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  RRSCHK(h, momr::begin_run(s, h->nVza));
  for (int m = 0; m < M; ++m) {
    for (int iz = 0; iz < Nz; ++iz) {                                              // rt_run.jl:143-165
      const int nd = h->nd[iz];
      RRSCHK(h, momr::elemental(s, q, m, nd, nd, h->d_tau_sum + S * iz, h->d_tau + S * iz, h->d_varpi + S * iz,
                                h->d_Zpp + NN * K * m, h->d_Zmp + NN * K * m, K, h->d_zw + (size_t)K * S * iz,
                                h->d_fscatt + S * iz, h->d_Zr[0] + NN * m, h->d_Zr[1] + NN * m, true, true));
      RRSCHK(h, momr::doubling(s, q, nd));
      if (iz == 0) RRSCHK(h, momr::copy_added_to_composite(s, q));                    // rt_kernel.jl:326-333
      else RRSCHK(h, momr::interaction(s, q, h->iface[iz], false));
    }
    RRSCHK(h, momr::surface(s, q, m, h->surf_kind, h->albedo, h->d_tau_sum + S * Nz,            // rt_run.jl:168-175
                            h->surf_kind == 1 ? h->d_Rsurf + NN * m : nullptr, h->d_albedo_spec));
    RRSCHK(h, momr::interaction(s, q, h->iface[Nz - 1], true));                    // rt_run.jl:179-185 (Q6)
    RRSCHK(h, momr::postprocess(s, q, m, h->nVza, h->d_node, h->d_cos, h->d_sin, M, m == 0 ? 0.5 : 1.0));
  }
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  s->timing = false;
  s->fast = false;
  return MOM_OK;
}

extern "C" int mom_get_hdr_rrs(mom_t *h, double *hdr, double *bhr_uw, double *bhr_dw) {
  int rc = rrs_ready(h, "mom_get_hdr_rrs");
  if (rc) return rc;
  momr::State *s = h->rrs;
  if (!s->d_out || !hdr || !bhr_uw || !bhr_dw) return fail(h, MOM_ESTATE, "mom_get_hdr_rrs: no run / null output");
  const size_t tot = (size_t)s->out_nVza * h->nS * h->S, fl = (size_t)h->nS * h->S;
  HIPCHK(h, hipMemcpyAsync(hdr, s->d_out + 4 * tot, tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(bhr_uw, s->d_out + 5 * tot, fl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(bhr_dw, s->d_out + 5 * tot + fl, fl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// The seven spectra of rt_run(::RRS)'s return tuple (rt_run.jl:226), restricted to the points this rank owns
// (mom_rrs_set_shard: [n1_lo, n1_hi) of the window), packed on the device: [R | T | ieR | ieT | hdr][nVza, nStokes, per],
// then [bhr_uw | bhr_dw][nStokes, per]; `per` >= the owned count, the tail of every spectrum is zero (ragged last shard).
// The spectral index is the slowest one of every output array, so an owned slice is one contiguous piece per spectrum.
static int rrs_pack_owned(mom_t *h, int per, double *d_dst) {
  momr::State *s = h->rrs;
  if (!s->d_out) return fail(h, MOM_ESTATE, "mom_get_spectra_rrs_device: no run");
  const int own = s->n1_hi - s->n1_lo;
  if (per < own || per <= 0) return fail(h, MOM_EINVAL, "mom_get_spectra_rrs_device: per must be >= the owned point count");
  const size_t a = (size_t)s->out_nVza * h->nS, b = (size_t)h->nS, S = (size_t)h->S;
  if (own < per) HIPCHK(h, hipMemsetAsync(d_dst, 0, mom_rrs_spectra_count(h, per) * sizeof(double), h->stream));
  for (int k = 0; k < 7; ++k) {
    const size_t row = k < 5 ? a : b;
    const double *src = (k < 5 ? s->d_out + (size_t)k * a * S : s->d_out + 5 * a * S + (size_t)(k - 5) * b * S) + row * s->n1_lo;
    double *dst = k < 5 ? d_dst + (size_t)k * a * per : d_dst + 5 * a * per + (size_t)(k - 5) * b * per;
    if (own > 0) HIPCHK(h, hipMemcpyAsync(dst, src, row * own * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  }
  return MOM_OK;
}

extern "C" size_t mom_rrs_spectra_count(mom_t *h, int per) {
  if (!h || !h->rrs || per <= 0) return 0;
  const int nV = h->rrs->out_nVza > 0 ? h->rrs->out_nVza : h->nVza;
  return ((size_t)5 * nV * h->nS + (size_t)2 * h->nS) * (size_t)per;
}

extern "C" int mom_get_spectra_rrs_device(mom_t *h, int per, void *d_local) {
  int rc = rrs_ready(h, "mom_get_spectra_rrs_device");
  if (rc) return rc;
  if (!d_local) return fail(h, MOM_EINVAL, "mom_get_spectra_rrs_device: null buffer");
  return rrs_pack_owned(h, per, static_cast<double *>(d_local));
}

// The ONE collective of a sharded RRS run: every rank contributes the packed block of its owned points
// (above) and receives d_global [nranks][mom_rrs_spectra_count(h, per)]; asynchronous on the handle's stream, nothing
// crosses the host.
extern "C" int mom_allgather_rrs_device(mom_t *h, int per, void *d_global) {
  int rc = rrs_ready(h, "mom_allgather_rrs_device");
  if (rc) return rc;
  if (!h->comm) return fail(h, MOM_ESTATE, "mom_allgather_rrs_device: call mom_comm_init first");
  if (!d_global) return fail(h, MOM_EINVAL, "mom_allgather_rrs_device: null buffer");
  const size_t cnt = mom_rrs_spectra_count(h, per);
  HIPCHK(h, h->d_rrs_send.reserve(cnt, h->stream));
  if ((rc = rrs_pack_owned(h, per, h->d_rrs_send))) return rc;
  return mom_allgather(h, h->d_rrs_send, d_global, cnt);
}

// test access: violations of the zero-padding invariant of the RRS layer arrays (mom_rrs.hip count_padding); 0 = intact
extern "C" int mom_rrs_check_padding(mom_t *h, unsigned long long *violations) {
  int rc = rrs_ready(h, "mom_rrs_check_padding");
  if (rc) return rc;
  if (!violations) return fail(h, MOM_EINVAL, "mom_rrs_check_padding: null output");
  RRSCHK(h, momr::ensure_pm(h->rrs, rrs_streams(h)));
  RRSCHK(h, momr::count_padding(h->rrs, violations));
  return MOM_OK;
}

extern "C" int mom_rrs_timers(mom_t *h, double *ms, int *launches, int n) {
  int rc = rrs_ready(h, "mom_rrs_timers");
  if (rc) return rc;
  if (!ms || !launches || n < momr::TK_COUNT + 1) return fail(h, MOM_EINVAL, "mom_rrs_timers: need room for 4 values");
  RRSCHK(h, momr::timing_read(h->rrs, ms, launches));
  float t = 0.f;
  if (hipEventElapsedTime(&t, h->ev[0], h->ev[3]) != hipSuccess) t = 0.f;
  ms[momr::TK_COUNT] = t;
  launches[momr::TK_COUNT] = 1;
  return MOM_OK;
}

extern "C" int mom_get_RT_rrs(mom_t *h, double *R_SFI, double *T_SFI, double *ieR_SFI, double *ieT_SFI, double *gpu_ms) {
  int rc = rrs_ready(h, "mom_get_RT_rrs");
  if (rc) return rc;
  momr::State *s = h->rrs;
  if (!s->d_out) return fail(h, MOM_ESTATE, "mom_get_RT_rrs: no run");
  const size_t tot = (size_t)s->out_nVza * h->nS * h->S;
  double *dst[4] = {R_SFI, T_SFI, ieR_SFI, ieT_SFI};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIPCHK(h, hipMemcpyAsync(dst[k], s->d_out + tot * k, tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if ((rc = rrs_check(h))) return rc;
  if (gpu_ms) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[0], h->ev[3]) != hipSuccess) ms = 0.f;
    *gpu_ms = ms;
  }
  return MOM_OK;
}
