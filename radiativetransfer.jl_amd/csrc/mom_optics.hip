// mom_optics.hip -- the device-side layer optics of the C ABI (include/momcore.h): the resident absorption table
// and the Voigt entry points (kernels: voigt.hip), k_optics and mom_scene_set_optics, mom_scene_get_layers, the Dual run of the
// layer optics: k_optics_dual and mom_scene_set_optics_partials, mom_scene_get_partials, and both for band-resolved scenes:
// k_optics_bands / mom_scene_set_optics_bands, k_optics_bands_dual / mom_scene_set_optics_bands_partials.
#include <cstring>

#include "mom_handle.hpp"

extern "C" int mom_absorption_begin(mom_t *h, int Nz, const double *grid) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (Nz <= 0) return fail(h, MOM_EINVAL, "mom_absorption_begin: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = h->S;
  h->optics_tables = false;  // a resident scene (mom_scene_set_optics) was assembled from the table that goes here
  HIPCHK(h, h->d_tau_abs.renew(S * Nz));
  HIPCHK(h, hipMemsetAsync(h->d_tau_abs, 0, S * Nz * sizeof(double), h->stream));  // τ_abs = zeros (model_from_parameters.jl:48)
  if (h->d_dtau_abs) {  // the partials restart with the table
    if (Nz != h->abs_Nz) HIPCHK(h, h->d_dtau_abs.renew(2 * S * Nz));
    HIPCHK(h, hipMemsetAsync(h->d_dtau_abs, 0, 2 * S * Nz * sizeof(double), h->stream));
  }
  h->abs_Nz = Nz;
  if (grid) {
    HIPCHK(h, mom_upload(h->d_grid, grid, S, h->stream));
    // what mom_lut_tau_abs_profile asks of the grid: its extent against the table's nu axis, and whether it is monotone
    bool up = true, down = true;
    h->grid_min = h->grid_max = grid[0];
    for (size_t n = 1; n < S; ++n) {
      up = up && grid[n] >= grid[n - 1];
      down = down && grid[n] <= grid[n - 1];
      h->grid_min = std::min(h->grid_min, grid[n]);
      h->grid_max = std::max(h->grid_max, grid[n]);
    }
    for (size_t n = 0; n < S; ++n)
      if (grid[n] != grid[n]) h->grid_min = h->grid_max = grid[n];   // a NaN is inside no axis
    h->grid_order = up ? 1 : (down ? -1 : 0);
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

extern "C" int mom_absorption_set(mom_t *h, int Nz, const double *tau_abs) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (Nz <= 0 || !tau_abs) return fail(h, MOM_EINVAL, "mom_absorption_set: bad argument");
  int rc = mom_absorption_begin(h, Nz, nullptr);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->d_tau_abs, tau_abs, (size_t)h->S * Nz * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->d_dtau_abs.reset();  // a host table has no partials
  return MOM_OK;
}

extern "C" int mom_absorption_get(mom_t *h, double *tau_abs) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->d_tau_abs || !tau_abs) return fail(h, MOM_ESTATE, "mom_absorption_get: no resident tau_abs table / null output");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(tau_abs, h->d_tau_abs, (size_t)h->S * h->abs_Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// HitranModel.broadening / .CEF of every later absorption call on the handle (Absorption/types.jl; parameters_from_yaml.jl:114-115)
extern "C" int mom_absorption_set_model(mom_t *h, int broadening, int cef) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  std::string err;
  if (mom_line_shape("mom_absorption_set_model", broadening, cef, &err) < 0) return fail(h, MOM_EINVAL, err.c_str());
  h->abs_broadening = broadening;
  h->abs_cef = cef;
  return MOM_OK;
}

namespace {
// the kernels' shape of the handle's model (cannot fail: mom_absorption_set_model checked the codes)
int handle_shape(const mom_t *h) {
  std::string err;
  return mom_line_shape("", h->abs_broadening, h->abs_cef, &err);
}
// mom_voigt_tau_abs / _dual take no gamma_l: Voigt with the handle's CEF, MOM_ESTATE under another broadening
int voigt_only(mom_t *h, const char *fn) {
  if (h->abs_broadening == MOM_BROADENING_VOIGT) return MOM_OK;
  char buf[200];
  snprintf(buf, sizeof buf, "%s: the handle's broadening (mom_absorption_set_model) is not Voigt; call mom_lineshape_tau_abs%s, which takes gamma_l",
           fn, strstr(fn, "_dual") ? "_dual" : "");
  return fail(h, MOM_ESTATE, buf);
}
// the checks the host-prefactor entry points share; line[] = nu, gamma_d, y, S, gamma_l
int lineshape_args(mom_t *h, const char *fn, int shape, int iz_1based, int nLines, const double *const *line, const int *ind_start_1based,
                   const int *ind_stop_1based) {
  char buf[200];
  const int rc = mom_absorption_state(h, fn, true, false);
  if (rc) return rc;
  bool lines_ok = ind_start_1based && ind_stop_1based;
  for (int k = 0; k < 5; ++k) lines_ok = lines_ok && (line[k] || !mom_shape_reads(shape, k));
  if (iz_1based < 1 || iz_1based > h->abs_Nz || nLines < 0 || (nLines > 0 && !lines_ok)) {
    snprintf(buf, sizeof buf, "%s: bad argument", fn);
    return fail(h, MOM_EINVAL, buf);
  }
  for (int j = 0; j < nLines; ++j)
    if (ind_start_1based[j] < 1 || ind_stop_1based[j] > h->S) {
      snprintf(buf, sizeof buf, "%s: line %d: window [%d, %d] outside the grid 1..%d", fn, j + 1, ind_start_1based[j], ind_stop_1based[j],
               h->S);
      return fail(h, MOM_EINVAL, buf);
    }
  return MOM_OK;
}
bool windows_sorted(int nLines, const int *i0, const int *i1) {
  for (int j = 1; j < nLines; ++j)
    if (i0[j] < i0[j - 1] || i1[j] < i1[j - 1]) return false;
  return true;
}
// dtau_abs [S, abs_Nz, 2], allocated and zeroed by the first Dual call after mom_absorption_begin
int dual_table(mom_t *h) {
  if (h->d_dtau_abs) return MOM_OK;
  const size_t n = 2 * (size_t)h->S * h->abs_Nz;
  HIPCHK(h, h->d_dtau_abs.renew(n));
  HIPCHK(h, hipMemsetAsync(h->d_dtau_abs, 0, n * sizeof(double), h->stream));
  return MOM_OK;
}
// The one owner of the handle's line buffers: d_lines as a block of `nz` layers with room for `nLines` lines each and, Dual run,
// d_dlines as the partial block to match.  A block is kept while it has the layer count asked for and the capacity the rule gives
// for nLines fits its stride (so a repeated call allocates nothing, and no entry point ever gets less room than the rule gives);
// otherwise it is allocated afresh, after the stream that may still read the old one has drained.  d_dlines only grows.
int line_blocks(mom_t *h, int nLines, int nz, MomLineBlock *pf, MomLinePartialBlock *dpf) {
  const size_t cap = MomLineBlock::capacity_for((size_t)nLines);
  if (!h->d_lines || cap > h->lines_per || nz != h->lines_nz) {
    if (h->d_lines) { HIPCHK(h, hipStreamSynchronize(h->stream)); h->d_lines.reset(); h->lines_per = 0; }
    HIPCHK(h, h->d_lines.renew(MomLineBlock{nullptr, cap, nz}.doubles()));
    h->lines_per = cap;
    h->lines_nz = nz;
  }
  *pf = MomLineBlock{h->d_lines, h->lines_per, nz};
  if (!dpf) return MOM_OK;
  HIPCHK(h, h->d_dlines.reserve(pf->partials(nullptr).doubles(), h->stream));
  *dpf = pf->partials(h->d_dlines);
  return MOM_OK;
}
// the blocks as the last call left them, for the test-access getters: they read the LAST layer of the last call
MomLineBlock resident_lines(const mom_t *h) { return {h->d_lines, h->lines_per, std::max(h->lines_nz, 1)}; }
MomLinePartialBlock resident_partials(const mom_t *h) { return resident_lines(h).partials(h->d_dlines); }
bool partials_resident(const mom_t *h) { return h->d_dlines && h->d_dlines.capacity() >= resident_partials(h).doubles(); }

// mom_voigt_tau_abs, mom_lineshape_tau_abs and, with dline[], their Dual runs: dline[] = the partials of line[], each [nLines, 2]
// column-major or null (zeros)
int lineshape_tau_abs_run(mom_t *h, const char *fn, int shape, int iz_1based, int nLines, const double *const *line,
                          const double *const *dline, const int *ind_start_1based, const int *ind_stop_1based, double factor) {
  int rc = lineshape_args(h, fn, shape, iz_1based, nLines, line, ind_start_1based, ind_stop_1based);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  if (dline && (rc = dual_table(h))) return rc;
  if (nLines == 0) return MOM_OK;
  const int sorted = windows_sorted(nLines, ind_start_1based, ind_stop_1based) ? 1 : 0;
  const size_t lb = (size_t)nLines;
  MomLineBlock pf;
  MomLinePartialBlock dpf;
  if ((rc = line_blocks(h, nLines, 1, &pf, dline ? &dpf : nullptr))) return rc;
  MomLineOut ln = pf.layer(0);
  // the host arrays are borrowed for the call only: the copies must have left them before we return
  for (int k = 0; k < 5; ++k)
    if (line[k] && mom_shape_reads(shape, k))
      HIPCHK(h, hipMemcpyAsync(ln.prefactor(k), line[k], lb * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ln.i0, ind_start_1based, lb * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ln.i1, ind_stop_1based, lb * sizeof(int), hipMemcpyHostToDevice, h->stream));
  MomLinePartialsOut dln{};
  if (dline) dln = dpf.layer(0);
  for (int q = 0; q < 5 && dline; ++q)   // a null array: zeros
    for (int k = 0; k < 2; ++k) {
      double *dst = dln.partial(q) + dln.ks * k;
      if (dline[q]) HIPCHK(h, hipMemcpyAsync(dst, dline[q] + lb * k, lb * sizeof(double), hipMemcpyHostToDevice, h->stream));
      else HIPCHK(h, hipMemsetAsync(dst, 0, lb * sizeof(double), h->stream));
    }
  const MomLinePartials dread = dln;
  const size_t col = (size_t)h->S * (iz_1based - 1);
  HIPCHK(h, mom_voigt_launch(h->stream, shape, nLines, ln, dline ? &dread : nullptr, h->S, h->d_grid, h->d_tau_abs + col,
                             dline ? h->d_dtau_abs + col : nullptr, (size_t)h->S * h->abs_Nz, factor, 1, sorted));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}
}  // namespace

extern "C" int mom_voigt_tau_abs(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *y,
                                 const double *S, const int *ind_start_1based, const int *ind_stop_1based, double factor) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const int rc = voigt_only(h, "mom_voigt_tau_abs");
  if (rc) return rc;
  const double *line[5] = {nu, gamma_d, y, S, nullptr};
  return lineshape_tau_abs_run(h, "mom_voigt_tau_abs", handle_shape(h), iz_1based, nLines, line, nullptr, ind_start_1based, ind_stop_1based, factor);
}

// mom_voigt_tau_abs for the handle's model: the five prefactors line_shape! takes (compute_absorption_cross_section.jl:118-124)
extern "C" int mom_lineshape_tau_abs(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *gamma_l,
                                     const double *y, const double *S, const int *ind_start_1based, const int *ind_stop_1based,
                                     double factor) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const double *line[5] = {nu, gamma_d, y, S, gamma_l};
  return lineshape_tau_abs_run(h, "mom_lineshape_tau_abs", handle_shape(h), iz_1based, nLines, line, nullptr, ind_start_1based,
                               ind_stop_1based, factor);
}

// ---- The Dual run of the absorption path: tau_abs and its partials with respect to the layer's pressure (k = 0) and temperature
// (k = 1), ForwardDiff.Dual through compute_absorption_cross_section as absorption_cross_section(...; autodiff = true) runs it
// (autodiff_helper.jl:17-51).  Works on Float64 and Float32 handles alike: the absorption table is Float64 on both.
extern "C" int mom_voigt_tau_abs_dual(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *y,
                                      const double *S, const double *dnu, const double *dgamma_d, const double *dy, const double *dS,
                                      const int *ind_start_1based, const int *ind_stop_1based, double factor) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const int rc = voigt_only(h, "mom_voigt_tau_abs_dual");
  if (rc) return rc;
  const double *line[5] = {nu, gamma_d, y, S, nullptr}, *dline[5] = {dnu, dgamma_d, dy, dS, nullptr};
  return lineshape_tau_abs_run(h, "mom_voigt_tau_abs_dual", handle_shape(h), iz_1based, nLines, line, dline, ind_start_1based,
                               ind_stop_1based, factor);
}

// mom_voigt_tau_abs_dual for the handle's model
extern "C" int mom_lineshape_tau_abs_dual(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d,
                                          const double *gamma_l, const double *y, const double *S, const double *dnu,
                                          const double *dgamma_d, const double *dgamma_l, const double *dy, const double *dS,
                                          const int *ind_start_1based, const int *ind_stop_1based, double factor) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const double *line[5] = {nu, gamma_d, y, S, gamma_l}, *dline[5] = {dnu, dgamma_d, dy, dS, dgamma_l};
  return lineshape_tau_abs_run(h, "mom_lineshape_tau_abs_dual", handle_shape(h), iz_1based, nLines, line, dline, ind_start_1based,
                               ind_stop_1based, factor);
}

extern "C" int mom_absorption_get_partials(mom_t *h, double *dtau_abs) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->d_dtau_abs || !dtau_abs) return fail(h, MOM_ESTATE, "mom_absorption_get_partials: no resident dtau_abs table (no Dual call since the table was set) / null output");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(dtau_abs, h->d_dtau_abs, 2 * (size_t)h->S * h->abs_Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// Resident line table of one absorber: the HITRAN columns of the lines inside the padded grid (the host selects them once,
// compute_absorption_cross_section.jl:54-72) and the TIPS-2017 spline tables of their isotopologues (qoft! :197-214: knots,
// values and the second derivatives of DataInterpolations.CubicSpline, computed once by the host in the tables' Float32).
extern "C" int mom_absorption_set_lines(mom_t *h, int nLines, const double *nu0, const double *S0, const double *gamma_air,
                                        const double *gamma_self, const double *E_lower, const double *n_air,
                                        const double *delta_air, const double *sqrt_mol_weight, const int *iso_index, int nIso,
                                        int nTmax, const int *nT, const double *tips_T, const double *tips_Q, const double *tips_z) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (nLines < 0 || nIso < 0 || nTmax < 0 || (nLines > 0 && (!nu0 || !S0 || !gamma_air || !gamma_self || !E_lower || !n_air ||
      !delta_air || !sqrt_mol_weight || !iso_index)) || (nIso > 0 && (nTmax < 2 || !nT || !tips_T || !tips_Q || !tips_z)))
    return fail(h, MOM_EINVAL, "mom_absorption_set_lines: bad argument");
  for (int j = 0; j < nLines; ++j)
    if (E_lower[j] != -1.0 && (iso_index[j] < 0 || iso_index[j] >= nIso))
      return fail(h, MOM_EINVAL, "mom_absorption_set_lines: iso_index out of range");
  for (int k = 0; k < nIso; ++k)
    if (nT[k] < 2 || nT[k] > nTmax) return fail(h, MOM_EINVAL, "mom_absorption_set_lines: bad knot count");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->d_lt.reset(); h->d_lt_i.reset();
  h->lt = MomLineTable{};
  const size_t L = (size_t)std::max(nLines, 1), Tn = (size_t)std::max(nIso, 1) * std::max(nTmax, 1);
  HIPCHK(h, h->d_lt.renew(8 * L + 3 * Tn));
  HIPCHK(h, h->d_lt_i.renew(L + std::max(nIso, 1) + 1));
  const double *cols[8] = {nu0, S0, gamma_air, gamma_self, E_lower, n_air, delta_air, sqrt_mol_weight};
  for (int k = 0; k < 8 && nLines > 0; ++k) HIPCHK(h, hipMemcpy(h->d_lt + k * L, cols[k], (size_t)nLines * sizeof(double), hipMemcpyHostToDevice));
  const double *tabs[3] = {tips_T, tips_Q, tips_z};
  for (int k = 0; k < 3 && nIso > 0; ++k) HIPCHK(h, hipMemcpy(h->d_lt + 8 * L + k * Tn, tabs[k], (size_t)nIso * nTmax * sizeof(double), hipMemcpyHostToDevice));
  if (nLines > 0) HIPCHK(h, hipMemcpy(h->d_lt_i, iso_index, (size_t)nLines * sizeof(int), hipMemcpyHostToDevice));
  if (nIso > 0) HIPCHK(h, hipMemcpy(h->d_lt_i + L, nT, (size_t)nIso * sizeof(int), hipMemcpyHostToDevice));
  MomLineTable &t = h->lt;
  t.nLines = nLines; t.nIso = nIso; t.nTmax = nTmax;
  t.nu0 = h->d_lt; t.S0 = h->d_lt + L; t.g_air = h->d_lt + 2 * L; t.g_self = h->d_lt + 3 * L; t.E = h->d_lt + 4 * L;
  t.n_air = h->d_lt + 5 * L; t.d_air = h->d_lt + 6 * L; t.sqw = h->d_lt + 7 * L;
  t.tT = h->d_lt + 8 * L; t.tQ = t.tT + Tn; t.tZ = t.tQ + Tn;
  t.iso = h->d_lt_i; t.nT = h->d_lt_i + L;
  // the common validity range of the TIPS tables in use (qoft! asserts Tmin < T < Tmax, :204)
  h->lt_Tmin = -1e300; h->lt_Tmax = 1e300;
  for (int k = 0; k < nIso; ++k) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < nT[k]; ++i) { lo = std::min(lo, tips_T[(size_t)k * nTmax + i]); hi = std::max(hi, tips_T[(size_t)k * nTmax + i]); }
    h->lt_Tmin = std::max(h->lt_Tmin, lo); h->lt_Tmax = std::min(h->lt_Tmax, hi);
  }
  return MOM_OK;
}

// compute_absorption_profile! for ONE layer (atmo_prof.jl:427-449) with the per-line prefactors formed ON THE DEVICE from the
// resident table: only (p, T, vmr, wing_cutoff, factor) cross the bus.
extern "C" int mom_voigt_tau_abs_layer(mom_t *h, int iz_1based, double pressure, double temperature, double vmr,
                                       double wing_cutoff, double factor) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  int rc = mom_absorption_state(h, "mom_voigt_tau_abs_layer", true, true);
  if (rc) return rc;
  if (iz_1based < 1 || iz_1based > h->abs_Nz || !(temperature > 0.0)) return fail(h, MOM_EINVAL, "mom_voigt_tau_abs_layer: bad argument");
  if ((rc = mom_tips_range(h, temperature))) return rc;
  const int nLines = h->lt.nLines;
  if (nLines == 0) return MOM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  MomLineBlock pf;
  if ((rc = line_blocks(h, nLines, 1, &pf, nullptr))) return rc;
  const MomLineOut ln = pf.layer(0);
  int *flag = h->d_lt_i + (size_t)std::max(nLines, 1) + std::max(h->lt.nIso, 1);
  HIPCHK(h, hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  HIPCHK(h, mom_line_prefactors_launch(h->stream, h->lt, h->S, h->d_grid, pressure, temperature, vmr, wing_cutoff, mom_doppler_scale(temperature),
                                       ln, flag));
  int unsorted = 0;
  HIPCHK(h, hipMemcpyAsync(&unsorted, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, mom_voigt_launch(h->stream, handle_shape(h), nLines, ln, nullptr, h->S, h->d_grid, h->d_tau_abs + (size_t)h->S * (iz_1based - 1),
                             nullptr, 0, factor, 1, unsorted ? 0 : 1));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// compute_absorption_profile! for ALL layers of a profile (atmo_prof.jl:427-449) in two launches: the reference walks the
// layers on the host and, per layer, launches one line-shape kernel per line; at its operating point (O2 A-band at
// 0.015 cm^-1, wing cut-off 40 cm^-1, 40 layers) a per-layer launch covers 90 workgroups -- a third of the GPU -- and the
// host round trips between the layers cost more than the arithmetic.  Here blockIdx.y = layer.  gpu_ms (optional): HIP-event
// time of the two kernels.
namespace {
// mom_voigt_tau_abs_profile and its Dual run; `fn` is the entry point's name in the error texts
int voigt_profile_run(mom_t *h, const char *fn, bool dual, int Nz, const double *pressure, const double *temperature, double vmr,
                      double wing_cutoff, const double *factor, double *gpu_ms) {
  char buf[200];
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  int rc = mom_absorption_state(h, fn, true, true);
  if (rc) return rc;
  snprintf(buf, sizeof buf, "%s: bad argument", fn);
  if (Nz < 1 || Nz > h->abs_Nz || !pressure || !temperature || !factor) return fail(h, MOM_EINVAL, buf);
  for (int z = 0; z < Nz; ++z) {
    if (!(temperature[z] > 0.0)) return fail(h, MOM_EINVAL, buf);
    if ((rc = mom_tips_range(h, temperature[z]))) return rc;
  }
  if (gpu_ms) *gpu_ms = 0.0;
  HIPCHK(h, hipSetDevice(h->device));
  if (dual && (rc = dual_table(h))) return rc;
  const int nLines = h->lt.nLines;
  if (nLines == 0) return MOM_OK;
  MomLineBlock pf;
  MomLinePartialBlock dpf;
  if ((rc = line_blocks(h, nLines, Nz, &pf, dual ? &dpf : nullptr))) return rc;
  // per-layer scalars [p | T | cgd | factor][Nz] (Dual run: | d cgd / dT) and the Nz sortedness flags
  const size_t nprm = dual ? 5 : 4;
  const size_t prm_doubles = nprm * (size_t)Nz + ((size_t)Nz + 1) / 2;
  HIPCHK(h, h->d_prof.reserve(prm_doubles, h->stream));
  std::vector<double> prm(nprm * (size_t)Nz);
  for (int z = 0; z < Nz; ++z) {
    prm[z] = pressure[z];
    prm[Nz + z] = temperature[z];
    prm[2 * (size_t)Nz + z] = mom_doppler_scale(temperature[z]);
    prm[3 * (size_t)Nz + z] = factor[z];
    if (dual) prm[4 * (size_t)Nz + z] = mom_doppler_scale_dT(temperature[z]);
  }
  HIPCHK(h, hipMemcpyAsync(h->d_prof, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  int *flags = reinterpret_cast<int *>(h->d_prof + nprm * (size_t)Nz);
  HIPCHK(h, hipMemsetAsync(flags, 0, sizeof(int) * (size_t)Nz, h->stream));
  if (gpu_ms) {
    for (int k = 0; k < 2; ++k)
      if (!h->ev_voigt[k]) HIPCHK(h, hipEventCreate(&h->ev_voigt[k]));
    HIPCHK(h, hipEventRecord(h->ev_voigt[0], h->stream));
  }
  HIPCHK(h, mom_voigt_profile_launch(h->stream, handle_shape(h), h->lt, pf, dual ? &dpf : nullptr, h->S, h->d_grid, h->d_prof, vmr, wing_cutoff,
                                     flags, h->d_tau_abs, dual ? h->d_dtau_abs.get() : nullptr, h->d_prof + 3 * (size_t)Nz));
  if (gpu_ms) HIPCHK(h, hipEventRecord(h->ev_voigt[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // prm is a host temporary
  if (gpu_ms) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev_voigt[0], h->ev_voigt[1]) == hipSuccess) *gpu_ms = ms;
  }
  return MOM_OK;
}
}  // namespace

extern "C" int mom_voigt_tau_abs_profile(mom_t *h, int Nz, const double *pressure, const double *temperature, double vmr,
                                         double wing_cutoff, const double *factor, double *gpu_ms) {
  return voigt_profile_run(h, "mom_voigt_tau_abs_profile", false, Nz, pressure, temperature, vmr, wing_cutoff, factor, gpu_ms);
}
// Its Dual run: the same two launches also form the prefactors' partials and add d_k sigma * factor into dtau_abs[:, iz, k]
extern "C" int mom_voigt_tau_abs_profile_dual(mom_t *h, int Nz, const double *pressure, const double *temperature, double vmr,
                                              double wing_cutoff, const double *factor, double *gpu_ms) {
  return voigt_profile_run(h, "mom_voigt_tau_abs_profile_dual", true, Nz, pressure, temperature, vmr, wing_cutoff, factor, gpu_ms);
}

// the partials of the prefactors of the last Dual call (test access), each [n, 2] column-major
extern "C" int mom_absorption_get_prefactor_partials(mom_t *h, int n, double *dnu, double *dgamma_d, double *dy, double *dS) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const MomLineBlock pf = resident_lines(h);
  if (!h->d_lines || n < 0 || (size_t)n > pf.cap || !partials_resident(h))
    return fail(h, MOM_ESTATE, "mom_absorption_get_prefactor_partials: no prefactor partials resident");
  HIPCHK(h, hipSetDevice(h->device));
  MomLinePartialsOut dln = resident_partials(h).layer(pf.nz - 1);
  double *dst[4] = {dnu, dgamma_d, dy, dS};
  for (int q = 0; q < 4; ++q)
    for (int k = 0; k < 2 && dst[q]; ++k)
      HIPCHK(h, hipMemcpy(dst[q] + (size_t)n * k, dln.partial(q) + dln.ks * k, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return MOM_OK;
}

// the prefactors of the last mom_voigt_tau_abs / mom_voigt_tau_abs_layer call (test access); n = its number of lines
extern "C" int mom_absorption_get_prefactors(mom_t *h, int n, double *nu, double *gamma_d, double *y, double *S, int *ind_start_1based,
                                             int *ind_stop_1based) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->d_lines || n < 0 || (size_t)n > h->lines_per) return fail(h, MOM_ESTATE, "mom_absorption_get_prefactors: no prefactors resident");
  HIPCHK(h, hipSetDevice(h->device));
  const MomLineBlock pf = resident_lines(h);
  MomLineOut ln = pf.layer(pf.nz - 1);
  double *dst[4] = {nu, gamma_d, y, S};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIPCHK(h, hipMemcpy(dst[k], ln.prefactor(k), (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (ind_start_1based) HIPCHK(h, hipMemcpy(ind_start_1based, ln.i0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  if (ind_stop_1based) HIPCHK(h, hipMemcpy(ind_stop_1based, ln.i1, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return MOM_OK;
}

// gamma_l (compute_absorption_cross_section.jl:82-84) of the last device-prefactor call (the LAST layer of a profile call) and,
// null to skip, its partials [n, 2] of the last Dual call (test access).  Only the device route fills the slot under every model.
extern "C" int mom_absorption_get_gamma_l(mom_t *h, int n, double *gamma_l, double *dgamma_l) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->d_lines || n < 0 || (size_t)n > h->lines_per) return fail(h, MOM_ESTATE, "mom_absorption_get_gamma_l: no prefactors resident");
  if (dgamma_l && !partials_resident(h)) return fail(h, MOM_ESTATE, "mom_absorption_get_gamma_l: no prefactor partials resident");
  HIPCHK(h, hipSetDevice(h->device));
  const MomLineBlock pf = resident_lines(h);
  if (gamma_l) HIPCHK(h, hipMemcpy(gamma_l, pf.layer(pf.nz - 1).gamma_l, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  const MomLinePartialsOut dln = resident_partials(h).layer(pf.nz - 1);
  for (int k = 0; k < 2 && dgamma_l; ++k)
    HIPCHK(h, hipMemcpy(dgamma_l + (size_t)n * k, dln.dgamma_l + dln.ks * k, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return MOM_OK;
}

// constructCoreOpticalProperties (compEffectiveLayerProperties.jl:1-78) with the `+` of types.jl:632-678, createAero
// (:80-85), the gas term (:672-678) and the cumulative τ_sum of extractEffectiveProps (:108), one thread per spectral
// point walking the layers; per-layer max(τ ϖ) for get_dtau_ndoubl / `scatter` by atomic max on the bit pattern
// (non-negative doubles order like their unsigned bit patterns).  Contraction off: the same IEEE operations as the
// host (numpy / Julia) path, so both routes give bitwise equal τ, ϖ, weights.
struct OpticsArgs {
  int S, Nz, nAer;
  double varpi_rayl;
  const double *tau_rayl, *tau_abs;  // [S,Nz]
  const double *aer;                 // [2,nAer,Nz]: τ_y, w_y = τ_y ϖ_y per aerosol type and layer (spectrally flat)
  const int *aer_mode;               // [nAer,Nz]: 0 = Rayleigh side all zero, 1 = mix, 2 = aerosol side all zero
  double *tau, *varpi, *zw, *tau_sum, *layer_max;
  // k_optics_bands only: `aer` and `aer_mode` are then one such block per band, [2,nAer,Nz,nBand] and [nAer,Nz,nBand]
  int nBand;
  const int *band_start;     // [nBand + 1]
  const double *varpi_band;  // [nBand] ϖ_Cabannes per band, in place of varpi_rayl
};
#pragma clang fp contract(off)
// One spectral point of one layer: Rayleigh `+` each aerosol type `+` the gas term; `aer` / `mode` are the [2,nAer,Nz] / [nAer,Nz]
// block of the point's band.  Leaves τ, ϖ and the 1 + nAer weights w of the point's own bases.
__device__ __forceinline__ void optics_point(const OpticsArgs &a, size_t o, int z, double varpi_rayl, const double *aer, const int *mode,
                                             double (&w)[8], double &tau, double &varpi) {
  const int K = 1 + a.nAer;
  tau = a.tau_rayl[o];
  varpi = varpi_rayl;
  w[0] = 1.0;
  for (int k = 1; k < K; ++k) w[k] = 0.0;
  for (int x = 0; x < a.nAer; ++x) {
    const double ty = aer[x + (size_t)a.nAer * z], wy = aer[a.nAer * a.Nz + x + (size_t)a.nAer * z];
    const int md = mode[x + (size_t)a.nAer * z];
    const double wx = tau * varpi, tot = wx + wy, tn = tau + ty;
    if (md == 0) {
      for (int k = 0; k < K; ++k) w[k] = 0.0;
      w[x + 1] = 1.0;
    } else if (md == 1) {
      const double fx = wx / tot;
      for (int k = 0; k < K; ++k) w[k] *= fx;
      w[x + 1] = wy / tot;
    }
    varpi = tot / tn;
    tau = tn;
  }
  const double tn = tau + a.tau_abs[o];
  varpi = (tau * varpi) / tn;
  tau = tn;
}
// max(τ ϖ) of a layer over the wavefront, then over the grid by atomic max on the bit pattern
__device__ __forceinline__ void optics_layer_max(double tw, double *layer_max) {
  // NaN (0/0 in an empty layer) must not win silently: fmax drops it like Julia's maximum would propagate it --
  // the host path would fail on such a scene as well; keep it visible as +inf
  if (tw != tw) tw = __longlong_as_double(0x7ff0000000000000ll);
  double m = tw;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0 && m > 0.0)
    atomicMax(reinterpret_cast<unsigned long long *>(layer_max), (unsigned long long)__double_as_longlong(m));
}
// the band of spectral point n < S: band_start is strictly ascending from 0 to S
__device__ __forceinline__ int optics_band(int n, int nBand, const int *band_start) {
  int b = 0;
  while (b + 1 < nBand && n >= band_start[b + 1]) ++b;
  return b;
}
__global__ void k_optics(OpticsArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = 1 + a.nAer;
  double tsum = 0.0;
  const bool live = n < a.S;
  if (live) a.tau_sum[n] = 0.0;
  for (int z = 0; z < a.Nz; ++z) {
    double tw = 0.0;
    if (live) {
      const size_t o = n + (size_t)a.S * z;
      double tau, varpi, w[8];
      optics_point(a, o, z, a.varpi_rayl, a.aer, a.aer_mode, w, tau, varpi);
      a.tau[o] = tau;
      a.varpi[o] = varpi;
      for (int k = 0; k < K; ++k) a.zw[k + (size_t)K * o] = w[k];
      tsum = tsum + 1.0 * tau;
      a.tau_sum[o + a.S] = tsum;
      tw = tau * varpi;
    }
    optics_layer_max(tw, a.layer_max + z);
  }
}

// k_optics for a band-resolved scene (constructCoreOpticalProperties' loop over iBand, compEffectiveLayerProperties.jl:24-75, and
// the concatenation `*` of types.jl:664-669): K = 1 + nAer nBand bases, basis 1 + x + nAer b = aerosol type x of band b.  A thread
// finds its band once and runs that band's statements -- its ϖ_Cabannes, its createAero columns, its three-way modes -- which are
// k_optics' own, so the results are bitwise the host twin's.  Of a point's K weights only the 1 + nAer of its own band can be
// nonzero: the host zeroes zw on the stream before the launch and a thread stores those alone.  The per-layer maxima run over all
// bands (rt_kernel.jl:241-242 takes them over the concatenated axis).
__global__ void k_optics_bands(OpticsArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = 1 + a.nAer * a.nBand;
  double tsum = 0.0;
  const bool live = n < a.S;
  const int b = live ? optics_band(n, a.nBand, a.band_start) : 0;
  const size_t AZ = (size_t)a.nAer * a.Nz;
  const double *aer = a.aer + 2 * AZ * b;
  const int *mode = a.aer_mode + AZ * b;
  const double varpi_rayl = a.varpi_band[b];
  if (live) a.tau_sum[n] = 0.0;
  for (int z = 0; z < a.Nz; ++z) {
    double tw = 0.0;
    if (live) {
      const size_t o = n + (size_t)a.S * z;
      double tau, varpi, w[8];
      optics_point(a, o, z, varpi_rayl, aer, mode, w, tau, varpi);
      a.tau[o] = tau;
      a.varpi[o] = varpi;
      double *zw = a.zw + (size_t)K * o;
      zw[0] = w[0];
      for (int x = 0; x < a.nAer; ++x) zw[1 + x + a.nAer * b] = w[x + 1];
      tsum = tsum + 1.0 * tau;
      a.tau_sum[o + a.S] = tsum;
      tw = tau * varpi;
    }
    optics_layer_max(tw, a.layer_max + z);
  }
}

// doubling_number (rt_helper_functions.jl:31-57): log10 arithmetic and the eps test as in the reference
static int doubling_number_host(double dtau_max, double tau_end) {
  if (tau_end <= dtau_max) return 0;
  const double q1 = std::log10(2.0), q2 = std::log10(dtau_max), q3 = std::log10(tau_end);
  const double tlimit = (q3 - q2) / q1, nlimit = std::floor(tlimit);
  if (tlimit - nlimit < 2.220446049250313e-16) return (int)nlimit;
  return (int)nlimit + 1;
}

namespace {
// MOM_EINVAL with the reason unless band_start [nBand + 1] runs strictly ascending from 0 to S and 1 + nAer nBand bases fit
int bands_check(mom_t *h, const char *fn, int nAer, int nBand, const int *band_start) {
  char buf[200];
  buf[0] = 0;
  if (nBand < 1) snprintf(buf, sizeof buf, "%s: nBand = %d: a band-resolved scene has at least one band", fn, nBand);
  else if (!band_start) snprintf(buf, sizeof buf, "%s: band_start is NULL", fn);
  else if (nAer >= 0 && 1 + (long long)nAer * nBand > 64)
    snprintf(buf, sizeof buf, "%s: 1 + nAer nBand = 1 + %d x %d phase-matrix bases, at most 64", fn, nAer, nBand);
  else if (band_start[0] != 0) snprintf(buf, sizeof buf, "%s: band_start[0] = %d, not 0", fn, band_start[0]);
  else if (band_start[nBand] != h->S) snprintf(buf, sizeof buf, "%s: band_start[nBand] = %d, not nSpec = %d", fn, band_start[nBand], h->S);
  else
    for (int b = 0; b < nBand && !buf[0]; ++b)
      if (band_start[b + 1] <= band_start[b])
        snprintf(buf, sizeof buf, "%s: band_start is not strictly ascending: band %d is [%d, %d)", fn, b + 1, band_start[b], band_start[b + 1]);
  return buf[0] ? fail(h, MOM_EINVAL, buf) : MOM_OK;
}

// mom_scene_set_optics (nBand = 0: one ϖ_Cabannes, one aerosol set for the whole axis, k_optics) and mom_scene_set_optics_bands
// (nBand >= 1, k_optics_bands): the checks, createAero and the three-way modes per band on the host, the launch, ndoubl / interface
// codes from the per-layer maxima and the tail every scene shares.  tau_aer [nAer, Nz, nB], omega_aer / ft_aer [nAer, nB],
// varpi_rayl [nB], nB = max(nBand, 1).
int scene_set_optics_run(mom_t *h, const char *fn, int Nz, int nAer, int nBand, const int *band_start, int M, const double *tau_rayl,
                         const double *varpi_rayl, const double *tau_aer, const double *omega_aer, const double *ft_aer,
                         const double *Zpp, const double *Zmp, double albedo, int nVza, const int *node_1based, const double *cos_mphi,
                         const double *sin_mphi) {
  const std::string f(fn);
  if (!h->streams_set) return fail(h, MOM_ESTATE, (f + ": call mom_set_streams first").c_str());
  if (Nz <= 0 || nAer < 0 || nAer > 7 || M <= 0 || M > h->M || nVza <= 0 || !tau_rayl || !varpi_rayl || (Zpp == nullptr) != (Zmp == nullptr) ||
      !node_1based || !cos_mphi || !sin_mphi || (nAer > 0 && (!tau_aer || !omega_aer || !ft_aer)))
    return fail(h, MOM_EINVAL, (f + ": bad argument").c_str());
  if (!Zpp) {  // the staged bases (mom_scene_stage_greeks), if any: one per (aerosol type, band) behind Rayleigh's
    const int rc_stage = mom_stage_claim(h, fn, 1 + nAer * std::max(nBand, 1), M);
    if (rc_stage) return rc_stage;
  }
  if (!h->d_tau_abs || h->abs_Nz != Nz)
    return fail(h, MOM_ESTATE, (f + ": no resident tau_abs table of this Nz (mom_absorption_begin / _set)").c_str());
  HIPCHK(h, hipSetDevice(h->device));
  h->scene_set = false;
  h->optics_scene = h->optics_tables = false;
  const size_t S = h->S, AZ = (size_t)nAer * Nz;
  const int nB = std::max(nBand, 1);
  const int K = 1 + nAer * nB;
  const int whole_axis[2] = {0, h->S};
  const int *bs = nBand ? band_start : whole_axis;
  int rc;
  HIPCHK(h, mom_upload(h->d_tau_rayl, tau_rayl, S * Nz, h->stream));
  // the Dual run of this assembly (mom_scene_set_optics_partials / _bands_partials) differentiates createAero on the host as well
  h->optics_nAer = nAer;
  h->optics_nBand = nBand;
  h->h_varpi_rayl.assign(varpi_rayl, varpi_rayl + nB);
  h->h_tau_aer.assign(tau_aer, tau_aer + (nAer > 0 ? AZ * nB : 0));
  h->h_omega_aer.assign(omega_aer, omega_aer + (nAer > 0 ? nAer * nB : 0));
  h->h_ft_aer.assign(ft_aer, ft_aer + (nAer > 0 ? nAer * nB : 0));
  // createAero (compEffectiveLayerProperties.jl:80-85): τ' = (1 - fᵗ ω̃) τ_aer, ϖ' = (1 - fᵗ) ω̃ / (1 - fᵗ ω̃); the
  // all-zero tests of types.jl:641-661 are decided here on the host (they are properties of a band's whole spectral columns)
  std::vector<double> aer((size_t)2 * std::max(nAer, 1) * Nz * nB, 0.0);
  std::vector<int> mode((size_t)std::max(nAer, 1) * Nz * nB, 2);
  for (int b = 0; b < nB; ++b)
    for (int z = 0; z < Nz; ++z) {
      bool x_zero = true;  // all(τ ϖ == 0) of the accumulated left operand
      if (varpi_rayl[b] != 0.0)
        for (size_t n = (size_t)bs[b]; n < (size_t)bs[b + 1]; ++n)
          if (tau_rayl[n + S * z] != 0.0) { x_zero = false; break; }
      for (int x = 0; x < nAer; ++x) {
        const size_t ax = x + (size_t)nAer * z, xb = x + (size_t)nAer * b;
        const double ty = (1 - ft_aer[xb] * omega_aer[xb]) * tau_aer[ax + AZ * b];
        const double vy = (1 - ft_aer[xb]) * omega_aer[xb] / (1 - ft_aer[xb] * omega_aer[xb]);
        const double wy = ty * vy;
        aer[2 * AZ * b + ax] = ty;
        aer[2 * AZ * b + AZ + ax] = wy;
        mode[AZ * b + ax] = x_zero ? 0 : (wy != 0.0 ? 1 : 2);
        x_zero = x_zero && (wy == 0.0);
      }
    }
  HIPCHK(h, mom_upload(h->d_aer, aer.data(), aer.size(), h->stream));
  HIPCHK(h, mom_upload(h->d_aer_mode, mode.data(), mode.size(), h->stream));
  HIPCHK(h, h->d_tau.renew(S * Nz));
  HIPCHK(h, h->d_varpi.renew(S * Nz));
  HIPCHK(h, h->d_zw.renew((size_t)K * S * Nz));
  HIPCHK(h, h->d_tau_sum.renew(S * (Nz + 1)));
  HIPCHK(h, h->d_layer_max.renew((size_t)Nz));
  HIPCHK(h, hipMemsetAsync(h->d_layer_max, 0, (size_t)Nz * sizeof(double), h->stream));
  OpticsArgs a{};
  a.S = h->S; a.Nz = Nz; a.nAer = nAer; a.varpi_rayl = varpi_rayl[0];
  a.tau_rayl = h->d_tau_rayl; a.tau_abs = h->d_tau_abs; a.aer = h->d_aer; a.aer_mode = h->d_aer_mode;
  a.tau = h->d_tau; a.varpi = h->d_varpi; a.zw = h->d_zw; a.tau_sum = h->d_tau_sum; a.layer_max = h->d_layer_max;
  if (nBand) {
    HIPCHK(h, mom_upload(h->d_band_start, band_start, (size_t)nBand + 1, h->stream));
    HIPCHK(h, mom_upload(h->d_varpi_band, varpi_rayl, (size_t)nBand, h->stream));
    a.nBand = nBand; a.band_start = h->d_band_start; a.varpi_band = h->d_varpi_band;
    // a point's weights outside its own band are exact zeros: zeroed here, and the kernel stores the 1 + nAer live ones only
    HIPCHK(h, hipMemsetAsync(h->d_zw, 0, (size_t)K * S * Nz * sizeof(double), h->stream));
    hipLaunchKernelGGL(k_optics_bands, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, a);
  } else {
    hipLaunchKernelGGL(k_optics, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, a);
  }
  HIPCHK(h, hipGetLastError());
  // get_dtau_ndoubl takes maximum(τ .* ϖ) over the WHOLE spectral axis (rt_kernel.jl:241-242): across the ranks of a
  // sharded run the per-layer maxima are combined first (one tiny all-reduce at set-up time, not in the sweep)
  if (h->comm && (rc = mom_comm_allreduce_max(h, h->d_layer_max, (size_t)Nz))) return rc;
  std::vector<double> mx((size_t)Nz);
  HIPCHK(h, hipMemcpyAsync(mx.data(), h->d_layer_max, (size_t)Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double mu_min = h->h_mu[0];
  for (double v : h->h_mu) mu_min = std::min(mu_min, v);
  h->nd.assign((size_t)Nz, 0);
  h->iface.assign((size_t)Nz, 0);
  int prev = 0;
  for (int z = 0; z < Nz; ++z) {
    if (!std::isfinite(mx[z])) return fail(h, MOM_EINVAL, (f + ": a layer has non-finite τ ϖ (empty layer: τ = 0?)").c_str());
    h->nd[z] = doubling_number_host(std::min(mx[z], 0.001 * mu_min), mx[z]);
    if (h->nd[z] > 60) return fail(h, MOM_EINVAL, (f + ": ndoubl out of range").c_str());
    const bool scatter = mx[z] > 2 * 2.220446049250313e-16;  // compEffectiveLayerProperties.jl:104
    prev = (z == 0) ? (scatter ? 3 : 0) : (prev == 0 ? (scatter ? 1 : 0) : (scatter ? 3 : 2));  // rt_helper_functions.jl:8-27
    h->iface[z] = prev;
  }
  if (h->f32) {  // Float32 handle: the Float64 assembly above is rounded to Float32 on the device (no host hop of tau_abs either)
    h->Nz = Nz; h->K = K; h->scene_M = M; h->nVza = nVza; h->albedo = albedo; h->surf_kind = 0;
    if ((rc = momf_scene_set_dev(h->f32, Nz, K, M, h->d_tau, h->d_varpi, h->d_zw, Zpp, Zmp, h->nd.data(), h->iface.data(), h->d_tau_sum,
                                 albedo, nVza, node_1based, cos_mphi, sin_mphi)))
      return fail(h, rc, momf_error(h->f32));
    h->scene_set = true;
    return MOM_OK;
  }
  if ((rc = scene_common(h, Nz, K, M, Zpp, Zmp, albedo, nVza, node_1based, cos_mphi, sin_mphi))) return rc;
  h->scene_set = true;
  h->optics_scene = h->optics_tables = true;
  return MOM_OK;
}
}  // namespace

extern "C" int mom_scene_set_optics(mom_t *h, int Nz, int nAer, int M, const double *tau_rayl, double varpi_rayl,
                                    const double *tau_aer, const double *omega_aer, const double *ft_aer,
                                    const double *Zpp, const double *Zmp, double albedo, int nVza, const int *node_1based,
                                    const double *cos_mphi, const double *sin_mphi) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  return scene_set_optics_run(h, "mom_scene_set_optics", Nz, nAer, 0, nullptr, M, tau_rayl, &varpi_rayl, tau_aer, omega_aer, ft_aer, Zpp,
                              Zmp, albedo, nVza, node_1based, cos_mphi, sin_mphi);
}

extern "C" int mom_scene_set_optics_bands(mom_t *h, int Nz, int nAer, int nBand, const int *band_start, int M, const double *tau_rayl,
                                          const double *varpi_rayl, const double *tau_aer, const double *omega_aer,
                                          const double *ft_aer, const double *Zpp, const double *Zmp, double albedo, int nVza,
                                          const int *node_1based, const double *cos_mphi, const double *sin_mphi) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  const char *fn = "mom_scene_set_optics_bands";
  const int rc = bands_check(h, fn, nAer, nBand, band_start);
  if (rc) return rc;
  if (h->comm)
    return fail(h, MOM_EUNSUPPORTED, "mom_scene_set_optics_bands: the handle has a communicator: the per-band all-zero tests of the `+` "
                                     "(types.jl:641-661) would need a reduction over the ranks; a sharded band-resolved run takes the host "
                                     "route (mom_scene_set)");
  return scene_set_optics_run(h, fn, Nz, nAer, nBand, band_start, M, tau_rayl, varpi_rayl, tau_aer, omega_aer, ft_aer, Zpp, Zmp, albedo,
                              nVza, node_1based, cos_mphi, sin_mphi);
}

extern "C" int mom_scene_get_layers(mom_t *h, int *ndoubl, int *iface, double *tau, double *varpi, double *zw, double *tau_sum) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set) return fail(h, MOM_ESTATE, "mom_scene_get_layers: no scene");
  if (h->f32 && (tau || varpi || zw || tau_sum) && !h->d_tau)
    return fail(h, MOM_ESTATE, "mom_scene_get_layers: a Float32 handle keeps the Float64 layer arrays only after mom_scene_set_optics");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = h->S, Nz = h->Nz;
  if (ndoubl) std::copy(h->nd.begin(), h->nd.end(), ndoubl);
  if (iface) std::copy(h->iface.begin(), h->iface.end(), iface);
  if (tau) HIPCHK(h, hipMemcpyAsync(tau, h->d_tau, S * Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (varpi) HIPCHK(h, hipMemcpyAsync(varpi, h->d_varpi, S * Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (zw) HIPCHK(h, hipMemcpyAsync(zw, h->d_zw, (size_t)h->K * S * Nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (tau_sum) HIPCHK(h, hipMemcpyAsync(tau_sum, h->d_tau_sum, S * (Nz + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}

// ---- The Dual run of k_optics: the partials of τ, ϖ and the basis weights with respect to P parameters, formed from the partials
// of the ingredients -- constructCoreOpticalProperties / createAero (compEffectiveLayerProperties.jl:1-85) and the `+` of
// types.jl:632-678 on ForwardDiff.Dual element types.  It follows k_optics statement by statement with ForwardDiff's rules:
// d(a b) = da b + db a, d(a / b) = da (1 / b) + db (-(a / b²)).  The three aerosol modes are the value run's (d_aer_mode): ForwardDiff
// takes `all(τϖ .== 0)` on the values.  One thread per (spectral point, layer, partial), the spectral index fastest across lanes:
// every load and store of an [S, ...] array is contiguous across a wavefront (dzw [K, S, ...] in runs of K doubles per lane, K stores
// that together cover the same contiguous range); the per-(layer, partial) scalars are uniform across a workgroup (blockIdx.y, .z).
// Unlike k_optics nothing here runs along the layers (dτ_sum is not formed: k_dtausum of the Dual sweep derives it from dτ), so the
// layers are grid blocks, not a loop: at S = 10⁴ a thread per (point, partial) would be 469 wavefronts for 1024 SIMDs, each waiting
// for its loads layer after layer.  The cheap value chain is recomputed per partial.
// Contraction stays off as for k_optics: the statements round as the host twin's (absorption.optics_partials_host) do.
struct OpticsDualArgs {
  int S, Nz, nAer;
  double varpi_rayl;
  const double *tau_rayl, *tau_abs;  // [S,Nz]
  const double *dtau_abs;            // [S,Nz,2] or null (no Dual absorption call: zeros)
  const double *aer;                 // [2,nAer,Nz] as in OpticsArgs
  const int *aer_mode;               // [nAer,Nz]
  const double *w_abs, *w_rayl;      // [Nz,3,P], [Nz,P]: chain weights onto dtau_abs[.., 0], dtau_abs[.., 1], tau_abs; onto tau_rayl
  const double *daer;                // [2,nAer,Nz,P]: partials of aer
  double *dtau, *dvarpi;             // [S,Nz,P]
  double *dzw;                       // [K,S,Nz,P] or null (identically zero: not stored)
  // k_optics_bands_dual only: aer, aer_mode one block per band as in OpticsArgs, daer [2,nAer,Nz,nBand,P]
  int nBand;
  const int *band_start;             // [nBand + 1]
  const double *varpi_band;          // [nBand]
};
__device__ __forceinline__ void dual_div(double a, double da, double b, double db, double &q, double &dq) {
  q = a / b;
  dq = da * (1.0 / b) + db * (-(a / (b * b)));
}
// One (spectral point, layer, partial): stores dτ and dϖ and leaves the partials dw of the 1 + nAer weights of the point's own bases;
// `aer` / `mode` are the value blocks of the point's band, `daer` the [2,nAer,Nz] partial block of (band, partial).
__device__ __forceinline__ void optics_point_dual(const OpticsDualArgs &a, int n, int z, int p, double varpi_rayl, const double *aer,
                                                  const int *aer_mode, const double *daer, double (&dw)[8]) {
  const size_t SZ = (size_t)a.S * a.Nz, AZ = (size_t)a.nAer * a.Nz;
  const size_t o = n + (size_t)a.S * z, op = o + SZ * p;
  double tau = a.tau_rayl[o], varpi = varpi_rayl;
  double dtau = tau * a.w_rayl[z + (size_t)a.Nz * p], dvarpi = 0.0;
  double w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { w[k] = k == 0 ? 1.0 : 0.0; dw[k] = 0.0; }
  for (int x = 0; x < a.nAer; ++x) {
    const size_t ax = x + (size_t)a.nAer * z;
    const double ty = aer[ax], wy = aer[AZ + ax];
    const double dty = daer[ax], dwy = daer[AZ + ax];
    const int mode = aer_mode[ax];
    const double wx = tau * varpi, dwx = dtau * varpi + dvarpi * tau;
    const double tot = wx + wy, dtot = dwx + dwy, tn = tau + ty, dtn = dtau + dty;
    if (mode == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { w[k] = k == x + 1 ? 1.0 : 0.0; dw[k] = 0.0; }
    } else if (mode == 1) {
      double fx, dfx, fy, dfy;
      dual_div(wx, dwx, tot, dtot, fx, dfx);
      dual_div(wy, dwy, tot, dtot, fy, dfy);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double dk = dw[k] * fx + dfx * w[k];
        dw[k] = k == x + 1 ? dfy : dk;
        w[k] = k == x + 1 ? fy : w[k] * fx;
      }
    }
    dual_div(tot, dtot, tn, dtn, varpi, dvarpi);
    tau = tn;
    dtau = dtn;
  }
  const double ta = a.tau_abs[o];
  const double *wa = a.w_abs + z + (size_t)a.Nz * 3 * p;
  double dta = ta * wa[2 * a.Nz];
  if (a.dtau_abs) dta = a.dtau_abs[o] * wa[0] + a.dtau_abs[o + SZ] * wa[a.Nz] + dta;
  const double tn = tau + ta, dtn = dtau + dta;
  const double num = tau * varpi, dnum = dtau * varpi + dvarpi * tau;
  dual_div(num, dnum, tn, dtn, varpi, dvarpi);
  a.dtau[op] = dtn;
  a.dvarpi[op] = dvarpi;
}
__global__ void __launch_bounds__(256) k_optics_dual(OpticsDualArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y, p = blockIdx.z;
  if (n >= a.S) return;
  const int K = 1 + a.nAer;
  const size_t AZ = (size_t)a.nAer * a.Nz, op = n + (size_t)a.S * z + (size_t)a.S * a.Nz * p;
  double dw[8];
  optics_point_dual(a, n, z, p, a.varpi_rayl, a.aer, a.aer_mode, a.daer + 2 * AZ * p, dw);
  if (a.dzw) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < K) a.dzw[k + (size_t)K * op] = dw[k];
  }
}
// k_optics_dual for a band-resolved scene, as k_optics_bands is k_optics': the same grid, the band found once per thread, that
// band's ϖ_Cabannes, value blocks and partial block (a partial that names one band's aerosol has zero blocks in the others, so the
// other bands' points see the Rayleigh and gas partials only).  dzw [K,S,Nz,P], K = 1 + nAer nBand, is zeroed by the host and a thread
// stores the 1 + nAer entries of its own band.
__global__ void __launch_bounds__(256) k_optics_bands_dual(OpticsDualArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y, p = blockIdx.z;
  if (n >= a.S) return;
  const int K = 1 + a.nAer * a.nBand;
  const int b = optics_band(n, a.nBand, a.band_start);
  const size_t AZ = (size_t)a.nAer * a.Nz, op = n + (size_t)a.S * z + (size_t)a.S * a.Nz * p;
  double dw[8];
  optics_point_dual(a, n, z, p, a.varpi_band[b], a.aer + 2 * AZ * b, a.aer_mode + AZ * b, a.daer + 2 * AZ * (b + (size_t)a.nBand * p), dw);
  if (a.dzw) {
    double *dzw = a.dzw + (size_t)K * op;
    dzw[0] = dw[0];
#pragma unroll
    for (int x = 0; x < 7; ++x)
      if (x < a.nAer) dzw[1 + x + a.nAer * b] = dw[x + 1];
  }
}

// createAero (compEffectiveLayerProperties.jl:80-85) on Duals for one aerosol type and layer: τ_y = (1 - fᵗ ω̃) τ_aer,
// ϖ_y = (1 - fᵗ) ω̃ / (1 - fᵗ ω̃), w_y = τ_y ϖ_y -> the partials of τ_y and w_y
static void create_aero_dual(double tau_aer, double om, double ft, double dtau_aer, double dom, double dft, double *dty, double *dwy) {
  const double fo = ft * om, dfo = dft * om + dom * ft;
  const double b = 1 - fo, db = -dfo;
  const double ty = b * tau_aer;
  *dty = db * tau_aer + dtau_aer * b;
  const double c = 1 - ft, dc = -dft;
  const double num = c * om, dnum = dc * om + dom * c;
  const double vy = num / b, dvy = dnum * (1.0 / b) + db * (-(num / (b * b)));
  *dwy = *dty * vy + dvy * ty;
}

namespace {
// mom_scene_set_optics_partials (banded = false, k_optics_dual) and mom_scene_set_optics_bands_partials (k_optics_bands_dual): the
// state rules, createAero on Duals per (band, layer, type, partial), the launch and mom_partials_rest.  dtau_aer [nAer, Nz, nB, P],
// domega_aer / dft_aer [nAer, nB, P], nB = the scene's bands (1 without).
int scene_set_optics_partials_run(mom_t *h, const char *fn, bool banded, int P, const double *w_abs, const double *w_rayl,
                                  const double *dtau_aer, const double *domega_aer, const double *dft_aer, const double *dZpp,
                                  const double *dZmp, const double *dalbedo, const double *dRsurf, const double *dalbedo_spec) {
  const std::string f(fn), setter = banded ? "mom_scene_set_optics_bands" : "mom_scene_set_optics";
  if (!h->scene_set) return fail(h, MOM_ESTATE, (f + ": call " + setter + " first").c_str());
  if (!h->optics_scene)
    return fail(h, MOM_ESTATE, (f + ": the resident scene came from mom_scene_set (host optics): its partials go through "
                                    "mom_scene_set_partials").c_str());
  if (banded != (h->optics_nBand != 0))
    return fail(h, MOM_ESTATE, (f + ": the resident scene came from " + (banded ? "mom_scene_set_optics (no bands): its partials go through "
                                    "mom_scene_set_optics_partials" : "mom_scene_set_optics_bands: its partials go through "
                                    "mom_scene_set_optics_bands_partials")).c_str());
  if (!h->optics_tables || !h->d_tau_abs || h->abs_Nz != h->Nz)
    return fail(h, MOM_ESTATE, (f + ": mom_absorption_begin / _set was called after the " + setter + " that made the scene: the resident "
                                    "tau_abs table is not the scene's").c_str());
  int rc = mom_partials_check(h, fn, P, dZpp, dZmp);
  if (rc) return rc;
  const int Nz = h->Nz, nAer = h->optics_nAer, K = h->K, nB = std::max(h->optics_nBand, 1);
  if (w_abs && !h->d_dtau_abs)
    for (size_t k = 0; k < (size_t)P; ++k)
      for (size_t i = 0; i < 2 * (size_t)Nz; ++i)
        if (w_abs[i + 3 * (size_t)Nz * k] != 0.0)
          return fail(h, MOM_ESTATE, (f + ": w_abs has a nonzero pressure or temperature weight, but no dtau_abs table is resident (no "
                                          "Dual absorption call since the table was set)").c_str());
  HIPCHK(h, hipSetDevice(h->device));
  mom_partials_reset(h, P);
  if (P == 0) return MOM_OK;
  const size_t S = h->S, SZ = S * Nz, AZ = (size_t)nAer * Nz;
  // per-(layer, partial) scalars: w_abs [Nz,3,P] | w_rayl [Nz,P] | d aer [2,nAer,Nz,nB,P]; a null argument: zeros
  const size_t n_abs = 3 * (size_t)Nz * P, n_rayl = (size_t)Nz * P, n_aer = 2 * AZ * nB * P;
  std::vector<double> prm(n_abs + n_rayl + n_aer, 0.0);
  if (w_abs) std::copy(w_abs, w_abs + n_abs, prm.begin());
  if (w_rayl) std::copy(w_rayl, w_rayl + n_rayl, prm.begin() + n_abs);
  if (nAer > 0 && (dtau_aer || domega_aer || dft_aer)) {
    double *da = prm.data() + n_abs + n_rayl;
    for (size_t k = 0; k < (size_t)P; ++k)
      for (int b = 0; b < nB; ++b)
        for (int z = 0; z < Nz; ++z)
          for (int x = 0; x < nAer; ++x) {
            const size_t ax = x + (size_t)nAer * z, xb = x + (size_t)nAer * b, blk = 2 * AZ * (b + (size_t)nB * k);
            create_aero_dual(h->h_tau_aer[ax + AZ * b], h->h_omega_aer[xb], h->h_ft_aer[xb],
                             dtau_aer ? dtau_aer[ax + AZ * (b + (size_t)nB * k)] : 0.0,
                             domega_aer ? domega_aer[xb + (size_t)nAer * nB * k] : 0.0, dft_aer ? dft_aer[xb + (size_t)nAer * nB * k] : 0.0,
                             &da[blk + ax], &da[blk + AZ + ax]);
          }
  }
  HIPCHK(h, h->d_optics_prm.reserve(prm.size(), h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_optics_prm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->d_dual_in[0].renew(SZ * P));
  HIPCHK(h, h->d_dual_in[1].renew(SZ * P));
  // the weights depend on the Rayleigh and aerosol ingredients only: without a partial of those dzw stays absent and the sweep skips it
  if (nAer > 0 && (w_rayl || dtau_aer || domega_aer || dft_aer)) {
    HIPCHK(h, h->d_dual_in[2].renew((size_t)K * SZ * P));
    // band-resolved: the entries outside a point's own band are exact zeros, and k_optics_bands_dual stores the live ones only
    if (banded) HIPCHK(h, hipMemsetAsync(h->d_dual_in[2], 0, (size_t)K * SZ * P * sizeof(double), h->stream));
  }
  OpticsDualArgs a{};
  a.S = h->S; a.Nz = Nz; a.nAer = nAer;
  a.varpi_rayl = h->h_varpi_rayl[0];
  a.tau_rayl = h->d_tau_rayl; a.tau_abs = h->d_tau_abs; a.dtau_abs = h->d_dtau_abs; a.aer = h->d_aer; a.aer_mode = h->d_aer_mode;
  a.w_abs = h->d_optics_prm; a.w_rayl = h->d_optics_prm + n_abs; a.daer = h->d_optics_prm + n_abs + n_rayl;
  a.dtau = h->d_dual_in[0]; a.dvarpi = h->d_dual_in[1]; a.dzw = h->d_dual_in[2];
  a.nBand = h->optics_nBand; a.band_start = h->d_band_start; a.varpi_band = h->d_varpi_band;
  // the launch between the handle's timing events: mom_timers right after this call gives the kernel's time as its total
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)Nz, (unsigned)P);
  if (banded) hipLaunchKernelGGL(k_optics_bands_dual, grid, dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL(k_optics_dual, grid, dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  for (int k = 1; k < 4; ++k) HIPCHK(h, hipEventRecord(h->ev[k], h->stream));
  h->launches = 1; h->launches_full = 0; h->launches_red = 0;
  HIPCHK(h, hipStreamSynchronize(h->stream));  // prm is a host temporary
  return mom_partials_rest(h, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec);
}
}  // namespace

extern "C" int mom_scene_set_optics_partials(mom_t *h, int P, const double *w_abs, const double *w_rayl, const double *dtau_aer,
                                             const double *domega_aer, const double *dft_aer, const double *dZpp, const double *dZmp,
                                             const double *dalbedo, const double *dRsurf, const double *dalbedo_spec) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_scene_set_optics_partials");
  return scene_set_optics_partials_run(h, "mom_scene_set_optics_partials", false, P, w_abs, w_rayl, dtau_aer, domega_aer, dft_aer, dZpp,
                                       dZmp, dalbedo, dRsurf, dalbedo_spec);
}

extern "C" int mom_scene_set_optics_bands_partials(mom_t *h, int P, const double *w_abs, const double *w_rayl, const double *dtau_aer,
                                                   const double *domega_aer, const double *dft_aer, const double *dZpp,
                                                   const double *dZmp, const double *dalbedo, const double *dRsurf,
                                                   const double *dalbedo_spec) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_scene_set_optics_bands_partials");
  return scene_set_optics_partials_run(h, "mom_scene_set_optics_bands_partials", true, P, w_abs, w_rayl, dtau_aer, domega_aer, dft_aer,
                                       dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec);
}

extern "C" int mom_scene_get_partials(mom_t *h, double *dtau, double *dvarpi, double *dzw) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->scene_set || h->dual_P == 0)
    return fail(h, MOM_ESTATE, "mom_scene_get_partials: no partials resident (mom_scene_set_partials / mom_scene_set_optics_partials with P > 0)");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t SZP = (size_t)h->S * h->Nz * h->dual_P;
  double *dst[3] = {dtau, dvarpi, dzw};
  const size_t cnt[3] = {SZP, SZP, (size_t)h->K * SZP};
  for (int k = 0; k < 3; ++k) {
    if (!dst[k]) continue;
    if (h->d_dual_in[k]) HIPCHK(h, hipMemcpyAsync(dst[k], h->d_dual_in[k], cnt[k] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    else std::fill(dst[k], dst[k] + cnt[k], 0.0);   // an absent buffer: no dependence
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MOM_OK;
}
