// mom_handle.hpp -- the handle behind mom_t and what more than one unit of the host driver needs of it (momcore.hip,
// mom_scene.hip, mom_optics.hip, mom_rrs_api.hip, mom_comm.hip).  Float64 driver only: include it with the default MOM_NS.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "momcore.h"

#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_host.hpp"

namespace momr { struct State; }  // mom_rrs.hpp

// One InterpolationModel of the handle (mom_lut.hip): sigma on a (nu, p, T) grid of ranges, axis 0 = nu, 1 = p, 2 = T
struct MomLut {
  bool live = false;                // the id is handed out
  int n[3] = {};                    // nodes per axis
  double first[3] = {}, step[3] = {};
  bool has_table = false, has_coef = false;
  MomDevBuf<double> d_table;        // sigma [nNu, nP, nT], nu fastest (the reference's cs_matrix)
  MomDevBuf<double> d_coef;         // the padded cubic B-spline coefficients [nNu + 2, nP + 2, nT + 2]
  MomDevBuf<double> d_nu;           // the model's nu grid [nNu] (mom_lut_build's spectral grid)
};

// Greek sets [nG][6][l_pad] (rows α, β, γ, δ, ϵ, ζ; mom_z_moments' layout) waiting for a setter.  Derivative sets: set d is the
// partial of basis `basis[d]` with respect to parameter `partial[d]` of P
struct MomGreekStage {
  bool live = false;
  int nG = 0, l_pad = 0, M = 0, P = 0;
  std::vector<int> l_max, basis, partial;
  std::vector<double> greek;
  void drop() { *this = MomGreekStage{}; }
};

// The resident scene's arrays and counts (d_mu ... d_scratch, Nz, K, nVza, scene_M, surf_kind, albedo, nd, iface) are the base:
// MomSceneBufs, mom_host.hpp -- the declaration the Float32 scene shares
struct mom_handle : MomSceneBufs<double> {
  int device = 0, N = 0, nS = 0, S = 0, M = 0;
  int dtype = 0;              // 0 = Float64, 1 = Float32 (scene-level path only, momcore_f32.hip)
  momf_scene *f32 = nullptr;
  bool lds_mode = true;
  int opt_inverse = 0, opt_force_generic = 0;
  hipStream_t stream = nullptr;
  mom::DevStreams q{};
  bool streams_set = false;
  std::vector<double> h_mu, h_wt;
  int strict = 1;
  MomDevBuf<double> added[6], surf[6], comp[6];
  bool op_layers = false;     // added / surface layers of the operator-level API: allocated on first use
  bool comp_pitched = false;  // composite matrix blocks hold scene-level (row-pitched) state
  bool comp_on_chip = false;  // the last mom_rt_run kept the composite layer in registers (lane / wave kernels)
  MomDevBuf<double> d_post;   // operator-level mom_postprocess: gathered J0- | J0+ rows [2][nVza*nS*S]
  // RCCL communicator (mom_comm_init); the library is dlopen'ed on first use
  void *comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  MomDevBuf<double> d_gather;
  MomDevBuf<double> d_rrs_send;  // packed owned spectra of the RRS run: send buffer of mom_allgather_rrs_device
  // device-side layer optics (mom_absorption_* / mom_voigt_tau_abs / mom_scene_set_optics)
  MomDevBuf<double> d_tau_abs, d_grid, d_lines, d_tau_rayl, d_layer_max, d_aer;
  MomDevBuf<int> d_aer_mode;
  int abs_Nz = 0;
  size_t lines_per = 0;   // d_lines is a MomLineBlock (mom_host.hpp, which owns the format) of this capacity per layer ...
  int lines_nz = 1;       // ... and this many layers, as the last absorption call left it (line_blocks, mom_optics.hip)
  int abs_broadening = 0, abs_cef = 0;  // mom_absorption_set_model: MOM_BROADENING_*, MOM_CEF_* of the absorption calls (Voigt / HW32SD)
  MomDevBuf<double> d_prof;  // per-layer scalars of mom_voigt_tau_abs_profile
  // Dual run of the absorption path (mom_voigt_tau_abs_dual / _profile_dual): partials with respect to (p, T) of every layer
  MomDevBuf<double> d_dtau_abs;  // [S, abs_Nz, 2]; exists from the first Dual call after mom_absorption_begin
  MomDevBuf<double> d_dlines;    // partials of d_lines' prefactors: the MomLinePartialBlock of the same (lines_per, lines_nz); grow-only
  // Dual run of the layer optics (mom_scene_set_optics_partials): what mom_scene_set_optics keeps of its scene for it
  bool optics_scene = false;     // the resident scene came from mom_scene_set_optics (mom_scene_set clears it) ...
  bool optics_tables = false;    // ... and d_tau_abs / d_dtau_abs are still the tables it read (mom_absorption_begin / _set clear it)
  int optics_nAer = 0;
  int optics_nBand = 0;          // 0: the scene came from mom_scene_set_optics; >= 1: from mom_scene_set_optics_bands, this many bands
  std::vector<double> h_varpi_rayl;                      // host copy of ϖ_Cabannes, one per band (one entry without bands)
  std::vector<double> h_tau_aer, h_omega_aer, h_ft_aer;  // host copies of its aerosol arguments [nAer, Nz(, nBand)], [nAer(, nBand)] twice
  MomDevBuf<int> d_band_start;     // [nBand + 1] offsets of the bands on the spectral axis (k_optics_bands, k_optics_bands_dual)
  MomDevBuf<double> d_varpi_band;  // [nBand] ϖ_Cabannes per band
  MomDevBuf<double> d_optics_prm;  // per-(layer, partial) scalars of k_optics_dual (OpticsDualArgs::w_abs | w_rayl | daer); grow-only
  MomDevBuf<double> d_vec[4];  // S-length temporaries (tau_sum, dtau, varpi, expk)
  MomDevBuf<double> d_Zop[2];
  // scene
  bool scene_set = false;
  // Greek coefficients staged for the next setter (mom_scene_stage_greeks / _greek_partials): host copies, no device memory.  The
  // setter that takes a stage forms the Z bases in the handle's own buffers (mom_zmom.hip) and the stage is gone
  MomGreekStage stage_z, stage_r, stage_d;  // the elastic bases, the Raman set, the derivative sets
  // m = 0 reduction (see mom_scene_set)
  int opt_m0 = 1;
  int opt_w4 = 1;
  int opt_stagger = 1;
  int opt_rrs_kernels = -1;  // MOM_OPT_RRS_KERNELS (-1: momr::KOPT_DEFAULT)
  int opt_overlap = 1;       // MOM_OPT_OVERLAP: the m = 0 sub-problem on a second (high-priority) stream of the handle
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_go = nullptr;
  // ForwardDiff.Dual run (mom_dual.hip): partials of the scene's inputs and of the outputs, the operator workspace
  int dual_P = 0;
  bool dual_ran = false;
  MomDevBuf<double> d_dual_in[8];  // dtau, dvarpi, dzw, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec
  MomDevBuf<double> d_dual_out, d_dual_ts;  // dR | dT [nVza,nS,S,P] x 2; d tau_sum [S,Nz+1,P]
  MomDevBuf<char> dual_work;
  size_t opt_dual_budget = 0;  // MOM_OPT_DUAL_WORKSPACE_MB (0: 60 % of the free HBM at the time of the run)
  MomDevBuf<double> d_Rsurf0;
  int opt_sweep = 1;       // one launch walks all layers of a unit (LayerArgs::Nz_sweep)
  MomDevBuf<double> comp_top[6];  // mom_rt_run_multisensor: composite state of the slab above a sensor
  MomDevBuf<double> d_msJ[2];     // interface fields dwJ, uwJ [Nk,S,M]
  std::vector<MomDevBuf<double>> ms_comp;  // multi-sensor: 6 arrays per composite set (snapshot of the top slab + bottom slab per sensor)
  MomDevBuf<double> d_ms_out;  // [2][nVza*nS*S*nSensors]
  int opt_pad = 1;         // scene-level path: pad the operator edge to the next strip-chained kernel size (strip_pad)
  int opt_lean = 3;        // N = 36, 40: 3 = the quad-block image (one wavefront per unit, 4 x 4 x 4 MFMA blocks, four units per CU;
                           // mom_q4.hpp), 1 = the four-wave lean strip image (three workgroups per CU), 2 = the six-wave one (half-strip
                           // doubling chains, two per CU: measured slower, profiles/r05_mid_ab.txt), each followed by the full image's
                           // resume launch; 0 = the full image only
  MomDevBuf<int> d_resume; // resume[unit] of the lean image (mom_lean.hpp)
  int opt_strip2 = 1;       // MOM_OPT_STRIP2: N = 52, 56, 60 on the two-buffer 4-wave image first (mom_strip2.hpp), the 8-wave image resumes
  MomDevBuf<int> d_resume2; // its resume[unit] (a table of its own: the m = 0 sub-problem's lean launch may run at the same time)
  size_t resume2_units = 0;  // units and layers of the image's last launch (mom_strip2_resumed)
  int resume2_nz = 0;
  int opt_strip2_sched = 1;  // MOM_OPT_STRIP2_SCHED: bit 0 = shared unit queue, bit 1 = asymmetric chain priority (mom_strip2.hpp; one
                             // kernel per value); the priority measured slower on top of the queue (profiles/r08_C2_ab.txt): off
  MomDevBuf<int> d_sched2;   // LayerArgs::sched of the two-buffer image: zeroed on the stream before each of its launches
  int opt_zero_skip = 7;     // MOM_OPT_ZERO_SKIP, a mask: the exact-zero products of the zero-weight trailing streams are left out by
                             // 1 the quad-block image (blocks), 2 the two-buffer strip image (k-steps of its strip products);
                             // 4 the two-buffer strip image multiplies only the live blocks of four rows of a partly live row tile
  int opt_sources_only = 1;  // MOM_OPT_SOURCES_ONLY: mom_rt_run's launches without an observable moment (the (I,Q) sub-problem's, a
                             // full-problem launch from moment 1 on) leave the composite R-+ and T++ out (two-buffer strip and
                             // quad-block images; MomLaunchForm::sources_only)
  int opt_elemental = 1;     // MOM_OPT_ELEMENTAL: the two-buffer strip image (default scheduling mode) and the quad-block image build
                             // the elemental layer in its table form (mom_elemental_tab.hpp; MomLaunchForm::elemental_tab,
                             // the tables below in LayerArgs::etab); 0 = elemental_build everywhere
  MomDevBuf<double> d_etab, d_etab0;  // stream-pair tables SI | F1 | F2, [3][Nq][Nq], of the full problem's streams (qk) and of the
                                      // (I,Q) sub-problem's (q0): built by scene_common where the table form can apply, else empty
  int nbw_0 = 0;             // blocks of four entries with a weighted one (mom_q4_nbw) of the m = 0 sub-problem, after reduction and padding
  int Nk = 0;              // operator edge the scene-level kernels of the full problem run with (>= N)
  mom::DevStreams qk{};         // q with N = Nk
  int opt_small = 1;       // N <= 4: lane-per-point sweep kernel (mom_small.hip)
  bool red0 = false;
  int N0 = 0, nS0 = 0;
  mom::DevStreams q0{};
  MomDevBuf<double> d_mu0, d_wt0, d_sg0, d_Zpp0, d_Zmp0, d_hdrJ0, d_scratch0;
  MomDevBuf<double> comp0[6];
  int G = 0;  // workgroups in generic mode
  int num_cu = 256;
  MomDevBuf<int> d_info;
  hipEvent_t ev[4] = {};
  hipEvent_t ev_voigt[2] = {};  // mom_voigt_tau_abs_profile's timing pair (created on first use, owned by the handle)
  std::vector<hipEvent_t> ev_full, ev_red;  // start/stop pairs around each full-problem / reduced layer launch
  int launches = 0, launches_full = 0, launches_red = 0;
  // rotational-Raman path (mom_rrs.hip): the persistent AddedLayerRS / CompositeLayerRS state and the scene's Raman inputs
  momr::State *rrs = nullptr;
  MomDevBuf<double> d_fscatt, d_Zr[2];  // fScattRayleigh [S,Nz]; Raman phase matrices [N,N,M] x2
  MomDevBuf<double> d_rrs_op[8];        // operator-level inputs: tau_sum, dtau, varpi, fscatt [S]; Z x4 [N,N]
  bool rrs_scene = false;
  double rrs_ms = 0.0;
  // grow-only device workspace of the operator-level batched entry points (no allocation per call, no leak on an error
  // return): bytes, viewed as the element type each call needs
  MomDevBuf<char> ws[4];
  // resident HITRAN table + TIPS splines of one absorber (mom_absorption_set_lines)
  MomLineTable lt{};
  MomDevBuf<double> d_lt;   // one allocation behind lt's double arrays
  MomDevBuf<int> d_lt_i;    // iso index [nLines] | knots per isotopologue [nIso] | unsorted flag [1]
  double lt_Tmin = 0.0, lt_Tmax = 0.0;
  // InterpolationModels (mom_lut_*): the id of a table is its index here; a destroyed slot is handed out again
  std::vector<MomLut> luts;
  MomDevBuf<double> d_lut_cp;    // the Thomas factors of the prefilter
  MomDevBuf<double> d_lut_prm;   // per-layer weight blocks of an evaluation
  MomDevBuf<double> d_lut_io;    // mom_lut_xsec: nu | sigma | J
  int opt_lut_batch = 0;         // MOM_OPT_LUT_BATCH: (p, T) nodes per batch of mom_lut_build (0: 64)
  // the spectral grid as mom_absorption_begin saw it: smallest and largest value, 1 ascending / -1 descending / 0 neither
  double grid_min = 0.0, grid_max = 0.0;
  int grid_order = 0;
  std::string err;
};

// what the units share besides the handle; internal to libmomcore.so, not part of the C ABI
#pragma GCC visibility push(hidden)
int fail(mom_t *h, int code, const char *msg);  // momcore.hip: error text -> the handle (if any) and the thread's string; returns code
int check_info(mom_t *h);                       // momcore.hip: the zero-pivot report of the handle's kernels (synchronises)
// what an absorption entry point `fn` needs before it may run: the resident tau_abs table and grid (`table`), the resident line
// table (`lines`); MOM_ESTATE with the call that is missing
inline int mom_absorption_state(mom_t *h, const char *fn, bool table, bool lines) {
  const bool no_table = table && (!h->d_tau_abs || !h->d_grid);
  if (!no_table && !(lines && !h->d_lt)) return MOM_OK;
  char buf[200];
  snprintf(buf, sizeof buf, no_table ? "%s: call mom_absorption_begin with the spectral grid first" : "%s: call mom_absorption_set_lines first", fn);
  return fail(h, MOM_ESTATE, buf);
}
// qoft! asserts Tmin < T < Tmax (compute_absorption_cross_section.jl:204): T against the common range of the resident TIPS tables
inline int mom_tips_range(mom_t *h, double T) {
  if (h->lt.nIso <= 0 || (h->lt_Tmin < T && T < h->lt_Tmax)) return MOM_OK;
  char buf[160];
  snprintf(buf, sizeof buf, "TIPS2017: T (%g) must be between %g K and %g K.", T, h->lt_Tmin, h->lt_Tmax);
  return fail(h, MOM_EINVAL, buf);
}
// momcore.hip: one launch of k_combine<lds> for mom_rt_run_multisensor (why not from mom_scene.hip: see its definition)
hipError_t mom_launch_combine(const mom::InterArgs &a, bool lds, int grid, size_t smem, hipStream_t st);
// mom_scene.hip: everything of a scene that does not depend on how the layer optics reach the device: phase-matrix bases, view
// geometry, output buffers, the m = 0 reduction
int scene_common(mom_t *h, int Nz, int K, int M, const double *Zpp, const double *Zmp, double albedo, int nVza,
                 const int *node_1based, const double *cos_mphi, const double *sin_mphi);
// mom_scene.hip: a setter `fn` of K bases and M moments was given Zpp == Zmp == NULL.  MOM_OK when staged Greek sets of that shape
// wait (scene_common takes them when its Zpp is null); MOM_EINVAL otherwise: without a stage the setter's "bad argument", with one
// of another shape a text that names both
int mom_stage_claim(mom_t *h, const char *fn, int K, int M);
// mom_comm.hip: set once RCCL is loaded (mom_comm_init); the maximum over the ranks of `count` doubles on the device, in place
extern void (*g_rccl_destroy)(void *);
int mom_comm_allreduce_max(mom_t *h, double *d_buf, size_t count);
#pragma GCC visibility pop

#define HIPCHK(h, call)                                                                            \
  do {                                                                                             \
    hipError_t e__ = (call);                                                                       \
    if (e__ != hipSuccess) {                                                                       \
      char buf__[512];                                                                             \
      snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      return fail(h, MOM_EHIP, buf__);                                                             \
    }                                                                                              \
  } while (0)

#define F64_ONLY(h, name)                                                                                 \
  if ((h) && (h)->dtype != 0)                                                                             \
  return fail(h, MOM_EINVAL, name ": not available on a Float32 (dtype = 1) handle (scene-level path only)")
