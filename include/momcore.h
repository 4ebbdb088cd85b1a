/*
 * momcore.h -- C ABI of libmomcore.so, the MI355X (gfx950) Matrix-Operator RT core.
 *
 * Drop-in boundary for ONE path of vSmartMOM.jl (RadiativeTransfer/RadiativeTransfer.jl):
 * the CoreRT layer-adding loop  elemental! -> doubling! -> interaction!  inside rt_run,
 * the Lambertian surface + post-processing that close it, and the Absorption line-shape
 * kernel (Voigt, Doppler and Lorentz broadening).  Every entry point names the reference interface it replaces
 * (file:line relative to the reference root).  A Julia maintainer binds these with
 * `ccall((:mom_xxx, libmomcore), Cint, (...), ...)` -- see INTEGRATION.md.
 *
 * Conventions
 *   - all functions return int status: MOM_OK (0) or a negative MOM_E* code; the text of
 *     the last error is available from mom_last_error().
 *   - arrays use the reference's memory order: Julia column-major [i, j, n] with the
 *     spectral index n slowest (batch stride N*N); sources are [i, 1, n]; optical depth
 *     tables are [nSpec, Nz] (model_from_parameters.jl:48); outputs are
 *     [nVza, nStokes, nSpec] (rt_run.jl:89-90).
 *   - indices passed as `*_1based` are Julia indices.
 *   - host pointers are borrowed for the duration of the call only.  All device memory is
 *     owned by the handle.  One handle <-> one GPU <-> one HIP stream; a handle is not
 *     thread-safe, distinct handles are independent.
 *   - `dtype` of mom_create: 0 = Float64 (the reference's default float_type), 1 = Float32 (float_type = Float32,
 *     parameters_from_yaml.jl:160): operators, sources and products in f32 on the GPU.  The ABI keeps Float64 host
 *     arrays for both (inputs are rounded on upload, outputs widened on download).  A Float32 handle supports the
 *     scene-level path -- mom_set_streams, mom_scene_set, mom_scene_set_optics with the mom_absorption_* / mom_voigt_tau_abs* /
 *     mom_lineshape_tau_abs* entry points that feed it, mom_absorption_set_model and mom_absorption_get_gamma_l included (the layer optics are assembled in Float64 on the device and rounded to Float32 there),
 *     mom_scene_set_surface, mom_set_option, mom_rt_run, mom_get_RT, mom_get_hdr, mom_timers, mom_sync, mom_check: the lane- and wave-per-point kernels (incl. the packed
 *     points at N = 5 ... 8), the strip-chained images (N = 36 ... 60, 4-wave builds: two workgroups per CU), the m = 0
 *     (I,Q) reduction and the padding to the strip sizes --, the operator-level API -- mom_elemental, mom_doubling,
 *     mom_interaction, mom_copy_added_to_composite, mom_surface_lambertian, mom_upload, mom_download (the operator-level
 *     composite layer is kept apart from the scene-level state on such a handle) -- and the two batched operators
 *     mom_batch_inv / mom_batched_mul (gpu_batched.jl:45-58); every other entry point returns MOM_EINVAL on it.
 */
#ifndef MOMCORE_H
#define MOMCORE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mom_handle mom_t;

enum {
  MOM_OK = 0,
  MOM_EINVAL = -1,   /* bad argument */
  MOM_EHIP = -2,     /* HIP runtime error (no device, launch failure, OOM ...) */
  MOM_ESTATE = -3,   /* call sequence error (e.g. streams not set) */
  MOM_ESINGULAR = -4, /* an (I - R r) operator was numerically singular (zero pivot) */
  MOM_EUNSUPPORTED = -5 /* the reference itself raises on this path (RRS strict position), or outside the built scope */
};

/* which-codes for mom_upload / mom_download (AddedLayer / CompositeLayer fields,
 * types.jl:105-142).  Matrices are N*N*S doubles, sources N*S doubles.
 * The surface layer (rt_run.jl:111-112 `added_layer_surface`) is a second AddedLayer. */
enum {
  MOM_ADDED_R_PM = 0, MOM_ADDED_R_MP = 1, MOM_ADDED_T_MM = 2, MOM_ADDED_T_PP = 3,
  MOM_ADDED_J0P = 4, MOM_ADDED_J0M = 5,
  MOM_COMP_R_MP = 6, MOM_COMP_R_PM = 7, MOM_COMP_T_PP = 8, MOM_COMP_T_MM = 9,
  MOM_COMP_J0P = 10, MOM_COMP_J0M = 11,
  MOM_SURF_R_PM = 12, MOM_SURF_R_MP = 13, MOM_SURF_T_MM = 14, MOM_SURF_T_PP = 15,
  MOM_SURF_J0P = 16, MOM_SURF_J0M = 17
};

/* ---- lifetime ------------------------------------------------------------------------ */

/* Allocates the layer state of rt_run.jl:109-115 (make_added_layer x2, make_composite_layer;
 * rt_helper_functions.jl:105-121,152-159) on GPU `device` for operators of edge
 * N = nStokes*Nquad and S spectral points, for up to `max_m` Fourier moments processed
 * as one batch (the moments of rt_run.jl:125 are independent).  */
int mom_create(mom_t **out, int device, int N, int nStokes, int S, int max_m, int dtype);
int mom_destroy(mom_t *h);
const char *mom_last_error(const mom_t *h);
/* library-level error text for failures that happen before a handle exists */
const char *mom_last_global_error(void);
/* blocks until everything queued on the handle's stream has finished */
int mom_sync(mom_t *h);
/* mom_sync + the deferred error report of the asynchronous calls (MOM_ESINGULAR if a kernel met a zero pivot) */
int mom_check(mom_t *h);

/* QuadPoints (types.jl:456-473) + polarization type (Scattering/types.jl:82-123).
 * qp_muN/wt_muN: N values (already repeated per Stokes component); imu0_1based = iμ₀;
 * mu0 = quad_points.μ₀; I0, D: nStokes values.  strict_reference_indexing != 0 keeps the
 * reference's 1-based `mod(i, nStokes)` Stokes-component rule of elemental.jl:259-269,
 * doubling.jl:95-117; 0 uses the zero-based component. */
int mom_set_streams(mom_t *h, const double *qp_muN, const double *wt_muN, int N, int imu0_1based, double mu0,
                    const double *I0, const double *D, int strict_reference_indexing);

/* ---- operator-level API: one call per reference operator (used for parity tests and for
 *      a Julia shim that overloads the operators one by one) ------------------------------ */

/* elemental!(pol_type, SFI, τ_sum, dτ, computed_layer_properties, m, ndoubl, scatter, quad_points,
 *            added_layer, architecture)  -- elemental.jl:109-162 (+ kernels :164-285).
 * tau_sum, dtau, varpi: S values; Zpp/Zmp: N*N*z_batch with z_batch = 1 or S
 * (expandOpticalProperties, compEffectiveLayerProperties.jl:124-135).  Fills the added layer. */
int mom_elemental(mom_t *h, int m, int ndoubl, const double *tau_sum, const double *dtau, const double *varpi,
                  const double *Zpp, const double *Zmp, int z_batch);

/* doubling!(pol_type, SFI, expk, ndoubl, added_layer, I_static, architecture) -- doubling.jl:81-91
 * (helper :13-79).  expk: S values, updated in place like the reference's `expk .= expk.^2`. */
int mom_doubling(mom_t *h, int ndoubl, double *expk);

/* interaction!(RS_type::noRS, scattering_interface, SFI, composite_layer, added_layer, I_static)
 * -- interaction_inelastic.jl:474-484 -> interaction.jl:8-117.
 * iface: 0 = ScatteringInterface_00, 1 = _01, 2 = _10, 3 = _11.
 * with_surface_layer != 0 uses added_layer_surface instead of added_layer (rt_run.jl:179-185). */
int mom_interaction(mom_t *h, int iface, int with_surface_layer);

/* rt_kernel.jl:227-230: composite <- added (first layer, iz == 1) */
int mom_copy_added_to_composite(mom_t *h);

/* create_surface_layer!(::LambertianSurfaceScalar, added_layer_surface, SFI, m, pol_type, quad_points,
 *                       τ_sum, architecture) -- lambertian_surface.jl:20-75.  tau_tot: S values. */
int mom_surface_lambertian(mom_t *h, int m, double albedo, const double *tau_tot);

/* elemental_inelastic!(RS_type::RRS, pol_type, SFI, τ_sum, dτ_λ, ϖ_λ, Z⁺⁺_λ₁λ₀, Z⁻⁺_λ₁λ₀, m, ndoubl, scatter, quad_points,
 *                      added_layer, I_static, architecture) -- CoreKernel/elemental_inelastic.jl:23-91: the elemental layer of
 * the rotational-Raman source operators (get_elem_rt_RRS! :93-160, get_elem_rt_SFI_RRS! :320-382, apply_D_elemental_RRS!
 * :384-402).  i_l1l0 [nRaman]: grid offsets n₀ - n₁ of the Raman lines (RS_type.i_λ₁λ₀), varpi_l1l0 [nRaman], fscattRayl,
 * tau_sum, dtau, varpi [nSpec], Z*_l1l0 [N,N].  Outputs (host): ier⁻⁺, iet⁺⁺, ier⁺⁻, iet⁻⁻ [N,N,nSpec,nRaman], ieJ₀⁺, ieJ₀⁻
 * [N,nSpec,nRaman] (Julia [N,1,nSpec,nRaman]).  For ndoubl >= 1 the reference leaves ier⁺⁻ / iet⁻⁻ untouched (they are
 * filled after doubling); zeros are returned.  Stateless form (fresh arrays in, host arrays out); the stateful RRS path
 * below (mom_rrs_*) keeps the reference's persistent AddedLayerRS instead. */
int mom_elemental_inelastic_rrs(mom_t *h, int m, int ndoubl, int nRaman, const int *i_l1l0, const double *varpi_l1l0,
                                const double *fscattRayl, const double *tau_sum, const double *dtau, const double *varpi,
                                const double *Zpp_l1l0, const double *Zmp_l1l0, double *ier_mp, double *iet_pp,
                                double *ier_pm, double *iet_mm, double *ieJ0p, double *ieJ0m);

/* ---- rotational-Raman scattering (BASELINE config 5): rt_run(RS_type::RRS, model, iBand) ---------------------------
 *
 * The reference's inelastic branch keeps, next to the elastic layers, the 4-D operators ier-+, ier+-, iet++, iet--
 * [N,N,nSpec,nRaman] and sources ieJ0+-[N,1,nSpec,nRaman] of the added layer and ieR-+, ieR+-, ieT++, ieT--, ieJ0+- of the
 * composite layer (AddedLayerRS / CompositeLayerRS, src/CoreRT/types.jl:145-205): element [.., n1, dn] takes radiation
 * from spectral index n0 = n1 + i_l1l0[dn] to n1.  These layers persist over layers and Fourier moments exactly like the
 * reference's (rt_run.jl:108-116), in the reference's memory order.
 *
 *   mom_rrs_set        the fields of the RRS struct (src/Inelastic/types.jl:13-33) the path reads: i_l1l0 [nRaman] (grid
 *                      offsets n0 - n1, |offset| < nSpec), varpi_l1l0 [nRaman]; allocates the layers (zeros, like
 *                      make_added_layer(::RRS, ...) rt_helper_functions.jl:127-141).  N <= 64 (N <= 16: one MFMA tile per operator and wavefront,
 *                      <= 32: 2 x 2 tiles in registers, <= 48 / <= 64: 3 x 3 / 4 x 4 tiles with the operators in scratch).
 *                      rrs_strict_reference: the reference's RRS text has defects (DESIGN.md "RRS", D1..D5); != 0 executes
 *                      it AS WRITTEN with the semantics of a single-threaded Julia run -- and returns MOM_EUNSUPPORTED
 *                      where the reference raises (interaction_helper! for interfaces 00/01/10, a MethodError) --,
 *                      0 applies the five documented corrections and nothing else.
 *   mom_rrs_elemental  rt_kernel!(::RRS) rt_kernel.jl:277-304: elemental_inelastic!(RS_type, pol_type, SFI, tau_sum, dtau, varpi,
 *                      Z++_l1l0, Z-+_l1l0, m, ndoubl, scatter, quad_points, added_layer, I_static, architecture)
 *                      (CoreKernel/elemental_inelastic.jl:23-91) followed by elemental!(...) (elemental.jl:109-162) on the
 *                      persistent added layer.  tau_sum, dtau, varpi, fscattRayl [nSpec]; Z* [N,N] (one phase matrix).
 *   mom_rrs_doubling   doubling_inelastic!(RS_type, pol_type, SFI, expk, ndoubl, added_layer, I_static, architecture)
 *                      (CoreKernel/doubling_inelastic.jl:13-134, 263-280); expk [nSpec] updated in place.
 *   mom_rrs_interaction  interaction!(RS_type::RRS, scattering_interface, SFI, composite_layer, added_layer, I_static)
 *                      (CoreKernel/interaction_inelastic.jl:464-472 -> :8-340); with_surface_layer != 0 uses added_layer_surface,
 *                      whose ie* arrays the reference never writes (zeros).
 *   mom_rrs_copy_added_to_composite   rt_kernel.jl:326-333 (iz == 1), all twelve arrays.
 *   mom_rrs_surface_lambertian        create_surface_layer!(::LambertianSurfaceScalar) into added_layer_surface.
 *   mom_rrs_upload / mom_rrs_download  test access; which = MOM_ADDED_* / MOM_COMP_* / MOM_SURF_* for the elastic fields of the RRS
 *                      layers, MOM_IE_ADDED_* / MOM_IE_COMP_* for the 4-D fields ([N,N,nSpec,nRaman] / [N,nSpec,nRaman]).
 *   mom_scene_set_rrs  scene-level inputs on top of mom_scene_set: fscattRayl [nSpec, Nz] (fScattRayleigh of
 *                      constructCoreOpticalProperties, compEffectiveLayerProperties.jl:58, expanded per band), Z*_l1l0 [N,N,M]
 *                      (computeRamanZlambda!, src/Inelastic/inelastic_helper.jl:457-464, per Fourier moment).
 *   mom_rt_run_rrs     rt_run.jl:125-215 with RS_type::RRS for the resident scene (every surface kind of
 *                      mom_scene_set_surface); asynchronous.
 *   mom_rrs_set_shard  spectral sharding of the RRS path (the Raman operators couple spectral points at the
 *                      offsets i_l1l0, inelastic_helper.jl:13-21, so a shard carries a halo): the handle's nSpec points are the
 *                      window [n_glob0, n_glob0 + nSpec) of a global axis of nSpec_global points, of which this rank OWNS the
 *                      local indices [n1_lo, n1_hi).  The elastic layers are computed for the whole window (they are the
 *                      operands at n0 = n1 + i_l1l0), the inelastic pairs (n1, dn) and the spectra only for the owned
 *                      points; on an interior edge the halo must be at least max |i_l1l0| long (MOM_EINVAL otherwise).
 *                      ndoubl / interface codes must come from the GLOBAL axis (rt_kernel.jl:241-242), as in the elastic
 *                      sharding.  Call after mom_rrs_set; the default is the whole window, n_glob0 = 0.
 *   mom_get_RT_rrs     R_SFI, T_SFI, ieR_SFI, ieT_SFI [nVza, nStokes, nSpec] (postprocessing_vza!(::RRS),
 *                      tools/postprocessing_vza.jl:95-147); any pointer may be NULL; gpu_ms (optional) = GPU time of the run.
 *   mom_get_hdr_rrs    the elastic RAMI extras of the same return tuple (rt_run.jl:187-213, 226): hdr [nVza, nStokes, nSpec],
 *                      bhr_uw, bhr_dw [nStokes, nSpec] (interaction_hdrf! + postprocessing_vza_hdrf!).
 *   mom_rrs_timers     HIP-event times of the last mom_rt_run_rrs, summed per kernel: ms[0] / launches[0] the doubling pair
 *                      kernel, [1] the interaction pair kernel, [2] the inelastic elemental kernel, [3] the whole run (n >= 4).
 *   mom_get_spectra_rrs_device  the SEVEN spectra of the return tuple (rt_run.jl:226) restricted to the owned points
 *                      [n1_lo, n1_hi) of mom_rrs_set_shard, packed into the caller's DEVICE buffer as
 *                      [R | T | ieR | ieT | hdr][nVza, nStokes, per] then [bhr_uw | bhr_dw][nStokes, per]; per >= owned count,
 *                      tails zero (ragged last shard); mom_rrs_spectra_count(h, per) doubles; asynchronous.
 *   mom_allgather_rrs_device    the ONE collective of a sharded RRS run: that block of every rank into d_global
 *                      [nranks][mom_rrs_spectra_count(h, per)] (RCCL on the handle's stream; the reference has no
 *                      multi-GPU path -- SURVEY section 8e / 8f-3; needs mom_comm_init). */
enum {
  MOM_IE_ADDED_R_PM = 18, MOM_IE_ADDED_R_MP = 19, MOM_IE_ADDED_T_MM = 20, MOM_IE_ADDED_T_PP = 21,
  MOM_IE_ADDED_J0P = 22, MOM_IE_ADDED_J0M = 23,
  MOM_IE_COMP_R_MP = 24, MOM_IE_COMP_R_PM = 25, MOM_IE_COMP_T_PP = 26, MOM_IE_COMP_T_MM = 27,
  MOM_IE_COMP_J0P = 28, MOM_IE_COMP_J0M = 29
};
int mom_rrs_set(mom_t *h, int nRaman, const int *i_l1l0, const double *varpi_l1l0, int rrs_strict_reference);
int mom_rrs_set_shard(mom_t *h, int nSpec_global, int n_glob0, int n1_lo, int n1_hi);
int mom_rrs_elemental(mom_t *h, int m, int ndoubl, const double *tau_sum, const double *dtau, const double *varpi,
                      const double *Zpp, const double *Zmp, const double *fscattRayl, const double *Zpp_l1l0,
                      const double *Zmp_l1l0);
int mom_rrs_doubling(mom_t *h, int ndoubl, double *expk);
int mom_rrs_interaction(mom_t *h, int iface, int with_surface_layer);
int mom_rrs_copy_added_to_composite(mom_t *h);
int mom_rrs_surface_lambertian(mom_t *h, int m, double albedo, const double *tau_tot);
int mom_rrs_upload(mom_t *h, int which, const double *src);
int mom_rrs_download(mom_t *h, int which, double *dst);
int mom_scene_set_rrs(mom_t *h, const double *fscattRayl, const double *Zpp_l1l0, const double *Zmp_l1l0);
int mom_rt_run_rrs(mom_t *h);
int mom_get_RT_rrs(mom_t *h, double *R_SFI, double *T_SFI, double *ieR_SFI, double *ieT_SFI, double *gpu_ms);
int mom_get_hdr_rrs(mom_t *h, double *hdr, double *bhr_uw, double *bhr_dw);
int mom_rrs_timers(mom_t *h, double *ms, int *launches, int n);
/* test access: number of nonzero entries in the zero padding of the handle's RRS layer arrays (device blocks are padded to the
 * MFMA tiling and the kernels store whole tiles: the padding must stay zero by value); 0 = intact */
int mom_rrs_check_padding(mom_t *h, unsigned long long *violations);
size_t mom_rrs_spectra_count(mom_t *h, int per);
int mom_get_spectra_rrs_device(mom_t *h, int per, void *d_local);
int mom_allgather_rrs_device(mom_t *h, int per, void *d_global);

/* batch_inv!(X, A) -- gpu_batched.jl:36-87;  X, A: n*n*batch doubles (host). */
int mom_batch_inv(mom_t *h, int n, int batch, const double *A, double *X);
/* A ⊠ B = batched_mul(A, B) -- gpu_batched.jl:90-97. */
int mom_batched_mul(mom_t *h, int n, int batch, const double *A, const double *B, double *C);
/* The ForwardDiff.Dual methods of the same two operators (gpu_batched.jl:100-150), values and partials as separate
 * arrays: values [n,n,batch], partials [n,n,batch,P] (one [n,n,batch] block per partial i = ForwardDiff.partials.(A, i)).
 *   batched_mul:  C = A ⊠ B,   dC_i = A ⊠ dB_i + dA_i ⊠ B            (gpu_batched.jl:100-110)
 *   batch_inv!:   X = A⁻¹,     dX_i = -A⁻¹ ⊠ dA_i ⊠ A⁻¹              (gpu_batched.jl:129-150)
 * P = 0 reduces to the plain operators (dA/dB/dC may be NULL then). */
int mom_batched_mul_dual(mom_t *h, int n, int batch, int P, const double *A, const double *dA, const double *B,
                         const double *dB, double *C, double *dC);
int mom_batch_inv_dual(mom_t *h, int n, int batch, int P, const double *A, const double *dA, double *X, double *dX);

/* Array(composite_layer.J₀⁻) etc. (postprocessing_vza.jl:17-20) / test access.
 * Operator-level state lives in moment slot 0 of the handle; the added and surface layers are allocated on the
 * first operator-level call.  After a scene-level mom_rt_run the composite codes return Fourier moment 0 of that
 * run in the same [N,N,nSpec] / [N,nSpec] layout (the internal row pitch is removed), or MOM_ESTATE when moment 0
 * ran on the (I,Q) sub-problem (MOM_OPT_M0_REDUCTION); mom_interaction / mom_postprocess refuse to continue from
 * scene-level state (MOM_ESTATE) until mom_copy_added_to_composite or a composite mom_upload restarts the
 * operator-level sequence. */
int mom_upload(mom_t *h, int which, const double *src);
int mom_download(mom_t *h, int which, double *dst);

/* postprocessing_vza!(RS_type::noRS, iμ₀, pol_type, composite_layer, vza, qp_μ, m, vaz, μ₀, weight, nSpec, SFI, R, R_SFI,
 * T, T_SFI, ieR_SFI, ieT_SFI) -- postprocessing_vza.jl:9-60, SFI branch, for ONE Fourier moment m of the
 * operator-level composite layer: R_SFI[i,:,s] += bigCS * J₀⁻[rows(i),1,s], T_SFI likewise with J₀⁺ (:48-49);
 * node_1based[i] = nearest_point(qp_μ, cosd(vza[i])) (:28), vaz_deg in degrees, weight = 0.5 for m = 0 else 1
 * (rt_run.jl:128).  R_SFI, T_SFI: [nVza, nStokes, nSpec] host arrays, accumulated in place like the reference. */
int mom_postprocess(mom_t *h, int m, int nVza, const int *node_1based, const double *vaz_deg, double weight,
                    double *R_SFI, double *T_SFI);

/* ---- scene-level API: inputs resident in HBM, fused per-layer kernels -------------------
 *
 * mom_scene_set uploads everything rt_run's loops (rt_run.jl:125-215) consume, prepared by
 * the host exactly as the reference's host code does (constructCoreOpticalProperties /
 * extractEffectiveProps / get_dtau_ndoubl):
 *   tau, varpi  [S, Nz]         layer optical depth and single-scattering albedo
 *   zw          [K, S, Nz]      weights of the K phase-matrix bases (Rayleigh + aerosols):
 *                               Z[:,:,n] = sum_k zw[k,n,z] * Zbasis_k  (types.jl:656-661)
 *   Zpp, Zmp    [N, N, K, M]    compute_Z_moments per basis and Fourier moment
 *   ndoubl      [Nz]            doubling_number per layer (GLOBAL over the spectral axis,
 *                               rt_kernel.jl:238-246 -- compute before sharding)
 *   iface       [Nz]            scattering-interface codes (rt_helper_functions.jl:8-27)
 *   tau_sum     [S, Nz+1]       cumulative optical depth (compEffectiveLayerProperties.jl:108)
 *   albedo                      LambertianSurfaceScalar
 *   node_1based [nVza]          nearest stream per view (postprocessing_vza.jl:28)
 *   cos_mphi, sin_mphi [nVza, M] cosd(m*vaz), sind(m*vaz) (postprocessing_vza.jl:32)
 *
 * m = 0 reduction.  For Fourier moment 0 the generalized spherical function T_l^0 vanishes, so every
 * phase-matrix basis from compute_Z_moments couples (I,Q) only with (I,Q) and (U,V) only with (U,V)
 * (compute_Z_matrices.jl:36-57 with legendre_functions.jl:38-58).  With an unpolarised source
 * (I0 = [1,0,0(,0)]) and a Lambertian surface the (U,V) block then has no source: it never reaches
 * R_SFI/T_SFI/hdr (its azimuthal weight sin(0) is 0 as well), and the (I,Q) block evolves exactly as in
 * the full problem (the cross products are exact zeros).  mom_scene_set verifies these conditions on the
 * uploaded arrays (bitwise zeros) and, if they hold, runs moment 0 on operators of edge 2*Nquad; the
 * outputs are unchanged.  MOM_OPT_M0_REDUCTION = 0 disables it.
 */
int mom_scene_set(mom_t *h, int Nz, int K, int M, const double *tau, const double *varpi, const double *zw,
                  const double *Zpp, const double *Zmp, const int *ndoubl, const int *iface, const double *tau_sum,
                  double albedo, int nVza, const int *node_1based, const double *cos_mphi, const double *sin_mphi);

/* ---- device-side layer optics: tau_abs never visits the host -----------------------
 *
 * mom_absorption_begin   τ_abs = zeros(nSpec, Nz) resident in HBM (model_from_parameters.jl:48) + the spectral grid
 *                        [nSpec] the line shapes are evaluated on (NULL keeps a previously uploaded grid)
 * mom_voigt_tau_abs      compute_absorption_profile! for ONE layer (atmo_prof.jl:427-449):
 *                          τ_abs[:, iz] += absorption_cross_section(model, grid, p[iz], T[iz]) * vcd_dry[iz] * vmr
 *                        with the Voigt/HW32SD line shape; the host passes the per-line prefactors like for
 *                        mom_voigt_xsec and factor = vcd_dry[iz] * vmr; σ is accumulated straight into the resident
 *                        table by the line-shape kernel (no σ round trip, no allocation in steady state)
 * mom_absorption_set     uploads a host τ_abs [nSpec, Nz] instead (ABSCO/LUT or synthetic tables)
 * mom_absorption_get     test access
 * mom_scene_set_optics   mom_scene_set with the layer optics assembled ON THE DEVICE from their ingredients:
 *                        constructCoreOpticalProperties (compEffectiveLayerProperties.jl:1-78) = Rayleigh
 *                        (tau_rayl [nSpec, Nz], ϖ = varpi_rayl = ϖ_Cabannes) `+` each aerosol type (createAero :80-85:
 *                        tau_aer [nAer, Nz], omega_aer, ft_aer [nAer]; types.jl:632-661) `+` the resident gas
 *                        absorption (:672-678), τ_sum (:108), then ndoubl (rt_kernel.jl:238-246) and the
 *                        interface codes (rt_helper_functions.jl:8-27) from per-layer maxima of τϖ -- reduced over all
 *                        ranks first when a communicator is initialised (mom_comm_init), so a sharded run uses the
 *                        GLOBAL doubling numbers.  Zpp/Zmp: [N, N, 1 + nAer, M].  Results are bitwise those of the
 *                        host route (mom_scene_set fed by the reference's host algebra).
 * mom_scene_get_layers   ndoubl / iface [Nz] and (optionally, NULL to skip) τ, ϖ [nSpec,Nz], zw [K,nSpec,Nz],
 *                        τ_sum [nSpec,Nz+1] of the resident scene */
int mom_absorption_begin(mom_t *h, int Nz, const double *grid);
/* The same accumulation with the per-line prefactors formed ON THE DEVICE (last clause):
 *   mom_absorption_set_lines   ONE resident table per absorber: the HITRAN columns (read_hitran.jl:14-68) of the lines inside
 *                              the padded grid -- selected once by the host, compute_absorption_cross_section.jl:54-72 --,
 *                              sqrt_mol_weight = Float64(sqrt(mol_weight(mol, iso)::Float32)) per line, iso_index = the line's
 *                              row in the TIPS tables below, and for each of the nIso isotopologues in use the TIPS-2017
 *                              table as qoft! (:197-214) interpolates it: nT[k] knots tips_T, values tips_Q and the second
 *                              derivatives tips_z of DataInterpolations.CubicSpline ([nTmax, nIso] column-major, i.e. one
 *                              row of nTmax entries per isotopologue; computed once by the host in the tables' Float32).
 *   mom_voigt_tau_abs_layer    compute_absorption_profile! for layer iz (atmo_prof.jl:427-449): pressure shift, Lorentz and
 *                              Doppler widths, y, TIPS ratio, Boltzmann and stimulated-emission factors, grid windows
 *                              (compute_absorption_cross_section.jl:79-107) by k_line_prefactors, then the Voigt kernel adds
 *                              sigma * factor into tau_abs[:, iz].  Only (p, T, vmr, wing_cutoff, factor) cross the bus.
 *                              Agrees with the host route (mom_voigt_tau_abs fed by the host's prefactors) to rounding of
 *                              exp/pow (device vs host libm), not bitwise.
 *   mom_absorption_get_prefactors   the prefactors of the last layer call (test access). */
int mom_absorption_set_lines(mom_t *h, int nLines, const double *nu0, const double *S0, const double *gamma_air,
                             const double *gamma_self, const double *E_lower, const double *n_air, const double *delta_air,
                             const double *sqrt_mol_weight, const int *iso_index, int nIso, int nTmax, const int *nT,
                             const double *tips_T, const double *tips_Q, const double *tips_z);
int mom_voigt_tau_abs_layer(mom_t *h, int iz_1based, double pressure, double temperature, double vmr, double wing_cutoff,
                            double factor);
/* compute_absorption_profile! (atmo_prof.jl:427-449) for layers 1..Nz of the profile in TWO launches (prefactors of every
 * (layer, line) pair, line shapes of every (layer, grid point) pair) instead of the reference's host loop over layers with
 * one launch per line: tau_abs[:, z] += sigma(nu; pressure[z], temperature[z]) * factor[z], factor[z] = vcd_dry[z] * vmr[z].
 * Same arithmetic per layer as mom_voigt_tau_abs_layer (bitwise).  gpu_ms (may be NULL): HIP-event time of the two kernels. */
int mom_voigt_tau_abs_profile(mom_t *h, int Nz, const double *pressure, const double *temperature, double vmr, double wing_cutoff,
                              const double *factor, double *gpu_ms);
int mom_absorption_get_prefactors(mom_t *h, int n, double *nu, double *gamma_d, double *y, double *S, int *ind_start_1based,
                                  int *ind_stop_1based);
int mom_voigt_tau_abs(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *y,
                      const double *S, const int *ind_start_1based, const int *ind_stop_1based, double factor);
int mom_absorption_set(mom_t *h, int Nz, const double *tau_abs);
int mom_absorption_get(mom_t *h, double *tau_abs);
/* ---- The Dual run of the absorption path: tau_abs together with its partials with respect to each layer's pressure (k = 0)
 * and temperature (k = 1) -- ForwardDiff.Dual numbers through compute_absorption_cross_section, as
 * absorption_cross_section(model, grid, p, T; autodiff = true) runs it (autodiff_helper.jl:17-51).  The partials are those of
 * the reference's statements as written (the two rational approximations of w(z), not the exact Faddeeva function); integer
 * and boolean decisions (line selection, grid windows, the branch |x| + y >= 8 of w, E_lower != -1, the TIPS range) are taken
 * on the values.  Float64 and Float32 handles alike: the absorption table is Float64 on both.
 *   mom_voigt_tau_abs_dual          mom_voigt_tau_abs that also takes the partials of the four per-line prefactors, each
 *                                   [nLines, 2] column-major (index j + nLines k; NULL = zeros), and adds d_k sigma * factor into
 *                                   dtau_abs[:, iz, k] (factor = vcd_dry[iz] * vmr is a constant)
 *   mom_voigt_tau_abs_profile_dual  mom_voigt_tau_abs_profile (same checks, two launches for all layers) whose prefactor kernel
 *                                   also forms those partials on the device
 *   mom_absorption_get_partials     dtau_abs [nSpec, Nz, 2] (partial index slowest).  The table is allocated and zeroed by the
 *                                   first Dual call after mom_absorption_begin, zeroed by mom_absorption_begin, dropped by
 *                                   mom_absorption_set (a host table has no partials); without it: MOM_ESTATE.  A value call
 *                                   (mom_voigt_tau_abs, _layer, _profile) into the same table adds an absorber whose partials
 *                                   count as zero.
 *   mom_absorption_get_prefactor_partials   the partials of the prefactors of the last Dual call (last layer of a profile
 *                                   call), each [n, 2] column-major, NULL to skip (test access). */
int mom_voigt_tau_abs_dual(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *y,
                           const double *S, const double *dnu, const double *dgamma_d, const double *dy, const double *dS,
                           const int *ind_start_1based, const int *ind_stop_1based, double factor);
int mom_voigt_tau_abs_profile_dual(mom_t *h, int Nz, const double *pressure, const double *temperature, double vmr,
                                   double wing_cutoff, const double *factor, double *gpu_ms);
int mom_absorption_get_partials(mom_t *h, double *dtau_abs);
int mom_absorption_get_prefactor_partials(mom_t *h, int n, double *dnu, double *dgamma_d, double *dy, double *dS);
enum { MOM_BROADENING_VOIGT = 0, MOM_BROADENING_DOPPLER = 1, MOM_BROADENING_LORENTZ = 2 };
enum { MOM_CEF_HW32SD = 0, MOM_CEF_HW32VOIGT = 1 };
/* ---- The absorption model: HitranModel.broadening and HitranModel.CEF (Absorption/types.jl; the YAML reader's
 * `broadening: Voigt() | Doppler() | Lorentz()` and `CEF:`, parameters_from_yaml.jl:114-115) select the method of line_shape!
 * (compute_absorption_cross_section.jl:167-183) and of w(CEF, z) (complex_error_functions.jl:195-271).  Built: Voigt with
 * HumlicekWeidemann32SDErrorFunction (:226-234, the default) or HumlicekWeidemann32VoigtErrorFunction (:210-219), Doppler and
 * Lorentz (which ignore the CEF, as the reference's methods do).  Value and Dual run, Float64 and Float32 handles alike.
 *   mom_absorption_set_model    the model of every later absorption call on the handle, kept until changed (also across
 *                               mom_absorption_begin, and allowed between two absorbers accumulated into one table); an unknown
 *                               code: MOM_EINVAL with the code in the text.  The device-prefactor entry points
 *                               (mom_voigt_tau_abs_layer, _profile, _profile_dual) follow it; mom_voigt_tau_abs / _dual take
 *                               no gamma_l, run Voigt with the handle's CEF and return MOM_ESTATE (pointing to
 *                               mom_lineshape_tau_abs) when the handle's broadening is not Voigt.
 *   mom_lineshape_tau_abs       mom_voigt_tau_abs for the handle's model: the five per-line prefactors that line_shape! takes
 *                               (compute_absorption_cross_section.jl:118-124).  An array the broadening does not read may be
 *                               NULL (Voigt: gamma_l; Doppler: gamma_l, y; Lorentz: gamma_d, y), one it reads may not.
 *   mom_lineshape_tau_abs_dual  mom_voigt_tau_abs_dual likewise, with the partials of the five (NULL = zeros)
 *   mom_absorption_get_gamma_l  gamma_l (compute_absorption_cross_section.jl:82-84) of the last device-prefactor call (last
 *                               layer of a profile call) and, NULL to skip, its partials [n, 2] column-major of the last Dual
 *                               call (test access). */
int mom_absorption_set_model(mom_t *h, int broadening, int cef);
/* line_shape!(A, grid, nu, gamma_d, gamma_l, y, S, broadening, CEF) (compute_absorption_cross_section.jl:167-183) of the handle's
 * model, accumulated into tau_abs[:, iz] like mom_voigt_tau_abs (atmo_prof.jl:427-449) */
int mom_lineshape_tau_abs(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *gamma_l,
                          const double *y, const double *S, const int *ind_start_1based, const int *ind_stop_1based, double factor);
/* ... on ForwardDiff.Dual numbers (autodiff_helper.jl:17-51), like mom_voigt_tau_abs_dual */
int mom_lineshape_tau_abs_dual(mom_t *h, int iz_1based, int nLines, const double *nu, const double *gamma_d, const double *gamma_l,
                               const double *y, const double *S, const double *dnu, const double *dgamma_d, const double *dgamma_l,
                               const double *dy, const double *dS, const int *ind_start_1based, const int *ind_stop_1based,
                               double factor);
/* gamma_l of compute_absorption_cross_section.jl:82-84 as the device formed it (test access) */
int mom_absorption_get_gamma_l(mom_t *h, int n, double *gamma_l, double *dgamma_l);
int mom_scene_set_optics(mom_t *h, int Nz, int nAer, int M, const double *tau_rayl, double varpi_rayl,
                         const double *tau_aer, const double *omega_aer, const double *ft_aer, const double *Zpp,
                         const double *Zmp, double albedo, int nVza, const int *node_1based, const double *cos_mphi,
                         const double *sin_mphi);
int mom_scene_get_layers(mom_t *h, int *ndoubl, int *iface, double *tau, double *varpi, double *zw, double *tau_sum);
/* ---- Band-resolved aerosol optics: mom_scene_set_optics for a spectral axis that concatenates nBand bands ----------
 * The reference keeps the aerosols per band -- model.aerosol_optics[iBand][iAer], model.τ_aer[iBand][iAer, iz]
 * (model_from_parameters.jl:92-166), RS_type.ϖ_Cabannes[iB] -- and constructCoreOpticalProperties runs the `+` algebra band by
 * band before it concatenates the bands with `*` (compEffectiveLayerProperties.jl:24-75, types.jl:632-678).
 *
 * mom_scene_set_optics_bands   band b (0-based) owns the points band_start[b] <= n < band_start[b+1] of the spectral axis;
 *                          band_start [nBand + 1] runs strictly ascending from 0 to nSpec, otherwise MOM_EINVAL with the reason.
 *                          varpi_rayl [nBand] = ϖ_Cabannes[iB]; tau_aer [nAer, Nz, nBand] = τ_aer[iB][iAer, iz] (iAer fastest);
 *                          omega_aer, ft_aer [nAer, nBand] = ω̃, fᵗ of aerosol_optics[iB][iAer].  The scene has
 *                          K = 1 + nAer nBand <= 64 phase-matrix bases: Zpp/Zmp [N, N, K, M] with basis 0 = Rayleigh and basis
 *                          1 + iAer + nAer b = aerosol type iAer of band b; a point's weights zw outside its own band are exact
 *                          zeros.  Per band the statements are mom_scene_set_optics' (createAero, the three cases of `+` with the
 *                          two all(. == 0) tests taken over the band's own points, the gas term); ndoubl, the interface codes and
 *                          τ_sum are taken over the concatenated axis (rt_kernel.jl:241-242, compEffectiveLayerProperties.jl:
 *                          104-108).  Results are bitwise those of the host route (mom_scene_set).  nAer <= 7, nBand >= 1.
 *                          Everything else as mom_scene_set_optics, Float32 handles included.  A handle with a communicator
 *                          (mom_comm_init): MOM_EUNSUPPORTED -- the per-band all-zero tests would need a reduction over the
 *                          ranks; a sharded band-resolved run keeps the host route (mom_scene_set with the slices of the host's
 *                          arrays). */
int mom_scene_set_optics_bands(mom_t *h, int Nz, int nAer, int nBand, const int *band_start, int M, const double *tau_rayl,
                               const double *varpi_rayl, const double *tau_aer, const double *omega_aer, const double *ft_aer,
                               const double *Zpp, const double *Zmp, double albedo, int nVza, const int *node_1based,
                               const double *cos_mphi, const double *sin_mphi);

/* Surface type of the resident scene (call after mom_scene_set / mom_scene_set_optics, which select
 * LambertianSurfaceScalar(albedo)):
 *   kind 0  LambertianSurfaceScalar (lambertian_surface.jl:20-75), the `albedo` of mom_scene_set
 *   kind 1  any BRDF surface handled by create_surface_layer!(brdf::AbstractSurfaceType, ...) (rpv_surface.jl:20-66:
 *           rpvSurfaceScalar, RossLiSurfaceScalar, ...): Rsurf [N, N, M] = the matrices the host obtains from
 *           reflectance(brdf, pol_type, qp_μ, m) (rpv_surface.jl:104-134), times 2 for m = 0 (:39-43).  The library
 *           forms j₀⁺, j₀⁻ = μ₀ (R_surf I₀) e^{-τ/μ₀}, r⁻⁺ = R_surf Diagonal(qp_μN .* wt_μN) (:48-62) and interacts
 *           the surface with the composite layer for EVERY Fourier moment; hdr accumulates over all moments.
 *   kind 2  LambertianSurfaceLegendre (lambertian_surface.jl:77-138): albedo_spec [nSpec] = P * legendre_coeff
 *           evaluated by the host (:90-96); reproduces that method's j₀⁺ = 0 (:112) and its t = 0 for m > 0 (:131-132).
 * Unused pointers may be NULL. */
int mom_scene_set_surface(mom_t *h, int kind, int M, const double *Rsurf, const double *albedo_spec);

/* The whole of rt_run.jl:125-215 for the resident scene: all Fourier moments, all layers,
 * surface, post-processing.  Asynchronous on the handle's stream; results stay on the GPU. */
int mom_rt_run(mom_t *h);

/* ---- rt_run on ForwardDiff.Dual numbers: Jacobians out of the hot path --------------------------------------------
 * The reference differentiates rt_run by running it on Dual element types: rt_run.jl:89-96 allocates R, T, R_SFI, T_SFI
 * in the Dual type of the optical properties, every AddedLayer / CompositeLayer array is a Dual array, and the two
 * batched operators have Dual methods (gpu_batched.jl:100-150).  This is that run for the resident scene: values and P
 * partials of every layer operator go through elemental! / doubling! / interaction! / create_surface_layer! /
 * postprocessing_vza! together (csrc/mom_dual.hip: the Dual product rule per product, dX = -X dA X per inverse, the
 * analytic derivative of every elemental expression; integer decisions -- ndoubl, interface codes -- are the value run's,
 * as ForwardDiff takes them on the values).
 *
 * mom_scene_set_partials   the partials of what mom_scene_set / mom_scene_set_surface uploaded, i.e. of the Dual inputs the
 *                          reference's host code (model_from_parameters on Dual parameters) hands to rt_run.  Layouts are
 *                          those of the value arrays with the partial index as the SLOWEST axis; NULL = no dependence:
 *                            dtau, dvarpi [S, Nz, P];  dzw [K, S, Nz, P];  dZpp, dZmp [N, N, K, M, P] (both or neither);
 *                            dalbedo [P] (LambertianSurfaceScalar);  dRsurf [N, N, M, P] (surface kind 1);
 *                            dalbedo_spec [S, P] (kind 2).
 *                          Call after mom_scene_set (and mom_scene_set_surface); P = 0 clears them (values only).
 * mom_rt_run_dual          the run; R_SFI / T_SFI are then read with mom_get_RT (they agree with mom_rt_run's to rounding:
 *                          the same statements in a different association), the partials with mom_get_RT_partials.
 *                          hdr / bhr_uw / bhr_dw (interaction_hdrf!, postprocessing_vza_hdrf!) come out as well: values through
 *                          mom_get_hdr, partials through mom_get_hdr_partials.  Operators larger than 128 x 128 return
 *                          MOM_EUNSUPPORTED.
 * mom_get_RT_partials      dR_SFI, dT_SFI [nVza, nStokes, nSpec, P] (host).
 * mom_get_hdr_partials     dhdr [nVza, nStokes, nSpec, P], dbhr_uw, dbhr_dw [nStokes, nSpec, P] (host). */
int mom_scene_set_partials(mom_t *h, int P, const double *dtau, const double *dvarpi, const double *dzw, const double *dZpp,
                           const double *dZmp, const double *dalbedo, const double *dRsurf, const double *dalbedo_spec);
int mom_rt_run_dual(mom_t *h);
int mom_get_RT_partials(mom_t *h, double *dR_SFI, double *dT_SFI);
int mom_get_hdr_partials(mom_t *h, double *dhdr, double *dbhr_uw, double *dbhr_dw);
/* ---- The Dual run of the device-side layer optics: the scene's partials formed ON THE DEVICE ------------------------
 * The reference gets dτ, dϖ and the partials of the basis weights by running constructCoreOpticalProperties / createAero
 * (compEffectiveLayerProperties.jl:1-85) and the `+` of types.jl:632-678 on ForwardDiff.Dual element types.  This is that run
 * for a scene that came from mom_scene_set_optics: k_optics_dual (csrc/mom_optics.hip) follows k_optics statement by statement
 * with the product and quotient rules -- the Rayleigh start, each aerosol's `+` with its three cases (types.jl:641-661, decided
 * on the values like every boolean), the gas term (types.jl:672-678) -- and writes dtau, dvarpi [S, Nz, P] and dzw [K, S, Nz, P]
 * straight into the buffers mom_rt_run_dual reads.  Lines -> Dual line shape (mom_voigt_tau_abs_profile_dual,
 * mom_lut_tau_abs_profile_dual) -> Dual layer optics -> mom_rt_run_dual is then one device pipeline: neither dtau_abs nor the
 * scene's partials cross the bus.  Float64 handles.
 *
 * mom_scene_set_optics_partials   mom_scene_set_partials for such a scene, from the partials of the INGREDIENTS.  All layouts have
 *                          the partial index as the SLOWEST axis; every array may be NULL (no dependence):
 *                            w_abs [Nz, 3, P]   chain weights onto the resident absorption tables,
 *                                 dτ_abs[s,z,k] = dtau_abs[s,z,0] w[z,0,k] + dtau_abs[s,z,1] w[z,1,k] + tau_abs[s,z] w[z,2,k]:
 *                                 rows 0 and 1 are ∂p_z/∂x_k and ∂T_z/∂x_k (each layer's τ_abs depends on its own p and T only),
 *                                 row 2 is the relative change of the layer's gas column, ∂ln(vcd vmr)_z/∂x_k, which needs no Dual
 *                                 absorption call.  A nonzero row-0/1 weight without a resident dtau_abs table: MOM_ESTATE.
 *                            w_rayl [Nz, P]     dτ_rayl[s,z,k] = tau_rayl[s,z] w_rayl[z,k]: the Rayleigh depth of a layer is a
 *                                 spectral factor times the layer's column (atmo_prof.jl:210-224), so any parameter acts on it as a
 *                                 per-layer relative change.  ϖ_Cabannes carries no partial.
 *                            dtau_aer [nAer, Nz, P], domega_aer, dft_aer [nAer, P]   the partials of mom_scene_set_optics'
 *                                 arguments; createAero on Duals (compEffectiveLayerProperties.jl:80-85) is O(nAer Nz P) host work
 *                                 like its value form (mom_scene_set_optics keeps host copies of the three for it).
 *                            dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec   as in mom_scene_set_partials, by the same code.
 *                          dzw exists only when nAer > 0 and one of w_rayl, dtau_aer, domega_aer, dft_aer is given (otherwise it
 *                          is identically zero and the sweep keeps skipping it).  P = 0 clears the partials.  0 <= P <= 64.
 *                          MOM_ESTATE without a resident scene, for a scene that came from mom_scene_set (host optics), and when
 *                          mom_absorption_begin / mom_absorption_set was called after the mom_scene_set_optics that made the scene
 *                          (the tables are no longer the scene's).  mom_timers right after the call reports the HIP-event time
 *                          of the kernel as its total.
 * mom_scene_get_partials   the resident dtau, dvarpi [S, Nz, P] and dzw [K, S, Nz, P] to the host, whichever of the two setters
 *                          produced them (test access).  NULL skips an array; an absent device buffer reads as zeros; without
 *                          partials (P = 0 or never set): MOM_ESTATE. */
int mom_scene_set_optics_partials(mom_t *h, int P, const double *w_abs, const double *w_rayl, const double *dtau_aer,
                                  const double *domega_aer, const double *dft_aer, const double *dZpp, const double *dZmp,
                                  const double *dalbedo, const double *dRsurf, const double *dalbedo_spec);
int mom_scene_get_partials(mom_t *h, double *dtau, double *dvarpi, double *dzw);
/* mom_scene_set_optics_partials for a scene that came from mom_scene_set_optics_bands: constructCoreOpticalProperties' loop over
 * iBand (compEffectiveLayerProperties.jl:24-75) on ForwardDiff.Dual element types.  The aerosol partials carry a band axis:
 * dtau_aer [nAer, Nz, nBand, P], domega_aer, dft_aer [nAer, nBand, P]; a parameter of one band's aerosol has zeros in the other
 * bands, and so has its dR_SFI / dT_SFI on their points.  dZpp, dZmp [N, N, K, M, P], K = 1 + nAer nBand.  dzw [K, S, Nz, P]
 * exists under the conditions of mom_scene_set_optics_partials, exact zeros outside a point's own band.  The MOM_ESTATE rules
 * are those of mom_scene_set_optics_partials; a scene without bands here, or a band-resolved scene there, is MOM_ESTATE too.
 * Float64 handles. */
int mom_scene_set_optics_bands_partials(mom_t *h, int P, const double *w_abs, const double *w_rayl, const double *dtau_aer,
                                        const double *domega_aer, const double *dft_aer, const double *dZpp, const double *dZmp,
                                        const double *dalbedo, const double *dRsurf, const double *dalbedo_spec);

/* rt_run_test_ms(RS_type::noRS, sensor_levels, model, iBand) (src/CoreRT/rt_run_multisensor.jl:14-191) for the resident
 * scene: sensors inside the atmosphere.  sensor_levels[ims] = 0 is the TOA/BOA pair (uwJ = R_SFI, dwJ = T_SFI of
 * mom_rt_run); L in 1..Nz-1 puts the sensor below layer L counted from the top: rt_kernel_multisensor!
 * (rt_kernel_multisensor.jl:2-113) builds the composite of layers 1..L ("top") and of layers L+1..Nz plus the surface
 * ("bot"), interlayer_flux_helper! (CoreKernel/interlayer_flux.jl:7-24) solves for the fields at the interface,
 *   dwJ = (I - topR+- botR-+)^-1 (topJ0+ + topR+- botJ0-),  uwJ = (I - botR-+ topR+-)^-1 (botJ0- + botR-+ topJ0+),
 * and postprocessing_vza_ms! (tools/postprocessing_vza_ms.jl:9-77) weights them azimuthally.
 * uwJ, dwJ: host [nVza, nStokes, nSpec, nSensors] (the reference's vector-of-arrays, sensor-major).  Synchronous.
 * Float64, noRS; the hdr / bhr outputs of mom_get_hdr are not defined after this call. */
int mom_rt_run_multisensor(mom_t *h, int nSensors, const int *sensor_levels, double *uwJ, double *dwJ);

/* R_SFI, T_SFI [nVza, nStokes, S] to host (synchronises). */
int mom_get_RT(mom_t *h, double *R_SFI, double *T_SFI);
/* The RAMI extras of rt_run's return tuple (rt_run.jl:226): hdr [nVza, nStokes, S] from
 * interaction_hdrf! (CoreKernel/interaction_hdrf.jl:9-45) + postprocessing_vza_hdrf!
 * (postprocessing_vza.jl:63-93), and the up-/down-welling flux sums bhr_uw, bhr_dw [nStokes, S]
 * (the reference returns their first rows). */
int mom_get_hdr(mom_t *h, double *hdr, double *bhr_uw, double *bhr_dw);
/* Same, into caller-owned DEVICE buffers (asynchronous on the handle's stream; errors surface at the next
 * synchronising call). */
int mom_get_RT_device(mom_t *h, void *dR_SFI, void *dT_SFI);

/* ---- multi-GPU: one process per GPU, spectral shards, ONE RCCL all-gather ----------
 * The reference has no multi-GPU path; a sharded host (Julia Distributed/MPI.jl ranks, or this repository's
 * bench.py) gives every rank a contiguous slice of the spectral axis with the GLOBAL ndoubl / interface codes
 * (rt_kernel.jl:241-242 takes maxima over the whole axis) and gathers the spectra once at the end.
 *   mom_comm_unique_id   rank 0 obtains the RCCL id (MOM_COMM_ID_BYTES bytes) and hands it to the other ranks
 *                        by whatever means the host has (MPI_Bcast, a TCP store, a file)
 *   mom_comm_init        ncclCommInitRank on the handle's GPU; librccl.so.1 is loaded on first use
 *   mom_allgather        count doubles per rank, device pointers, asynchronous on the handle's stream
 *   mom_allgather_RT_device  the handle's R_SFI || T_SFI block (2*nVza*nStokes*S_loc doubles) of every rank into
 *                        d_global [nranks][2][nVza*nStokes*S_loc]; asynchronous
 *   mom_allgather_RT     the same into host arrays R_SFI, T_SFI [nVza, nStokes, nranks*S_loc] (rank-major
 *                        spectral axis: every rank must run the same S_loc, pad the tail); synchronises */
enum { MOM_COMM_ID_BYTES = 128 };
int mom_comm_unique_id(void *id_out, size_t bytes);
int mom_comm_init(mom_t *h, int rank, int nranks, const void *nccl_id);
int mom_comm_destroy(mom_t *h);
int mom_allgather(mom_t *h, const void *d_local, void *d_global, size_t count);
int mom_allgather_RT_device(mom_t *h, void *d_global);
int mom_allgather_RT(mom_t *h, double *R_SFI_global, double *T_SFI_global);

/* Per-stage GPU time of the last mom_rt_run in milliseconds (hipEvent based):
 * ms[0] = layer kernels, ms[1] = surface, ms[2] = post-processing, ms[3] = total;
 * with n >= 8 also ms[4] = sum over the full-problem layer launches (k_layer of namespace mom, or the
 * only layer kernel when the m = 0 reduction is off), ms[5] = sum over the reduced m = 0 launches,
 * ms[6], ms[7] = their launch counts.  kernel_launches = number of layer-kernel launches.  Synchronises. */
int mom_timers(mom_t *h, double *ms, int n, int *kernel_launches);

/* Tuning / test knobs (call before mom_scene_set):
 *   MOM_OPT_INVERSE       0 = automatic (default), 1 = force the pivoted Gauss-Jordan inverse, 2 = automatic
 *                         without the strip-chained kernels' register-resident chains (A/B testing)
 *   MOM_OPT_FORCE_GENERIC 1 = use the generic (global-memory) kernels even when the LDS-resident ones apply
 *   MOM_OPT_M0_REDUCTION  1 (default) = run Fourier moment 0 on the (I,Q) sub-problem when the scene allows
 *                         it (see mom_scene_set), 0 = always the full nStokes problem
 *   MOM_OPT_SMALL_WG      1 (default) = operators small enough for two LDS images per CU run in 4-wave
 *                         workgroups, two per CU; 0 = always 8-wave workgroups
 *   MOM_OPT_STAGGER       1 (default) = the persistent one-per-CU workgroups of the strip-chained kernels start
 *                         with offsets spread over one unit time, so that the CUs' composite loads/stores do
 *                         not all fall into the same microseconds; 0 = all start together
 *   MOM_OPT_SMALL_N       1 (default) = operators of edge N <= 4 (with at most 4 view angles and 4 phase-matrix bases)
 *                         run the lane-per-spectral-point sweep kernel: the whole of mom_rt_run in one launch, all
 *                         operators in registers (csrc/mom_small.hip); edges 4 < N <= 32 (scattering in every layer after the
 *                         first, at most 256 view x Stokes outputs) the wave-per-spectral-point sweep kernel
 *                         (csrc/mom_wave.hip), with 3 (N = 5) or 2 (N = 6..8) spectral points per wavefront as diagonal
 *                         blocks of one MFMA tile; 2 = the same kernels with one point per wavefront throughout;
 *                         0 = the general workgroup-per-point kernels
 *   MOM_OPT_LAYER_SWEEP   1 (default) = one launch per problem size walks ALL layers of a (spectral point, moment)
 *                         unit before the next unit: the composite blocks stay in the storing CU's L2 between layers,
 *                         one tail per sweep instead of one per layer (needs one interface code for all layers >= 2,
 *                         else falls back); 0 = one launch per layer (per-layer timing for profiling)
 *   MOM_OPT_STRIP_PAD     1 (default) = an operator edge N (or the m = 0 sub-problem's) without a strip-chained kernel
 *                         image is padded with up to 4 decoupled dummy stream entries (mu = 1, weight 0, zero
 *                         phase-matrix rows and columns) when that reaches a size with one (36, 40, 44, 52, 56, 60);
 *                         results for the real streams are unchanged; 0 = run the edge as given
 *   MOM_OPT_LEAN          operators of edge 36 / 40 (Float64, layer-sweep mode, ScatteringInterface_11 after the first layer; the
 *                         m = 0 (I,Q) sub-problem of a 20-stream IQU scene is one): which image runs them before the full image
 *                         finishes whatever it left (series beyond 12 terms) -- TWO launches per sweep, both counted in mom_timers'
 *                         kernel_launches.  3 (default, r6) = the QUAD-BLOCK image: one wavefront per unit, products on
 *                         v_mfma_f64_4x4x4 (no padding at N = 40, no idle SIMD), four units per CU (csrc/mom_q4.hpp); needs two or
 *                         more Stokes components per stream, else falls to 1; 1 = the four-wave LEAN strip image (three operator
 *                         buffers, 168 registers: three workgroups per CU; bitwise the full image's strip path); 2 = the six-wave lean
 *                         image (doubling chains on half-strips: an experiment, measured slower); 0 = the full image only.
 *   MOM_OPT_OVERLAP       1 (default) = when Fourier moment 0 runs on the (I,Q) sub-problem (MOM_OPT_M0_REDUCTION) in layer-sweep
 *                         mode AND the full problem runs on a one-workgroup-per-CU strip image (operator edge 52, 56, 60: the two
 *                         kernels then cannot share a CU; where they can, overlapping them measured slower), its launches and its surface interaction go to a second, high-priority stream of the handle and
 *                         overlap the launch of moments 1..M-1: the partial last round of the persistent workgroups of either
 *                         launch is filled by the other; results are unchanged (the launches are independent); mom_timers then
 *                         reports overlapping intervals for the two.  0 = everything on the handle's one stream.
 *   MOM_OPT_RRS_KERNELS   kernel forms of the rotational-Raman path, a mask (default 15; every form executes the same products in
 *                         the same order, results agree to 1e-13): 1 = one workgroup per (n1, dn) pair above N = 16 (else one
 *                         wavefront per pair), 2 = ... also for 16 < N <= 32, 4 = one workgroup per spectral point above N = 16 for
 *                         the per-point operands (Gauss-Jordan inverse over all waves), 8 = the inelastic elemental layer as a tile
 *                         kernel, 16 / 32 = form it inside the first doubling step always / never (neither: above N = 48 only).
 *                         (r5 read these from environment variables, once per process.)
 *   MOM_OPT_DUAL_WORKSPACE_MB   operator workspace of mom_rt_run_dual in MiB (0, default: 60 % of the free HBM when the run
 *                         starts); a scene that needs more is processed in chunks of spectral points.
 *   MOM_OPT_STRIP2        operators of edge 52 / 56 / 60 (Float64, layer-sweep mode, ScatteringInterface_11 after the first layer,
 *                         stream-pair tables that fit the front of one operator buffer): 1 (default) = the TWO-BUFFER 4-wave strip
 *                         image runs them first, two workgroups per CU (csrc/mom_strip2.hpp), and the 8-wave image finishes
 *                         whatever it left (series beyond 12 terms) -- two launches per sweep, both counted in mom_timers'
 *                         kernel_launches; results are bitwise those of the 8-wave image.  0 = the 8-wave image only.
 *   MOM_OPT_STRIP2_SCHED  how the two workgroups of a CU share it in the two-buffer image, a mask (default 1): 1 = the units come from
 *                         a shared queue (an atomic ticket per unit; the counter is zeroed on the stream before the launch)
 *                         instead of a fixed stride per workgroup, 2 = the workgroup that arrives second on its CU runs its strip
 *                         chains at raised wave priority (an experiment: the two units do not run in lock-step to begin with, and the
 *                         priority measured 1.6 ms slower on C2 on top of the queue, profiles/r08_C2_ab.txt).  0 = neither (the
 *                         scheduling before this option existed).  Results do not depend on it: units are independent.
 *   MOM_OPT_ZERO_SKIP     a mask (default 7) of the images whose products leave out what is an exact zero because of the zero-weight
 *                         streams at the end of the stream set (the view angles, the Sun, dummy entries): the driver counts the
 *                         trailing weights that are exactly 0.0, and the first nbw = ceil((N - count) / 4) blocks of four entries
 *                         hold the weighted ones.  Bit 0 = the quad-block image (operator edges 20 .. 40, csrc/mom_q4.hpp) leaves
 *                         out the zero blocks: a launch takes the kernel compiled for nbw (or the next larger number it has: 0, 1,
 *                         2 or 4 blocks left out).  Bit 1 = the two-buffer strip image (edges 52 / 56 / 60, csrc/mom_strip2.hpp)
 *                         leaves out the last KS - nbw k-steps of every strip product (0 .. 3 of them, the largest number it has
 *                         that is still exact) and adds the diagonal entries of those columns by a fused multiply-add.  Bit 2 =
 *                         the two-buffer strip image's row-block rule: a 16-row tile of a strip product in which only some blocks
 *                         of four rows are live (rows of weighted entries, the riding source rows) runs one 4 x 4 x 4 matrix
 *                         instruction per live block instead of the 16 x 16 x 4 one; the rows of the zero-weight streams get
 *                         their one term from the fused multiply-add of bit 1, the rows past the riding rows are not computed.
 *                         Without bit 1 it covers only the latter (edges 52 and 56).  A bit that is off = the kernel that
 *                         multiplies everything.  The terms left out are exact zeros: stored values, series lengths and resume
 *                         decisions do not depend on the option (at most the sign of a zero does).
 *   MOM_OPT_LUT_BATCH     (p, T) nodes that mom_lut_build fills per pair of launches (default 0 = 64): the per-line prefactor block
 *                         of a batch takes nodes x lines.  Nodes are independent: the table does not depend on it by a bit.
 *   MOM_OPT_SOURCES_ONLY  1 (default) = a sweep launch of mom_rt_run that holds no observable Fourier moment leaves the composite
 *                         operators R-+ and T++ out of its layers.  Such a launch is the (I,Q) sub-problem's (moment 0 under
 *                         MOM_OPT_M0_REDUCTION: mom_download answers MOM_ESTATE for it) or a full-problem launch that starts at
 *                         moment 1 or later (mom_download returns moment 0 only); and the rule exists in the two-buffer strip image
 *                         (edges 52 / 56 / 60, csrc/mom_strip2.hpp) and the quad-block image (csrc/mom_q4.hpp) alone.  R-+ and T++
 *                         feed nothing but themselves: the sources J0-, J0+ -- all that R, T, hdr and the BHRs are formed from --
 *                         take from the two products one row each, J0+^T (T01 r-+)^T and J0+^T T21^T, which the launch forms on its
 *                         own with the same matrix instructions in the same order.  After such a launch the two arrays hold the
 *                         FIRST layer's r-+ and t++ (finite, rewritten by every run, meaningless); a unit that the 8-wave image
 *                         finishes, and the surface kernel, go on updating the two operators from there, and nothing of them reaches
 *                         a source, a series length or a resume decision.  mom_rt_run_multisensor, the Dual and RRS runs, the
 *                         operator-level calls, the finishers, the surface kernel, the other images and the Float32 handles never
 *                         take this form; with MOM_OPT_M0_REDUCTION = 0 the one launch carries moment 0 and keeps all four
 *                         operators.  0 = every launch updates all four.  No output and no return value depends on the option.
 *   MOM_OPT_ELEMENTAL     1 (default) = the two-buffer strip image (edges 52 / 56 / 60, default scheduling mode) and the quad-block
 *                         image build the elemental layer in its table form (csrc/mom_elemental_tab.hpp).  The layer-independent
 *                         stream-pair tables 1/mu_i + 1/mu_j, mu_j/(mu_i + mu_j), mu_j/(mu_i - mu_j) are computed once per scene on
 *                         the device (mom_scene_set and its kin) instead of once per layer and unit; a layer evaluates only
 *                         1 - exp(-dtau (1/mu_i + 1/mu_j)), on the pairs i <= j; the elements are formed in batches of four, all
 *                         operands requested together, every alternative computed with the expressions of the other form and picked
 *                         by select.  It applies to regular streams, two phase-matrix bases and an edge of whole streams; any other
 *                         launch of the two images, every other image, the finishers, the Float32 handles, the multisensor, Dual,
 *                         RRS and operator-level paths build the layer as before.  0 = the other form everywhere: the kernels of the
 *                         library without the option.  Every output is bit for bit the same under both values.
 */
int mom_set_option(mom_t *h, int option, int value);

/* The two-buffer strip image's last launch on this handle (MOM_OPT_STRIP2): *units = the units it was given, *left = how many of
 * them it handed to the 8-wave image through the resume table (a series beyond 12 terms).  0, 0 if it never ran.  Synchronises.
 * A test observable: results do not depend on it. */
int mom_strip2_resumed(mom_t *h, int *units, int *left);
enum { MOM_OPT_INVERSE = 0, MOM_OPT_FORCE_GENERIC = 1, MOM_OPT_M0_REDUCTION = 2, MOM_OPT_SMALL_WG = 3, MOM_OPT_STAGGER = 4,
       MOM_OPT_SMALL_N = 5, MOM_OPT_LAYER_SWEEP = 6, MOM_OPT_STRIP_PAD = 7, MOM_OPT_LEAN = 8, MOM_OPT_OVERLAP = 9,
       MOM_OPT_RRS_KERNELS = 10, MOM_OPT_DUAL_WORKSPACE_MB = 11, MOM_OPT_STRIP2 = 12, MOM_OPT_STRIP2_SCHED = 13,
       MOM_OPT_ZERO_SKIP = 14, MOM_OPT_LUT_BATCH = 15, MOM_OPT_SOURCES_ONLY = 16, MOM_OPT_ELEMENTAL = 17 };

/* ---- The InterpolationModel: cross sections computed once on a (nu, p, T) grid and kept on the device as a cubic B-spline
 * interpolant -- make_interpolation_model (make_model_helpers.jl:55-99) and compute_absorption_cross_section(model::InterpolationModel,
 * grid, p, T) (compute_absorption_cross_section.jl:139-159): Interpolations.jl's interpolate(A, BSpline(Cubic(Line(OnGrid()))))
 * scaled to the model's three ranges (first, step, length).  Per axis of n nodes the interpolant has n + 2 coefficients c_0 .. c_{n+1}
 * with (c_{i-1} + 4 c_i + c_{i+1}) / 6 = f_i at the nodes and zero second derivative at the first and the last node (the natural cubic
 * spline).  A point is evaluated at x = (value - first) / step + 1 -- one subtraction, one division --, i = clamp(floor(x), 1, n - 1),
 * delta = x - i, with the cubic B-spline weights of c_{i-1} .. c_{i+2}; the 3-D value is the tensor product.  There is no
 * extrapolation: a nu, p or T outside [first, last] of its axis is MOM_EINVAL, with a text that names the axis, the value and the
 * range; the end points are inside.  A table belongs to the handle, is named by a small integer id and is Float64 on every handle;
 * any number of tables live at once (one per absorber).  Not built: the ABSCO method of make_interpolation_model (:112-), whose
 * interpolant is mixed linear / quadratic -- a table derived from ABSCO on the host goes through mom_lut_set_table --, and
 * wavelength_flag.
 *   mom_lut_create         an empty table on the three ranges; an axis of fewer than 3 nodes or a step <= 0: MOM_EINVAL.  *lut = its id
 *   mom_lut_set_table      takes sigma [nNu, nP, nT] (nu fastest: the reference's cs_matrix) from the host and prefilters it on
 *                          the device: the route of a model loaded from disk
 *   mom_lut_build          make_model_helpers.jl:82-91 on the device: sigma at every node (p_i, T_j) from the resident line table
 *                          (mom_absorption_set_lines, selected against the model's nu grid) under the handle's absorption model
 *                          (mom_absorption_set_model), by the kernels of mom_voigt_tau_abs_profile with the nodes as layers and
 *                          factor 1 -- column (i, j) of the table is bitwise what that call adds to a zeroed tau_abs[:, z] --, then the
 *                          prefilter.  The nodes run in batches (MOM_OPT_LUT_BATCH).  The handle's tau_abs, dtau_abs and spectral grid
 *                          are not touched.  Errors as mom_voigt_tau_abs_profile (the TIPS-2017 range of the T axis included).
 *                          gpu_ms: NULL or two doubles, the HIP-event times of the fill and of the prefilter.
 *   mom_lut_get_table, mom_lut_get_coefficients   test access: sigma [nNu, nP, nT] and the coefficients [nNu + 2, nP + 2, nT + 2]
 *   mom_lut_xsec           sigma [n] at the points nu [n] (any values inside the nu range, in any order) and one (p, T).  J: NULL, or
 *                          [n, 2] column-major like mom_voigt_xsec_dual's dsigma -- the Jacobian with respect to (p, T) of
 *                          absorption_cross_section(...; autodiff = true) (autodiff_helper.jl:17-51): ForwardDiff through the weights,
 *                          floor and clamp taken on the values.  sigma does not depend on whether J is asked for (bitwise).
 *   mom_lut_tau_abs_profile        tau_abs[:, z] += sigma_lut(grid; p[z], T[z]) * factor[z] for layers 1..Nz on the grid of
 *                          mom_absorption_begin, all layers in one launch; accumulating like mom_voigt_tau_abs_profile, so it adds
 *                          to whatever absorbers the table holds already, line-by-line or interpolated.
 *   mom_lut_tau_abs_profile_dual   the same, and adds d_k sigma * factor into dtau_abs[:, z, k] (mom_absorption_get_partials): the
 *                          table is allocated and zeroed by the first Dual call after mom_absorption_begin, and a value call counts
 *                          as an absorber with zero partials.
 *   mom_lut_destroy        frees the table; its id may be handed out again.
 * A wrong or destroyed id: MOM_EINVAL.  Evaluating a table that has no coefficients yet: MOM_ESTATE.  A profile call without
 * mom_absorption_begin (with the grid): MOM_ESTATE. */
int mom_lut_create(mom_t *h, int nNu, double nu_first, double nu_step, int nP, double p_first, double p_step, int nT, double t_first,
                   double t_step, int *lut);
int mom_lut_set_table(mom_t *h, int lut, const double *sigma);
int mom_lut_build(mom_t *h, int lut, double vmr, double wing_cutoff, double *gpu_ms);
int mom_lut_get_table(mom_t *h, int lut, double *sigma);
int mom_lut_get_coefficients(mom_t *h, int lut, double *c);
int mom_lut_xsec(mom_t *h, int lut, int n, const double *nu, double p, double T, double *sigma, double *J);
int mom_lut_tau_abs_profile(mom_t *h, int lut, int Nz, const double *pressure, const double *temperature, const double *factor,
                            double *gpu_ms);
int mom_lut_tau_abs_profile_dual(mom_t *h, int lut, int Nz, const double *pressure, const double *temperature, const double *factor,
                                 double *gpu_ms);
int mom_lut_destroy(mom_t *h, int lut);

/* ---- Voigt line-by-line cross section --------------------------------------------------
 * compute_absorption_cross_section(model::HitranModel, grid, p, T)
 * (compute_absorption_cross_section.jl:19-130) with Voigt broadening and the
 * HumlicekWeidemann32SDErrorFunction (complex_error_functions.jl:226-234).  The host passes
 * the per-line prefactors of :79-107: nu = pressure-shifted centre, gamma_d, y, S =
 * temperature-corrected strength, and the 1-based inclusive grid window of each line.
 * sigma[nGrid] (host) receives sum over lines in line order.  `device` as in mom_create.
 * Error text: mom_last_global_error(). */
int mom_voigt_xsec(int device, int nLines, const double *nu, const double *gamma_d, const double *y,
                   const double *S, const int *ind_start_1based, const int *ind_stop_1based, int nGrid,
                   const double *grid, double *sigma);

/* The Dual run of mom_voigt_xsec: dnu, dgamma_d, dy, dS are the partials of the four prefactors with respect to pressure
 * (k = 0) and temperature (k = 1), each [nLines, 2] column-major (index j + nLines k; NULL = zeros).  sigma[nGrid] as above,
 * dsigma [nGrid, 2] column-major = the Jacobian absorption_cross_section(...; autodiff = true) returns as result.derivs[1]. */
int mom_voigt_xsec_dual(int device, int nLines, const double *nu, const double *gamma_d, const double *y, const double *S,
                        const double *dnu, const double *dgamma_d, const double *dy, const double *dS,
                        const int *ind_start_1based, const int *ind_stop_1based, int nGrid, const double *grid,
                        double *sigma, double *dsigma);

/* line_shape!(A, grid, nu, gamma_d, gamma_l, y, S, broadening, CEF) (compute_absorption_cross_section.jl:167-183) summed over
 * the lines in line order: mom_voigt_xsec for any absorption model (MOM_BROADENING_*, MOM_CEF_*; see mom_absorption_set_model).
 * gamma_l = the Lorentz half width of :82-84.  An array the broadening does not read may be NULL; an unknown code: MOM_EINVAL.
 * With (MOM_BROADENING_VOIGT, MOM_CEF_HW32SD) the result is bitwise that of mom_voigt_xsec. */
int mom_lineshape_xsec(int device, int broadening, int cef, int nLines, const double *nu, const double *gamma_d,
                       const double *gamma_l, const double *y, const double *S, const int *ind_start_1based,
                       const int *ind_stop_1based, int nGrid, const double *grid, double *sigma);

/* The Dual run of mom_lineshape_xsec (ForwardDiff.Dual numbers through line_shape!, autodiff_helper.jl:17-51): the partials of
 * the five prefactors as for mom_voigt_xsec_dual, dsigma [nGrid, 2] column-major.  The branch |x| + y > 15 of
 * w(::HumlicekWeidemann32VoigtErrorFunction, z) (complex_error_functions.jl:210-219) is taken on the values. */
int mom_lineshape_xsec_dual(int device, int broadening, int cef, int nLines, const double *nu, const double *gamma_d,
                            const double *gamma_l, const double *y, const double *S, const double *dnu,
                            const double *dgamma_d, const double *dgamma_l, const double *dy, const double *dS,
                            const int *ind_start_1based, const int *ind_stop_1based, int nGrid, const double *grid,
                            double *sigma, double *dsigma);

/* GPU time (HIP events around the kernel, ms) of the last mom_voigt_xsec / mom_lineshape_xsec call (or Dual run) of the calling thread. */
double mom_voigt_last_kernel_ms(void);

/* ---- Mie aerosol optics: Siewert NAI-2 -------------------------------------------------------
 * compute_aerosol_optical_properties(model::MieModel{NAI2}) (src/Scattering/compute_NAI2.jl:16-182) for one wavelength and one
 * refractive index m = n_r + i n_i (n_i >= 0, the absorbing convention with xi = psi - i chi), Float64.  Handle-free like
 * mom_lineshape_xsec; error text: mom_last_global_error().  The host brings the quadratures and the tables:
 *   r [nR]                  radii, ascending, r[0] > 0, in the unit of lambda; size parameter x_i = (2 pi / lambda) r_i,
 *                           n_max,i = round(x_i + 4.05 x_i^(1/3) + 10), downward recurrence from round(max(n_max,i, |x_i (n_r - n_i)|) + 51)
 *   w [nW, nR]              weight rows (row-major, 1 <= nW <= 4): row 0 = 4 pi r^2 w_x for the value, further rows the same with
 *                           d w_x / d theta for a parameter of the size distribution (everything below is linear in w)
 *   w_mu [n_mu]             Gauss weights of the scattering-angle nodes
 *   pi_tab, tau_tab         pi_l(mu), tau_l(mu), l = 1..n_max: [n_max, n_mu], mu fastest (compute_mie_pi_tau, column-major [n_mu, n_max]);
 *                           n_max >= the largest n_max,i
 *   P, P2, R2, T2           compute_legendre_poly(mu, l_max): [l_max, n_mu], mu fastest
 * Outputs (host), none of them divided by the bulk C_sca (that and the quotient rule of the partial rows are host arithmetic):
 *   bulk_f [nW, 4, n_mu]    sum_i w[k, i] f(mu, i) for f = f11, f33, f12, f34 (compute_NAI2.jl:107-110, 119-123)
 *   C [nW, 2]               sum_i w[k, i] / (4 pi r_i^2) * (C_sca,i, C_ext,i) (:103-104, 115-116)
 *   greek [nW, 6, l_max]    the projections of :146-160 on bulk_f, in the order alpha, beta, gamma, delta, epsilon, zeta
 *   gpu_ms [3] or NULL      HIP-event times (ms): coefficient kernel, amplitude GEMM with its reduction, projection
 * The radii are tiled by 16 and a tile's sum over l ends at the tile's largest n_max,i rounded up to 4: only products with the
 * exact zeros above a radius' own n_max,i are left out.  flags = MOM_MIE_FULL_K runs every tile to n_max instead (test access:
 * the results are bitwise equal).  Two calls with the same arguments give bitwise equal results.
 * MOM_EINVAL: nR < 1, n_mu < 1, l_max < 1, nW outside 1..4, lambda <= 0, n_i < 0, r not ascending or r[0] <= 0, n_max smaller
 * than the largest n_max,i, an unknown flag, a null pointer (gpu_ms excepted). */
enum { MOM_MIE_MAX_WEIGHT_ROWS = 4, MOM_MIE_FULL_K = 1 };
int mom_mie_nai2(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                 int n_mu, const double *w_mu, int n_max, const double *pi_tab, const double *tau_tab, int l_max,
                 const double *P, const double *P2, const double *R2, const double *T2, int flags, double *bulk_f,
                 double *C, double *greek, double *gpu_ms);

/* Test access: the Mie coefficients a_n, b_n (compute_mie_ab!, mie_helper_functions.jl:31-71) of nX size parameters x > 0 (any
 * order), n = 1..n_max, as four real arrays [n_max, nX], x fastest; zeros above each x's own n_max.  MOM_EINVAL as above. */
int mom_mie_coefficients(int device, int nX, const double *x, double n_r, double n_i, int n_max, double *a_re, double *a_im,
                         double *b_re, double *b_im);

/* The Dual run of mom_mie_nai2 with respect to the refractive index (phase_function_autodiff.jl:41-95, the columns n_r and n_i of
 * x = (r_m, sigma_g, n_r, n_i)): same arguments, 1 <= nW <= 3, and nW + 2 output rows,
 *   bulk_f [nW + 2, 4, n_mu], C [nW + 2, 2], greek [nW + 2, 6, l_max].
 * Rows 0 .. nW - 1 are bitwise what mom_mie_nai2 writes for the same arguments; row nW is d/dn_r and row nW + 1 is d/dn_i of row
 * 0's sums.  a_n and b_n are holomorphic in m = n_r + i n_i, so the coefficient kernel carries ONE complex derivative d/dm
 * (d/dn_r = d/dm, d/dn_i = i d/dm) through both recurrences; n_max,i and the start of the downward recurrence are integers and
 * are taken on the values, as ForwardDiff's round(Int, .) does.  gpu_ms and flags as for mom_mie_nai2; two calls are bitwise equal.
 * MOM_EINVAL: the list of mom_mie_nai2 with nW outside 1..3. */
enum { MOM_MIE_DUAL_MAX_WEIGHT_ROWS = 3, MOM_MIE_INDEX_ROWS = 2 };
int mom_mie_nai2_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                      int n_mu, const double *w_mu, int n_max, const double *pi_tab, const double *tau_tab, int l_max,
                      const double *P, const double *P2, const double *R2, const double *T2, int flags, double *bulk_f,
                      double *C, double *greek, double *gpu_ms);

/* Test access: mom_mie_coefficients and da_n / dm, db_n / dm as four more real arrays [n_max, nX] (d/dn_r = d/dm, d/dn_i = i d/dm);
 * a and b are bitwise those of mom_mie_coefficients.  MOM_EINVAL as there; no pointer may be null. */
int mom_mie_coefficients_dual(int device, int nX, const double *x, double n_r, double n_i, int n_max, double *a_re, double *a_im,
                              double *b_re, double *b_im, double *da_re, double *da_im, double *db_re, double *db_im);

/* The angle tables of mom_mie_nai2 built on the device from the nodes mu [n_mu], one lane per mu, serial over the order:
 *   pi_tab, tau_tab         [n_max, n_mu], mu fastest (compute_mie_pi_tau)
 *   P, P2, R2, T2           [l_max, n_mu], mu fastest (compute_legendre_poly)
 * The kernel performs the statements of the host's recurrences in their order, without contraction: the tables are bitwise those
 * the host builds.  Test access, and of use on its own.  MOM_EINVAL: n_mu, n_max or l_max < 1, a null pointer. */
int mom_mie_tables(int device, int n_mu, const double *mu, int n_max, int l_max, double *pi_tab, double *tau_tab, double *P,
                   double *P2, double *R2, double *T2);

/* mom_mie_nai2 for a batch of nL wavelengths lambda [nL], each with its own refractive index n_r [nL] + i n_i [nL], in one call.
 * Radii and weight rows are shared (w = 4 pi r^2 w_x does not depend on lambda), and so is ONE angle grid mu, w_mu [n_mu], which
 * the caller sizes for the shortest wavelength; the tables are built on the device from mu (mom_mie_tables), none is uploaded.
 * n_max is the row count of the pi / tau tables, at least the largest per-radius n_max,i over all wavelengths: a longer
 * wavelength runs with spare table rows.  Outputs, wavelength slowest:
 *   bulk_f [nL, nW, 4, n_mu], C [nL, nW, 2], greek [nL, nW, 6, l_max]
 *   gpu_ms [4] or NULL      HIP-event times (ms): tables, coefficient kernel, amplitude GEMM with its reduction, projection
 * The wavelength is one more grid dimension of the kernels of mom_mie_nai2, and each wavelength keeps the single call's radius
 * chunks, tile walk and reduction order: its rows are bitwise those of mom_mie_nai2 on the same grid and tables, whatever else is
 * in the batch.  max_batch = 0 runs sub-batches of consecutive wavelengths sized to a workspace of 2 GiB; max_batch > 0 caps the
 * sub-batch (test access).  flags as for mom_mie_nai2.
 * MOM_EINVAL: the list of mom_mie_nai2, per wavelength (the message names the wavelength's index), and nL < 1, max_batch < 0. */
int mom_mie_nai2_spectral(int device, int nR, const double *r, int nW, const double *w, int nL, const double *lambda,
                          const double *n_r, const double *n_i, int n_mu, const double *mu, const double *w_mu, int n_max,
                          int l_max, int flags, int max_batch, double *bulk_f, double *C, double *greek, double *gpu_ms);

/* The Dual run of mom_mie_nai2_spectral: 1 <= nW <= 3 and nO = nW + 2 rows per wavelength, the last two d/dn_r and d/dn_i of row
 * 0's sums as in mom_mie_nai2_dual: bulk_f [nL, nO, 4, n_mu], C [nL, nO, 2], greek [nL, nO, 6, l_max]. */
int mom_mie_nai2_spectral_dual(int device, int nR, const double *r, int nW, const double *w, int nL, const double *lambda,
                               const double *n_r, const double *n_i, int n_mu, const double *mu, const double *w_mu, int n_max,
                               int l_max, int flags, int max_batch, double *bulk_f, double *C, double *greek, double *gpu_ms);

/* ---- Mie aerosol optics: Domke-PCW -------------------------------------------------------------
 * compute_aerosol_optical_properties(model::MieModel{PCW}) (src/Scattering/compute_PCW.jl:16-193; Sanghavi 2014, eq. 22-24): the
 * Greek coefficients expanded directly in the Mie coefficients, with Wigner 3j symbols and no scattering-angle quadrature; the
 * independent check of mom_mie_nai2.  Float64, handle-free, error text: mom_last_global_error().  The reference reads the symbols
 * from two tables it loads (compute_wigner_values); here they are produced in registers by the recursions of
 * compute_wigner_values.jl and no table exists.
 *   r [nR], lambda, n_r, n_i as for mom_mie_nai2
 *   w [nR]                  w_x, the weights of the size distribution themselves (NOT times 4 pi r^2)
 *   N_max                   get_n_max(2 pi r_max / lambda), at least the largest n_max,i; 1 <= N_max <= MOM_PCW_MAX_ORDER
 *   flags                   0
 * Outputs (host):
 *   greek [6, 2 N_max - 1]  alpha, beta, gamma, delta, epsilon, zeta of compute_PCW.jl:86-100, NOT divided by C_sca (host arithmetic)
 *   C [2]                   compute_avg_C_scatt_ext: C_sca, C_ext
 *   gpu_ms [3] or NULL      HIP-event times (ms): coefficient kernel, radius averages, symbols and sums
 * The pair averages of compute_avg_anbns! are one symmetric product X~ diag(w) X~^T on v_mfma_f64_16x16x4, X = [Re a; Im a; Re b;
 * Im b]; as in the reference a radius enters a pair average only for orders below its own n_max,i (strict), and keeps order
 * n_max,i in C_sca, C_ext and the sums of |a_n +- b_n|^2.  Every reduction has a fixed order: two calls are bitwise equal.
 * MOM_EINVAL: nR < 1, lambda <= 0, n_i < 0, r not ascending or r[0] <= 0, N_max outside 1..MOM_PCW_MAX_ORDER or smaller than the
 * largest n_max,i, flags != 0, a null pointer (gpu_ms excepted). */
enum { MOM_PCW_MAX_ORDER = 640 };
int mom_mie_pcw(int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N_max, int flags,
                double *greek, double *C, double *gpu_ms);

/* compute_wigner_values(m_max, n_max, l_max) (compute_wigner_values.jl:190-210): wigner_A = (m n l-1; -1 1 0) and wigner_B =
 * (m n l-1; -1 -1 2) as two tables [l_max, n_max, m_max] with m fastest (the reference's column-major [m_max, n_max, l_max]),
 * entry (m - 1, n - 1, l - 1); exact zeros outside |n - (l - 1)| <= m <= n + l - 1 and, in wigner_B, for l - 1 < 2.  One lane per
 * (n, l) column runs the device function mom_mie_pcw walks.  A column starts at m = n + l - 1 whatever m_max is, so a table keeps
 * the symbols' values where the reference's memoised recursion, which answers 0 beyond the table's extent, leaves zeros (columns
 * with n + l - 1 > m_max).  Two calls are bitwise equal.
 * MOM_EINVAL: a size < 1, n_max + l_max > 1900 (the recursion's 64-bit integer products), a table above
 * MOM_WIGNER_MAX_TABLE_BYTES (checked before any allocation), a null pointer. */
enum { MOM_WIGNER_MAX_TABLE_BYTES = 1073741824 };   /* 1 GiB */
int mom_wigner_tables(int device, int m_max, int n_max, int l_max, double *A, double *B);

/* Test access: the four pair averages of compute_avg_anbns! for the arguments of mom_mie_pcw, sum_i w_i conj(a_n) a_m, conj(a_n) b_m,
 * conj(b_n) a_m, conj(b_n) b_m, as eight real arrays [N_max, N_max], entry [m - 1][n - 1] for m >= n, zeros above the diagonal.
 * MOM_EINVAL as mom_mie_pcw; no pointer may be null. */
int mom_pcw_pair_averages(int device, int nR, const double *r, const double *w, double lambda, double n_r, double n_i, int N_max,
                          double *anam_re, double *anam_im, double *anbm_re, double *anbm_im, double *bnam_re, double *bnam_im,
                          double *bnbm_re, double *bnbm_im);

/* mom_mie_pcw with Jacobian rows: the partials of every sum with respect to (r_m, sigma_g, n_r, n_i), PCW's own second route to what
 * mom_mie_nai2_dual gives.
 *   w [nW, nR]              row-major, 1 <= nW <= MOM_PCW_MAX_WEIGHT_ROWS: row 0 is w_x, a further row is d w_x / d theta of a
 *                           size-distribution parameter (every sum is linear in w; a row may be negative)
 *   flags                   0 or MOM_PCW_INDEX_ROWS: two more output rows; nO = nW + 2 (flag set)
 * Outputs (host), everything else as for mom_mie_pcw:
 *   greek [nO, 6, 2 N_max - 1], C [nO, 2]
 * Row k < nW holds the sums of weight row k, bitwise what mom_mie_pcw writes when handed w[k], with or without the flag and whatever
 * else is in the call.  Row nW is d/dn_r and row nW + 1 is d/dn_i of row 0's sums: the coefficient kernel carries d/dm (as for
 * mom_mie_nai2_dual; n_max,i, the start of the downward recurrence and the strict mask of the pair averages are integers, taken on
 * the values), the sums over the radii that keep order n_max,i take one complex sum each, and the pair averages take ONE
 * non-symmetric product Y~ diag(w_0) X~^T on v_mfma_f64_16x16x4, Y = [Re a'; Im a'; Re b'; Im b'], from which both parameters follow
 * by a row map.  All nO rows share one walk over the Wigner symbols.  Two calls are bitwise equal.
 * MOM_EINVAL: the list of mom_mie_pcw, nW outside 1..3, a flag other than MOM_PCW_INDEX_ROWS. */
enum { MOM_PCW_MAX_WEIGHT_ROWS = 3, MOM_PCW_INDEX_ROWS = 1 /* flag */ };
int mom_mie_pcw_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r, double n_i,
                     int N_max, int flags, double *greek, double *C, double *gpu_ms);

/* Test access: mom_pcw_pair_averages for the arguments of mom_mie_pcw_dual: pairs [nO, 8, N_max, N_max], per row the eight arrays
 * in the order and entry convention of mom_pcw_pair_averages; rows nW and nW + 1 their partials.  MOM_EINVAL as mom_mie_pcw_dual. */
int mom_pcw_pair_averages_dual(int device, int nR, const double *r, int nW, const double *w, double lambda, double n_r,
                               double n_i, int N_max, int flags, double *pairs);

/* ---- Phase-matrix Fourier moments ---------------------------------------------------------------
 * Scattering.compute_Z_moments(mod, mu, greek_coefs, m) (src/Scattering/compute_Z_matrices.jl:5-84) for a batch of nG sets of Greek
 * coefficients and the Fourier moments m_first .. m_first + M - 1 in one call: the generalised spherical functions P, R, T of
 * compute_associated_legendre_PRT (legendre_functions.jl:17-178) at +mu and -mu for the requested m only, then
 * A++ = sum_l Pi_l(mu_i) B_l Pi_l(mu_j) and A-+ = sum_l Pi_l(mu_i) B_l Pi_l(-mu_j), l = m .. l_max - 1 (construct_Pi_matrix,
 * construct_B_matrix, mie_helper_functions.jl:287-348), as one product on v_mfma_f64_16x16x4 per (set, m, sign).  Float64,
 * handle-free like the mom_mie_* calls, error text: mom_last_global_error().  The moments are linear in the coefficients, so a
 * set may as well hold derivatives of coefficients (negative, all zero): the Z bases of a scene and those of its Jacobian are the
 * same call.
 *   nStokes                 1, 3 or 4; N = nStokes n_mu
 *   mu [n_mu]               quadrature nodes, every one in ]0, 1] (the reference's @assert); mu = 1 is an ordinary node
 *   l_max [nG]              length of each set, 1 <= l_max[g] <= l_pad; a set with l_max[g] <= m gives an all-zero matrix
 *   greek [l_pad, 6, nG]    l fastest, rows in the reference's order alpha, beta, gamma, delta, epsilon, zeta; entries at
 *                           l >= l_max[g] are not used
 *   set_inner               0 (or nG): the matrices of (set g, moment m) are stored as [N, N, nG, M], i fastest -- what mom_scene_set*
 *                           take as Zpp / Zmp with K = nG.  A divisor K of nG: the sets are read as g = k + K p and the matrices
 *                           are stored as [N, N, K, M, P], P = nG / K -- what mom_scene_set_partials takes as dZpp / dZmp; no
 *                           transpose is left to the host
 * Outputs (host):
 *   Zpp, Zmp                Z++ and Z-+ = 2 fact A, fact = 1/2 at m = 0 and 1 otherwise, Z-+ with the sign flipped on the blocks
 *                           (i <= 2, j >= 3) and (i >= 3, j <= 2) of the Stokes index
 *   gpu_ms or NULL          HIP-event time (ms) of the two kernels
 * P, R, T are bitwise the reference's (same statements, same association, no contraction); the sum over l runs in the MFMA's
 * k order with fused multiply-adds, so Z agrees with the host's to rounding, not bitwise.  Two calls are bitwise equal, and a
 * set's matrices do not depend on what else is in the batch or on the (m_first, M) window.
 * MOM_EINVAL, checked before the first HIP call: nStokes not 1, 3 or 4; n_mu, nG, M or l_pad < 1; m_first < 0; an l_max[g] outside
 * 1..l_pad; a mu outside ]0, 1]; set_inner negative or not a divisor of nG; a null pointer (gpu_ms excepted). */
int mom_z_moments(int device, int nStokes, int n_mu, const double *mu, int nG, int l_pad, const int *l_max, const double *greek,
                  int m_first, int M, int set_inner, double *Zpp, double *Zmp, double *gpu_ms);

/* ---- Scenes from Greek coefficients (Float64 handles) ----------------------------------------------
 * The Z bases of a scene formed in the handle's own memory: no N x N matrix crosses the bus.  The staging calls do no GPU work;
 * they check the arguments (mom_z_moments' checks, with the handle's nStokes and one mu per stream of mom_set_streams, each in
 * ]0, 1]) and copy them, so the caller's arrays are free when they return.  greek [l_pad, 6, nG] and l_max [nG] as in mom_z_moments.
 *   mom_scene_stage_greeks         which = 0: the nG = K phase-matrix bases, M moments, of the next mom_scene_set / _set_optics /
 *                                  _set_optics_bands; which = 1: the one Raman set (nG = 1) of the next mom_scene_set_rrs.
 *   mom_scene_stage_greek_partials nD derivative sets: set d is the partial of basis basis[d] (0-based) with respect to parameter
 *                                  partial[d] (0-based, < P); every other (basis, partial) block of dZpp / dZmp is exactly zero.  A
 *                                  pair named twice: MOM_EINVAL.  The moments are the scene's.
 * A setter called with Zpp == Zmp == NULL (mom_scene_set_rrs: Zpp_l1l0 == Zmp_l1l0 == NULL) takes the stage: K and M have to agree
 * with it (MOM_EINVAL, the text names both), the bases -- padded to the kernels' edge, and where the m = 0 reduction applies cut to
 * the (I,Q) sub-problem as well, with the (I,Q) <-> (U,V) test of that reduction made on the device -- are written by the kernels
 * of mom_z_moments with unchanged arithmetic, and the stage is gone.  Without a stage NULL is the MOM_EINVAL it always was.
 * mom_scene_set_partials / _set_optics_partials / _set_optics_bands_partials with dZpp == dZmp == NULL take a staged partial set
 * (P has to agree, and every basis[d] < K); without one NULL means "no dependence" as before.  A new scene drops a partial stage
 * that is still pending; mom_set_streams drops every stage.
 * Float32 handle: MOM_EUNSUPPORTED; before mom_set_streams: MOM_ESTATE.
 *   mom_scene_get_bases            the resident arrays as the kernels read them, whichever route set them: which = 0 the bases
 *                                  [edge, edge, K, M]; 1 the (I,Q) sub-problem's [edge, edge, K] (edge = 0: the scene is not reduced);
 *                                  2 dZpp / dZmp [edge, edge, K, M, P] (blocks = 0: none resident); 3 the Raman set [N, N, M].
 *                                  *blocks = the product of the trailing extents.  Zpp == Zmp == NULL: a size query. */
int mom_scene_stage_greeks(mom_t *h, int which, int nG, int l_pad, const int *l_max, const double *greek, int M);
int mom_scene_stage_greek_partials(mom_t *h, int P, int nD, const int *basis, const int *partial, int l_pad, const int *l_max,
                                   const double *dgreek);
int mom_scene_get_bases(mom_t *h, int which, int *edge, int *blocks, double *Zpp, double *Zmp);

/* ---- delta-BGE truncation of Greek coefficients ---------------------------------------------------
 * truncate_phase(mod::dBGE, aero) (src/Scattering/truncate_phase.jl:95-220) with the forward-mode partials of that function, for a
 * batch of nG Greek sets of one length l_full, each with nP derivative sets, in one call.  The phase functions f11 = P beta,
 * f12 = P2 (fac gamma), f34 = P2 (fac epsilon) are rebuilt from all l_full terms at the n_mu nodes; the three weighted fits (beta on
 * P[:, 0:l_tr], gamma and epsilon on fac P2[:, 2:l_tr]) run over ALL nodes (the reference reads D_angle and does not use it).  Every
 * normal matrix and right-hand side, of the value run and of each partial, is one product B^T diag(d) B with one more column B^T d'
 * on v_mfma_f64_16x16x4; A c = b and A dc = db - dA c are solved by one Cholesky factor per (set, fit) held in LDS.  Float64,
 * handle-free like mom_z_moments, error text: mom_last_global_error().
 *   mu, w_mu [n_mu]           nodes in [-1, 1] and weights; the reference takes gausslegendre(l_full), the call keeps n_mu free
 *   greek [l_full, 6, 1 + nP, nG]  l fastest, rows alpha, beta, gamma, delta, epsilon, zeta; row 0 of the third axis is the set,
 *                             rows 1 .. nP are its derivative sets (any direction: the map is differentiated along what it is given)
 *   l_tr                      the truncation order, 1 <= l_tr <= min(l_full, 128); above 128: MOM_EUNSUPPORTED
 * Outputs (host):
 *   greek_t [l_tr, 6, 1 + nP, nG]  beta^t = cl / c0, (alpha, delta, zeta)^t = (a - (beta - cl)) / c0, gamma^t and epsilon^t the fits
 *                             themselves with exact zeros at l < 2, and the partials of all of them by the quotient rules
 *   c0 [1 + nP, nG]           c0 = cl[0] and its partials: f^t = 1 - c0, df^t = -dc0.  (omega and k do not enter.)
 *   status [nG]               0, or bit q set when fit q (0 beta, 1 gamma, 2 epsilon) met a divisor f or a Cholesky pivot (for
 *                             fit 0 also c0) that is zero, negative (pivot) or not finite
 *   gpu_ms or NULL            HIP-event time (ms) of the kernels
 * Two calls are bitwise equal, and a set's rows do not depend on what else is in the batch.
 * MOM_EINVAL, checked before the first HIP call: n_mu, nG, l_full or l_tr < 1; nP < 0; l_tr > l_full; a null pointer (gpu_ms
 * excepted); a mu outside [-1, 1]; a weight or coefficient that is not finite; nG > 65535 or nP > 16383.
 * MOM_ESINGULAR when a status word is not zero: the text names the first such set and its first fit, every row of such a set (and
 * its c0 row) is NaN, every other set of the batch is as it would be alone. */
int mom_truncate_phase(int device, int n_mu, const double *mu, const double *w_mu, int nG, int nP, int l_full, int l_tr,
                       const double *greek, double *greek_t, double *c0, int *status, double *gpu_ms);

#ifdef __cplusplus
}
#endif
#endif /* MOMCORE_H */
