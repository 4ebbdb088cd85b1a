// mom_rrs.hpp -- host interface of the rotational-Raman (RRS) kernels (mom_rrs.hip) towards mom_rrs_api.hip.
//
// State of the inelastic path of rt_run(::RRS) (src/CoreRT/rt_run.jl:41-230): the reference's AddedLayerRS / CompositeLayerRS
// (types.jl:145-205) as persistent HBM arrays in the reference's own memory order -- elastic operators [N,N,S], sources
// [N,S], inelastic operators [N,N,S,nRaman], inelastic sources [N,S,nRaman] (Julia column-major) -- plus per-point scratch
// operands of the current doubling step / interaction.
//
// Device memory: every allocation of State is a MomDevBuf (mom_host.hpp) or a GuardedBuf in State::arrays; the role pointers
// (added, comp, surf, smat ...) are aliases into those and are never freed.  Launches: the host driver (mom_rrs.hip) describes
// the kernel form it wants as a Form; one function per object turns a Form into a launch (momr::launch, momr_big_launch).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mom_host.hpp"

namespace momr {

struct Streams {
  const double *mu, *wt;  // [N] device
  double I0[4], D[4];
  int N, nS, imu0, strict_idx;
  double mu0;
};

// indices into State::added / surf / comp
enum { R_PM = 0, R_MP = 1, T_MM = 2, T_PP = 3, J0P = 4, J0M = 5 };        // AddedLayer field order of momcore.h
enum { C_R_MP = 0, C_R_PM = 1, C_T_PP = 2, C_T_MM = 3, C_J0P = 4, C_J0M = 5 };  // CompositeLayer field order

// kernel-form switches (State::kopt; MOM_OPT_RRS_KERNELS): every form computes the same products in the same order
enum { KOPT_WG = 1, KOPT_WG2 = 2, KOPT_WG_POINT = 4, KOPT_EL_TILE = 8, KOPT_EL_FUSE_ON = 16, KOPT_EL_FUSE_OFF = 32,
       KOPT_DEFAULT = KOPT_WG | KOPT_WG2 | KOPT_WG_POINT | KOPT_EL_TILE };

#pragma GCC visibility push(hidden)  // internal to libmomcore.so, like the helpers of mom_host.hpp
// A layer array between two GUARD BANDS of kGuard doubles filled with a canary pattern (r5, ADVICE r4: the kernels store whole
// tiles without edge masks; the zero-padding invariant only sees writes that land INSIDE an array).  count_padding checks the
// bands of every array too: a store before the first or behind the last block of any layer array shows up as a violation
// (tests/test_gpu_rrs.py::test_rrs_zero_padding_invariant, N = 15 ... 60, both switch positions).
constexpr size_t kGuard = 2048;               // doubles per band (16 KB: more than a 4 x 4-tile block row)
constexpr unsigned kCanary = 0xDEADBEEFu;     // both halves of a canary double
struct GuardedBuf {
  // Layer: state of the layers in padded blocks (reset_layers zeroes it, count_padding scans its padding); Sequence: layer state
  // count_padding does not scan (expk, jpseq); Scratch: per-point operands of the current step (neither)
  enum class Use { Layer, Sequence, Scratch };
  MomDevBuf<double> mem;  // band | count doubles | band
  size_t count = 0;
  Use use = Use::Scratch;
  bool matrix = false;    // blocks of P x P doubles (else P)
  size_t nblk = 0;        // S or S x nR
  double *data() const { return mem.get() + kGuard; }
  // `n` zeros between two canary bands (MomDevBuf::renew does not fill)
  hipError_t renew(size_t n);
};

// The kernel form of one launch.  Family: what is computed and by which unit (a wavefront per point / per pair, a workgroup of
// nt waves per point / per pair, mom_rrs_wg.hpp); nt: tiles per operator edge, 16 nt >= N; the variant fields are the template
// arguments of the family that reads them.
enum class Family { ElPoint, DblPoint, IntPoint, DblPair, IntPair, DblPairWg, IntPairWg, DblPointWg, IntPointWg, TileElemental };
struct Form {
  Family family;
  int nt;
  bool fuse_el = false;  // DblPair(Wg): first doubling step of a layer, the inelastic elemental layer is formed in registers
  int mode = 0;          // DblPair(Wg): 0 corrected position, 1 its last step of a layer, 2 strict position
  bool surface = false;  // IntPair(Wg): the added layer is the surface (its ie* arrays are zeros)
  bool derive = false;   // IntPair(Wg): ier+- / iet-- derived where they are read
  bool nd0 = false;      // TileElemental: a layer without doublings (the D kernels are applied at once)
};
constexpr bool workgroup_form(Family f) {
  return f == Family::DblPairWg || f == Family::IntPairWg || f == Family::DblPointWg || f == Family::IntPointWg;
}

struct State {
  int N = 0, nS = 0, S = 0, nR = 0;
  int kopt = KOPT_DEFAULT;
  int P = 16;              // row pitch of every device block: 16 (N <= 16) or 32; matrices P x P, vectors P, zero padding --
                           // the tile loads of the kernels are then unmasked, 128-byte aligned and at immediate offsets
  int strict_rrs = 1;      // rrs_strict_reference (DESIGN.md "RRS": D1..D5)
  int n_glob0 = 0;         // global 0-based spectral index of local index 0 (shards; strict D2/D3 use absolute indices)
  int n1_lo = 0, n1_hi = 0;  // spectral points this rank owns: pairs (n1, dn) are processed for n1 in [n1_lo, n1_hi)
  hipStream_t stream = nullptr;
  MomDevBuf<int> d_off;         // [nR] i_l1l0
  MomDevBuf<double> d_varpiR;   // [nR]
  int max_off = 0;
  // Every layer array, in allocation order (create): what reset_layers, count_padding and the destructor walk.  The role
  // pointers below are aliases into it.
  std::vector<GuardedBuf> arrays;
  // elastic added layer, double-buffered over the doubling steps (cur = buffer holding the current state)
  double *added[2][6] = {};     // R_PM / T_MM exist once (added[0]) and are written after the doubling
  double *expk[2] = {};
  int cur = 0;
  double *surf[6] = {};
  double *comp[2][6] = {};
  int ccur = 0;
  // per-point scratch operands: up to 10 matrices [N,N,S], 6 vectors [N,S], the j0+ sequence of the strict position
  double *smat[10] = {};
  double *svec[6] = {};
  double *jpseq = nullptr;      // [N,S,nR]
  // inelastic layers
  double *ie_added[6] = {};     // ier+-, ier-+, iet--, iet++ [N,N,S,nR]; ieJ0+, ieJ0- [N,S,nR]   (R_PM.. order)
  double *ie_comp[6] = {};      // ieR-+, ieR+-, ieT++, ieT-- ; ieJ0+, ieJ0-                     (C_R_MP.. order)
  MomDevBuf<double> d_out;      // R_SFI | T_SFI | ieR_SFI | ieT_SFI | hdr [5][nVza,nS,S], then bhr_uw | bhr_dw [2][nS,S]
  int out_nVza = 0;             // the nVza d_out is sized for (0: none yet)
  MomDevBuf<int> d_info;
  MomDevBuf<double> d_stage;    // ABI-order staging of upload / download (grown on demand)
  // fast scene-level mode (mom_rt_run_rrs): the inelastic elemental of a layer with ndoubl >= 1 is deferred into the first
  // doubling step (el_pending + its inputs), and in the corrected position ier+- / iet-- are not stored by the doubling but
  // derived where they are read (pm_derivable); pm_valid says whether the arrays themselves hold the current values
  bool fast = false, el_pending = false, pm_valid = true, pm_derivable = false;
  // true once an operator-level entry may have written the layers (uploads, mom_rrs_elemental ...) or a strict-position run
  // has ended: the next scene-level run zeroes the layers first (the reference allocates them zeroed per rt_run)
  bool dirty = false;
  struct { int m, nd, sh; const double *tau_sum, *tau, *varpi, *fscatt, *Zr_pp, *Zr_mp; } el{};
  // HIP-event pairs around the launches of the heavy kernels of the last run (timing_reset .. timing_read)
  std::vector<hipEvent_t> ev_pool;
  std::vector<int> ev_kind;  // kind of the launch bracketed by ev_pool[2k], ev_pool[2k+1]
  bool timing = false;
  std::string err;
};
#pragma GCC visibility pop
enum { TK_DBL_PAIR = 0, TK_INT_PAIR = 1, TK_IE_ELEMENTAL = 2, TK_COUNT = 3 };
void timing_reset(State *s, bool on);
// ms[k], launches[k] for k < TK_COUNT (synchronises the stream)
hipError_t timing_read(State *s, double *ms, int *launches);

hipError_t create(State **out, hipStream_t st, int N, int nS, int S, int nR, const int *off_host, const double *varpi_host,
                  int strict_rrs);
void destroy(State *s);
// one layer array between the ABI's memory order (host, [N,N,nblk] or [N,nblk]) and the padded device blocks (synchronous)
hipError_t upload(State *s, double *dev, const double *host, bool matrix, size_t nblk);
hipError_t download(State *s, double *host, const double *dev, bool matrix, size_t nblk);

// elemental!(...) elastic part + elemental_inelastic!(::RRS) on the persistent added layer.  Zpp/Zmp: device [N,N] x nTerms with
// per-point weights zw [nTerms,S] (zw == nullptr: one term of weight 1); Zr*: device [N,N] Raman phase matrices; all
// spectral vectors device [S]; the elemental optical thickness is tau / 2^shift.
hipError_t elemental(State *s, const Streams &q, int m, int nd, int shift, const double *tau_sum, const double *tau, const double *varpi,
                     const double *Zpp, const double *Zmp, int nTerms, const double *zw, const double *fscatt,
                     const double *Zr_pp, const double *Zr_mp, bool elastic, bool inelastic);
// doubling_helper!(::RRS): nd steps on the persistent added layer (expk in s->expk[s->cur]); applies the D kernels at the end
hipError_t doubling(State *s, const Streams &q, int nd);
// rt_kernel.jl:326-333
hipError_t copy_added_to_composite(State *s, const Streams &q);
// writes ier+- / iet-- out if they are only derivable at the moment (before downloads, copies and operator-level reads)
hipError_t ensure_pm(State *s, const Streams &q);
// an upload replaced layer arrays: whatever is resident is what the arrays hold
inline void mark_uploaded(State *s) { s->pm_valid = true; s->pm_derivable = false; s->el_pending = false; }
// interaction_helper!(::RRS, iface): returns hipErrorInvalidValue with s->err set where the reference raises (strict position)
hipError_t interaction(State *s, const Streams &q, int iface, bool with_surface);
// create_surface_layer! into s->surf (ie* of the surface layer are zeros: never allocated).  kind 0 LambertianSurfaceScalar
// (albedo), 1 BRDF Fourier matrix Rsurf_m [N,N] of moment m (device), 2 LambertianSurfaceLegendre (albedo_spec [S], device)
hipError_t surface(State *s, const Streams &q, int m, int kind, double albedo, const double *tau_tot, const double *Rsurf_m,
                   const double *albedo_spec);
// number of nonzero (or NaN) entries in the zero padding of all layer arrays (the invariant the whole-tile stores rest on)
hipError_t count_padding(State *s, unsigned long long *out);
// start of a scene-level run: zeroed layers where needed (State::dirty, strict position), double-buffer / pm flags reset,
// output block zeroed (postprocessing_vza!(::RRS) accumulates into s->d_out)
hipError_t begin_run(State *s, int nVza);
hipError_t postprocess(State *s, const Streams &q, int m, int nVza, const int *d_node, const double *d_cos, const double *d_sin,
                       int M, double weight);

}  // namespace momr

#pragma GCC visibility push(hidden)
// mom_rrs.hip built with -DMOMR_BIG_TU (mom_rrs_big.o): the one launcher of the device code of that object -- the 3 x 3- and
// 4 x 4-tile images of the wave families (32 < N <= 64) and every workgroup family (nt = 2 ... 4).  `args` is the KArgs of the
// caller as a void *: KArgs is declared once per namespace (momr, momr_big; layout-identical, same source text), and a shared
// declaration would rename every kernel of both objects.  `iface` is read by the interaction families only.
hipError_t momr_big_launch(const momr::Form &f, unsigned grid, hipStream_t stream, const void *args, int iface);
#pragma GCC visibility pop
