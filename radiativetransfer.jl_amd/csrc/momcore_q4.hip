// momcore_q4.hip -- the quad-block image (mom_q4.hpp): one wavefront per (spectral point, moment) unit of an N = 36 / 40 problem,
// v_mfma_f64_4x4x4_4b products, four units per CU.  One object per operator size N = 4 * MOM_STRIP_KS (KS = 9, 10), compiled with
// -DMOM_WAVES=1 -DMOM_NS=momq.  Its entry in the image table: mom_images.hpp.  An object holds the kernel once per instantiated
// number of weighted block rows (MOM_OPT_ZERO_SKIP, LayerArgs::nbw): the image's launch function picks among them.
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_q4.hpp"
#include "mom_host.hpp"
#include "mom_images.hpp"

using namespace MOM_NS;

// The instantiations of the zero-skip rule (mom_q4.hpp q4_mul_c): NBW = NB - kSkip[v] block rows of weighted entries.  A rule for
// FEWER zero blocks than the problem has is still exact, so a launch takes the smallest instantiated NBW >= LayerArgs::nbw:
// one to four zero-weight streams of two to four components (the view angles, the Sun, a dummy stream) are 0, 1, 2 .. 4 blocks
constexpr int kNB = MOM_STRIP_KS;
constexpr int kSkip[] = {0, 1, 2, 4};
static_assert(kNB > 4, "momcore_q4.hip: NB - 4 >= 1");
// SRC: every variant once more in the sources-only form (MOM_OPT_SOURCES_ONLY; the flag kMomNbwSourcesOnly beside the count)
// EL: and each of those once more with the table form of the elemental layer (MOM_OPT_ELEMENTAL; the flag kMomNbwElemental)
template <int V, bool SRC = false, bool EL = false>
static const void *variant_fn() { return reinterpret_cast<const void *>(k_layer_q4<MOM_STRIP_KS, kNB - kSkip[V], SRC, EL>); }
static int variant_for(int nbw) {
  nbw &= ~(kMomNbwSourcesOnly | kMomNbwElemental);
  if (nbw < 1 || nbw > kNB) return 0;
  int v = 0;
  for (int c = 1; c < (int)(sizeof kSkip / sizeof kSkip[0]); ++c)
    if (kNB - kSkip[c] >= nbw) v = c;
  return v;
}
template <int V, bool SRC, bool EL>
static hipError_t launch_variant(const LayerArgs &a, int grid, hipStream_t st) {
  const size_t smem = q4_lds_bytes(4 * MOM_STRIP_KS);
  hipError_t e = mom_allow_lds(variant_fn<V, SRC, EL>(), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_layer_q4<MOM_STRIP_KS, kNB - kSkip[V], SRC, EL>), dim3(grid), dim3(64), smem, st, a);
  return hipGetLastError();
}
template <bool SRC, bool EL>
static hipError_t launch_form(const LayerArgs &a, int grid, hipStream_t st) {
  switch (variant_for(a.nbw)) {
    case 1: return launch_variant<1, SRC, EL>(a, grid, st);
    case 2: return launch_variant<2, SRC, EL>(a, grid, st);
    case 3: return launch_variant<3, SRC, EL>(a, grid, st);
    default: return launch_variant<0, SRC, EL>(a, grid, st);
  }
}
template <bool EL>
static hipError_t launch_el(const LayerArgs &a, int grid, hipStream_t st) {
  return (a.nbw & kMomNbwSourcesOnly) ? launch_form<true, EL>(a, grid, st) : launch_form<false, EL>(a, grid, st);
}
static hipError_t image_launch(const void *layer_args, int, int grid, hipStream_t st) {
  const LayerArgs a = *reinterpret_cast<const LayerArgs *>(layer_args);
  return (a.nbw & kMomNbwElemental) ? launch_el<true>(a, grid, st) : launch_el<false>(a, grid, st);
}
// workgroups of this image a CU holds: by LDS and by the registers the compiler gave the kernel (occupancy API); the least of the
// instantiations, so that the persistent grid fits whichever of them a launch takes
template <int V, bool SRC, bool EL>
static int query_variant_per_cu() {
  int nb = 0;
  const size_t smem = q4_lds_bytes(4 * MOM_STRIP_KS);
  if (mom_allow_lds(variant_fn<V, SRC, EL>(), smem) != hipSuccess) return 4;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_layer_q4<MOM_STRIP_KS, kNB - kSkip[V], SRC, EL>, 64, smem) != hipSuccess || nb < 1) return 4;
  return nb;
}
template <bool SRC, bool EL>
static int query_form_per_cu() {
  return std::min(std::min(query_variant_per_cu<0, SRC, EL>(), query_variant_per_cu<1, SRC, EL>()),
                  std::min(query_variant_per_cu<2, SRC, EL>(), query_variant_per_cu<3, SRC, EL>()));
}
static int query_per_cu() {
  return std::min(std::min(query_form_per_cu<false, false>(), query_form_per_cu<true, false>()),
                  std::min(query_form_per_cu<false, true>(), query_form_per_cu<true, true>()));
}
static int image_per_cu() {
  static const int per_cu = query_per_cu();  // (per process: the occupancy of an image does not depend on the handle)
  return per_cu;
}
// LDS bytes of one (one-wave) workgroup; 0 if the image does not apply to ns Stokes components per stream and K phase-matrix bases
static size_t image_lds_bytes(int ns, int, int K) { return q4_applies(4 * MOM_STRIP_KS, ns, K) ? q4_lds_bytes(4 * MOM_STRIP_KS) : 0; }
MOM_DEFINE_IMAGE(QUAD, MOM_STRIP_KS, image_launch, image_lds_bytes, image_per_cu)

#ifdef MOM_DIAG_STAMPS
#define MOM_CAT2(a, b) a##b
#define MOM_CAT(a, b) MOM_CAT2(a, b)
extern "C" int MOM_CAT(momq_q4_diag_read, MOM_STRIP_KS)(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mom_diag_acc), 128 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mom_diag_acc), z, sizeof z) != hipSuccess) return 1;
  }
  return 0;
}
#endif
