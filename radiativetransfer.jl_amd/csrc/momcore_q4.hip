// momcore_q4.hip -- the quad-block image (mom_q4.hpp): one wavefront per (spectral point, moment) unit of an N = 36 / 40 problem,
// v_mfma_f64_4x4x4_4b products, four units per CU.  One object per operator size N = 4 * MOM_STRIP_KS (KS = 5 .. 10: MOM_IMAGE_LIST),
// compiled with -DMOM_WAVES=1 -DMOM_NS=momq.  Its entry in the image table: mom_images.hpp.  An object holds the kernel once per
// instantiated number of weighted block rows (MOM_OPT_ZERO_SKIP, MomLaunchForm::nbw): the image's launch function picks among them.
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_q4.hpp"
#include "mom_host.hpp"
#include "mom_image_variants.hpp"

using namespace MOM_NS;

// The instantiations of the zero-skip rule (mom_q4.hpp q4_mul_c): NBW = NB - kQ4Skip[v] block rows of weighted entries, the smallest
// instantiated NBW >= MomLaunchForm::nbw (mom_image_variants.hpp): one to four zero-weight streams of two to four components (the
// view angles, the Sun, a dummy stream) are 0, 1, 2 .. 4 blocks.  SRC: every variant once more in the sources-only form
// (MOM_OPT_SOURCES_ONLY); EL: and each of those once more with the table form of the elemental layer (MOM_OPT_ELEMENTAL)
static_assert(MOM_STRIP_KS > kQ4Skip[kSkipVariants - 1], "momcore_q4.hip: NB - 4 >= 1");
using LayerKernel = void (*)(LayerArgs);
static LayerKernel q4_kernel(int v, bool src, bool el) {
  return mom_with_int<0, kSkipVariants - 1>(v, [&](auto V) {
    return mom_with_bool(src, [&](auto SRC) {
      return mom_with_bool(el, [&](auto EL) -> LayerKernel { return k_layer_q4<MOM_STRIP_KS, MOM_STRIP_KS - kQ4Skip[V], SRC, EL>; });
    });
  });
}
static hipError_t image_launch(const void *layer_args, const MomLaunchForm &f, int grid, hipStream_t st) {
  const LayerKernel k = q4_kernel(mom_skip_variant(kQ4Skip, MOM_STRIP_KS, f.nbw), f.sources_only, f.elemental_tab);
  return mom_launch_lds(k, grid, 64, q4_lds_bytes(4 * MOM_STRIP_KS), st, *reinterpret_cast<const LayerArgs *>(layer_args));
}
// workgroups of this image a CU holds: by LDS and by the registers the compiler gave the kernel (occupancy API); the least of the
// instantiations, so that the persistent grid fits whichever of them a launch takes
static int query_per_cu() {
  const size_t smem = q4_lds_bytes(4 * MOM_STRIP_KS);
  int per_cu = 1 << 30;
  for (int key = 0; key < 4 * kSkipVariants; ++key) {
    const LayerKernel k = q4_kernel(key >> 2, (key & 1) != 0, (key & 2) != 0);
    int nb = 0;
    if (mom_allow_lds(reinterpret_cast<const void *>(k), smem) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 64, smem) != hipSuccess || nb < 1)
      nb = 4;  // (a kernel whose query fails counts as four per CU)
    per_cu = std::min(per_cu, nb);
  }
  return per_cu;
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
