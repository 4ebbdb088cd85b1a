// momcore_strip.hip -- k_layer with the strip-chained doubling / interaction paths (mom_strip.hpp) for ONE
// operator size N = 4 * MOM_STRIP_KS, compiled once per size so that each kernel image carries a single
// unrolled variant (Makefile: KS = 13, 14, 15, i.e. N = 52, 56, 60, in the 8-wave build, namespace mom;
// KS = 9, 10, 11, i.e. N = 36, 40, 44, in the 4-wave build, namespace mom4, two workgroups per CU).
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_host.hpp"
#include "mom_images.hpp"
// the lean image (three operator buffers, three workgroups per CU): Float64, 4-wave build, N = 36, 40
#if defined(MOM_WAVES) && MOM_WAVES == 4 && !defined(MOM_REAL_IS_FLOAT) && (MOM_STRIP_KS == 9 || MOM_STRIP_KS == 10)
#define MOM_HAVE_LEAN 1
#include "mom_lean.hpp"
#endif

using namespace MOM_NS;

// family of this build in the image table (mom_images.hpp), from its workgroup shape and precision
#if defined(MOM_REAL_IS_FLOAT)
#if defined(MOM_WAVES) && MOM_WAVES == 4
#define MOM_IMAGE_FAMILY F32_STRIP4
#else
#define MOM_IMAGE_FAMILY F32_STRIP8
#endif
#elif defined(MOM_WAVES) && MOM_WAVES == 4
#define MOM_IMAGE_FAMILY STRIP4
#else
#define MOM_IMAGE_FAMILY STRIP8
#endif

// LDS bytes of one workgroup of this image: the vector area depends on the workgroup shape of the build, the Float64 builds
// add the persistent stream-pair tables for ns Stokes components per stream
static size_t image_lds_bytes(int ns, int, int) { return strip_lds_bytes(4 * MOM_STRIP_KS, ns); }
static int image_per_cu() { return kWaves == 4 ? 2 : 1; }  // 4-wave builds: two LDS images fit a CU (mom_kernels.hpp ld_for)

static hipError_t image_launch(const void *layer_args, const MomLaunchForm &, int grid, hipStream_t st) {
  const LayerArgs &a = *reinterpret_cast<const LayerArgs *>(layer_args);
  const size_t smem = image_lds_bytes(a.q.regular ? a.q.nS : 1, 0, 0);
  // multi-target form (interface code dispatched at run time)
  if (a.ntgt > 0) return mom_launch_lds(k_layer<true, -1, MOM_STRIP_KS, true>, grid, kThreads, smem, st, a);
  hipError_t e = hipSuccess;
#define STRIP_LAUNCH(IF) e = mom_launch_lds(k_layer<true, IF, MOM_STRIP_KS>, grid, kThreads, smem, st, a)
  MOM_IFACE_SWITCH(a.iface, STRIP_LAUNCH)
#undef STRIP_LAUNCH
  return e;
}
MOM_DEFINE_IMAGE(MOM_IMAGE_FAMILY, MOM_STRIP_KS, image_launch, image_lds_bytes, image_per_cu)

#ifdef MOM_HAVE_LEAN
// the lean sweep kernel of the same build: LDS bytes 0 if it does not apply to ns Stokes components per stream
static size_t lean_image_lds_bytes(int ns, int, int) { return lean_applies(4 * MOM_STRIP_KS, ns) ? lean_lds_bytes(4 * MOM_STRIP_KS) : 0; }
static int lean_image_per_cu() { return 3; }
static hipError_t lean_image_launch(const void *layer_args, const MomLaunchForm &, int grid, hipStream_t st) {
  return mom_launch_lds(k_layer_lean<MOM_STRIP_KS>, grid, kThreads, lean_lds_bytes(4 * MOM_STRIP_KS), st,
                        *reinterpret_cast<const LayerArgs *>(layer_args));
}
MOM_DEFINE_IMAGE(LEAN, MOM_STRIP_KS, lean_image_launch, lean_image_lds_bytes, lean_image_per_cu)
#endif

#ifdef MOM_DIAG_STAMPS
// diagnostic builds (tools/phase_stamps*.py load it by name): mom_strip_diag_read<KS>, or with the prefix of the build's rule
#define MOM_CAT2(a, b) a##b
#define MOM_CAT(a, b) MOM_CAT2(a, b)
#ifndef MOM_STRIP_PREFIX
#define MOM_STRIP_PREFIX mom_strip
#endif
extern "C" int MOM_CAT(MOM_CAT(MOM_STRIP_PREFIX, _diag_read), MOM_STRIP_KS)(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mom_diag_acc), 128 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mom_diag_acc), z, sizeof z) != hipSuccess) return 1;
  }
  return 0;
}
#endif
