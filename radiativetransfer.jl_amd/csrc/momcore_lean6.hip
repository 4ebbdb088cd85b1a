// momcore_lean6.hip -- the six-wave lean strip image (mom_lean.hpp, kLean6): half-strip doubling chains, two workgroups per CU,
// three chain waves on every SIMD.  One object per operator size N = 4 * MOM_STRIP_KS (KS = 9, 10), compiled with -DMOM_WAVES=6
// -DMOM_NS=mom6.  Its entry in the image table: mom_images.hpp.
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_lean.hpp"
#include "mom_host.hpp"
#include "mom_images.hpp"

using namespace MOM_NS;

static hipError_t image_launch(const void *layer_args, const MomLaunchForm &, int grid, hipStream_t st) {
  return mom_launch_lds(k_layer_lean<MOM_STRIP_KS>, grid, kThreads, lean_lds_bytes(4 * MOM_STRIP_KS), st,
                        *reinterpret_cast<const LayerArgs *>(layer_args));
}
static size_t image_lds_bytes(int ns, int, int) { return lean_applies(4 * MOM_STRIP_KS, ns) ? lean_lds_bytes(4 * MOM_STRIP_KS) : 0; }
static int image_per_cu() { return 2; }
MOM_DEFINE_IMAGE(LEAN6, MOM_STRIP_KS, image_launch, image_lds_bytes, image_per_cu)
