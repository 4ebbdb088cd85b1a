// momcore_gen.hip -- the general (non strip-chained) layer kernels of the 8-wave build, k_layer<LDSM, IFACE>, in a
// translation unit of their own: they are the largest kernel images of the library (eight of them), and compiling them
// next to the rest of momcore.hip serialised the build.  Host entry point used by mom_scene.hip.
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_host.hpp"

using namespace MOM_NS;

hipError_t mom_gen_launch_layer(const void *layer_args, int iface, bool lds, int grid, size_t smem, hipStream_t st) {
  const LayerArgs a = *reinterpret_cast<const LayerArgs *>(layer_args);
  // multi-target form: one image per LDS mode, interface code dispatched at run time (IFACE = -1)
  if (a.ntgt > 0) return mom_launch_ldsm(MOM_LDSM(k_layer, -1, 0, true), lds, grid, kThreads, smem, st, a);
#define GEN_LAUNCH(IF) return mom_launch_ldsm(MOM_LDSM(k_layer, IF), lds, grid, kThreads, smem, st, a)
  MOM_IFACE_SWITCH(iface, GEN_LAUNCH)
#undef GEN_LAUNCH
}

#ifdef MOM_DIAG_STAMPS
// diagnostic builds: the stamp accumulators of THIS translation unit (the general layer kernels)
extern "C" int mom_diag_read_gen(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mom_diag_acc), 128 * sizeof(unsigned long long)) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mom_diag_acc), z, sizeof z) != hipSuccess) return -2;
  }
  return 0;
}
#endif
