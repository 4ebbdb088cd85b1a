// momcore_w4.hip -- the fused kernels instantiated for 4-wave (256-thread) workgroups, namespace mom4.
// Two such workgroups share a CU when 4 operators + vectors fit 80 KB of LDS (N <= 40); their phases then
// overlap each other's barriers and LDS latencies.  Host entry points are plain C++ functions used by
// mom_scene.hip; the argument blocks are layout-identical to mom::LayerArgs / mom::SurfArgs.
#define MOM_WAVES 4
#define MOM_TJ 3
#define MOM_NO_STRAIGHT  // operators of this build have at most 12 MFMA k-steps
#define MOM_NS mom4
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_entry.hpp"
#include "mom_host.hpp"

using namespace mom4;

size_t mom4_lds_bytes(int N, bool lds_mats) { return lds_bytes(N, lds_mats); }
int mom4_generic_bufs_elems(int N) { return (int)(kGenericBufs * mat_elems(N)); }

hipError_t mom4_launch_layer(const void *layer_args, int iface, bool lds, int grid, size_t smem, hipStream_t st) {
  const LayerArgs a = *reinterpret_cast<const LayerArgs *>(layer_args);
  // multi-target form (interface code dispatched at run time)
  if (a.ntgt > 0) return mom_launch_ldsm(MOM_LDSM(k_layer, -1, 0, true), lds, grid, kThreads, smem, st, a);
#define W4_LAUNCH(IF) return mom_launch_ldsm(MOM_LDSM(k_layer, IF), lds, grid, kThreads, smem, st, a)
  MOM_IFACE_SWITCH(iface, W4_LAUNCH)
#undef W4_LAUNCH
}

hipError_t mom4_launch_surface(const void *surf_args, bool lds, int grid, size_t smem, hipStream_t st) {
  const SurfArgs a = *reinterpret_cast<const SurfArgs *>(surf_args);
  return mom_launch_ldsm(MOM_LDSM(k_surface), lds, grid, kThreads, smem, st, a);
}
