// momcore_strip2.hip -- the two-buffer 4-wave strip image (mom_strip2.hpp) for ONE operator size N = 4 * MOM_STRIP_KS
// (Makefile: KS = 13, 14, 15, namespace mom2, -DMOM_WAVES=4).  Only the sweep kernel of the image is compiled here; the 8-wave
// image (momcore_strip.hip, namespace mom) finishes whatever it leaves.
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_host.hpp"
#include "mom_strip2.hpp"

using namespace MOM_NS;

#define MOM_CAT2(a, b) a##b
#define MOM_CAT(a, b) MOM_CAT2(a, b)

// mom2_strip<KS>_launch(args, grid, stream): the sweep kernel; mom2_strip<KS>_lds_bytes(ns, nS): its LDS bytes, 0 if the image
// does not apply to ns Stokes components per stream (nS per stream entry of the scene)
hipError_t MOM_CAT(MOM_CAT(mom2_strip, MOM_STRIP_KS), _launch)(const void *layer_args, int grid, hipStream_t st) {
  const LayerArgs a = *reinterpret_cast<const LayerArgs *>(layer_args);
  const size_t smem = s2_lds_bytes(4 * MOM_STRIP_KS);
  hipError_t e = mom_allow_lds(reinterpret_cast<const void *>(k_layer_s2<MOM_STRIP_KS>), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_layer_s2<MOM_STRIP_KS>), dim3(grid), dim3(kThreads), smem, st, a);
  return hipGetLastError();
}
size_t MOM_CAT(MOM_CAT(mom2_strip, MOM_STRIP_KS), _lds_bytes)(int ns, int nS) {
  return s2_applies(4 * MOM_STRIP_KS, ns, nS) ? s2_lds_bytes(4 * MOM_STRIP_KS) : 0;
}
