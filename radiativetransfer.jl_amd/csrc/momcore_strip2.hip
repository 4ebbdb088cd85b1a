// momcore_strip2.hip -- the two-buffer 4-wave strip image (mom_strip2.hpp) for ONE operator size N = 4 * MOM_STRIP_KS
// (Makefile: KS = 13, 14, 15, namespace mom2, -DMOM_WAVES=4).  Only the sweep kernel of the image is compiled here; the 8-wave
// image (momcore_strip.hip, namespace mom) finishes whatever it leaves.
#ifndef MOM_STRIP_KS
#error "compile with -DMOM_STRIP_KS=<N/4>"
#endif
#include <hip/hip_runtime.h>

#include "mom_diag.hpp"
#include "mom_host.hpp"
#include "mom_images.hpp"
#include "mom_strip2.hpp"
#include "mom_strip2_variants.hpp"

using namespace MOM_NS;

static_assert(kMomStrip2SchedInts == (size_t)kS2SchedInts, "mom_images.hpp: size of LayerArgs::sched");

// the sweep kernel, one per scheduling mode (mom_strip2.hpp) and, for the default mode 1, one per number of k-steps the zero-weight
// streams let a strip product leave out (MOM_OPT_ZERO_SKIP bit 1, LayerArgs::nbw; mom_strip2_variants.hpp): KW = KS - kS2Skip[V].
// Modes 0, 2 and 3 are the recorded forms of the scheduling experiments and keep KW = KS.  RB: the row-block rule (MOM_OPT_ZERO_SKIP
// bit 2, the flag kS2RowBlocks in LayerArgs::nbw), default mode only and only where it changes a row tile.  SRC: the sources-only
// form (MOM_OPT_SOURCES_ONLY, the flag kMomNbwSourcesOnly in LayerArgs::nbw), default mode only, for every (KW, RB) of it; a launch
// in another mode takes its kernel with all four composite operators
static_assert(MOM_STRIP_KS > kS2Skip[kS2Variants - 1], "momcore_strip2.hip: KS - skip >= 1");
// EL: the table form of the elemental layer (MOM_OPT_ELEMENTAL, the flag kMomNbwElemental in LayerArgs::nbw), default mode only,
// for every (KW, RB, SRC) of it
template <int MODE, int V = 0, bool RB = false, bool SRC = false, bool EL = false>
static hipError_t launch_s2(const LayerArgs &a, int grid, hipStream_t st) {
  constexpr int KW = MOM_STRIP_KS - kS2Skip[V];
  constexpr bool RBK = RB && s2_row_blocks_change(MOM_STRIP_KS, KW);
  const size_t smem = s2_lds_bytes(4 * MOM_STRIP_KS);
  hipError_t e = mom_allow_lds(reinterpret_cast<const void *>(k_layer_s2<MOM_STRIP_KS, MODE, KW, RBK, SRC, EL>), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_layer_s2<MOM_STRIP_KS, MODE, KW, RBK, SRC, EL>), dim3(grid), dim3(kThreads), smem, st, a);
  return hipGetLastError();
}
template <bool RB, bool SRC, bool EL>
static hipError_t launch_s2_default(const LayerArgs &a, int grid, hipStream_t st) {
  switch (s2_variant_for(MOM_STRIP_KS, s2_nbw_count(a.nbw))) {
    case 1: return launch_s2<1, 1, RB, SRC, EL>(a, grid, st);
    case 2: return launch_s2<1, 2, RB, SRC, EL>(a, grid, st);
    case 3: return launch_s2<1, 3, RB, SRC, EL>(a, grid, st);
    default: return launch_s2<1, 0, RB, SRC, EL>(a, grid, st);
  }
}
template <bool EL>
static hipError_t launch_s2_form(const LayerArgs &a, int grid, hipStream_t st) {
  if (a.nbw & kMomNbwSourcesOnly)
    return s2_row_blocks_for(MOM_STRIP_KS, a.nbw) ? launch_s2_default<true, true, EL>(a, grid, st) : launch_s2_default<false, true, EL>(a, grid, st);
  return s2_row_blocks_for(MOM_STRIP_KS, a.nbw) ? launch_s2_default<true, false, EL>(a, grid, st) : launch_s2_default<false, false, EL>(a, grid, st);
}
static hipError_t image_launch(const void *layer_args, int, int grid, hipStream_t st) {
  const LayerArgs a = *reinterpret_cast<const LayerArgs *>(layer_args);
  switch (a.sched_mode & 3) {
    case 1: return (a.nbw & kMomNbwElemental) ? launch_s2_form<true>(a, grid, st) : launch_s2_form<false>(a, grid, st);
    case 2: return launch_s2<2>(a, grid, st);
    case 3: return launch_s2<3>(a, grid, st);
    default: return launch_s2<0>(a, grid, st);
  }
}
// LDS bytes, 0 if the image does not apply to ns Stokes components per stream (nS per stream entry of the scene)
static size_t image_lds_bytes(int ns, int nS, int) { return s2_applies(4 * MOM_STRIP_KS, ns, nS) ? s2_lds_bytes(4 * MOM_STRIP_KS) : 0; }
static int image_per_cu() { return 2; }
MOM_DEFINE_IMAGE(STRIP2, MOM_STRIP_KS, image_launch, image_lds_bytes, image_per_cu)

#ifdef MOM_DIAG_TIMELINE
// diagnostic builds (tools/phase_stamps_s2.py): the timelines of the last launch; ev[kTlWgs * kTlCap], hdr[4 * kTlWgs]
#define MOM_CAT2(a, b) a##b
#define MOM_CAT(a, b) MOM_CAT2(a, b)
extern "C" int MOM_CAT(MOM_CAT(mom2_strip, MOM_STRIP_KS), _timeline_read)(unsigned long long *ev, unsigned *hdr, int *wgs, int *cap) {
  *wgs = kTlWgs; *cap = kTlCap;
  if (!ev) return 0;
  if (hipMemcpyFromSymbol(ev, HIP_SYMBOL(mom_tl_ev), sizeof(unsigned long long) * kTlWgs * kTlCap) != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(hdr, HIP_SYMBOL(mom_tl_hdr), sizeof(unsigned) * 4 * kTlWgs) != hipSuccess) return 1;
  return 0;
}
#endif
