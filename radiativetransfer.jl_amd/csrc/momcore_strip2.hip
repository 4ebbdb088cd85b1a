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
#include "mom_image_variants.hpp"

using namespace MOM_NS;

static_assert(kMomStrip2SchedInts == (size_t)kS2SchedInts, "mom_images.hpp: size of LayerArgs::sched");

// the sweep kernel, one per scheduling mode (mom_strip2.hpp) and, for the default mode 1, one per number of k-steps the zero-weight
// streams let a strip product leave out (MOM_OPT_ZERO_SKIP bit 1, MomLaunchForm::nbw; mom_image_variants.hpp): KW = KS - kS2Skip[V].
// Modes 0, 2 and 3 are the recorded forms of the scheduling experiments: KW = KS, all four composite operators, elemental_build.
// Default mode only: RB, the row-block rule (MOM_OPT_ZERO_SKIP bit 2), instantiated only where it changes a row tile; SRC, the
// sources-only form (MOM_OPT_SOURCES_ONLY), for every (KW, RB); EL, the table form of the elemental layer (MOM_OPT_ELEMENTAL), for
// every (KW, RB, SRC)
static_assert(MOM_STRIP_KS > kS2Skip[kSkipVariants - 1], "momcore_strip2.hip: KS - skip >= 1");
using LayerKernel = void (*)(LayerArgs);
static LayerKernel s2_kernel(int mode, int v, bool rb, bool src, bool el) {
  if (mode != 1) return mode == 2 ? k_layer_s2<MOM_STRIP_KS, 2> : mode == 3 ? k_layer_s2<MOM_STRIP_KS, 3> : k_layer_s2<MOM_STRIP_KS, 0>;
  return mom_with_int<0, kSkipVariants - 1>(v, [&](auto V) {
    return mom_with_bool(rb, [&](auto RB) {
      return mom_with_bool(src, [&](auto SRC) {
        return mom_with_bool(el, [&](auto EL) -> LayerKernel {
          constexpr int KW = MOM_STRIP_KS - kS2Skip[V];
          constexpr bool RBK = RB && s2_row_blocks_change(MOM_STRIP_KS, KW);
          return k_layer_s2<MOM_STRIP_KS, 1, KW, RBK, SRC, EL>;
        });
      });
    });
  });
}
static hipError_t image_launch(const void *layer_args, const MomLaunchForm &f, int grid, hipStream_t st) {
  const LayerKernel k = s2_kernel(f.sched_mode & 3, mom_skip_variant(kS2Skip, MOM_STRIP_KS, f.nbw), s2_row_blocks_for(MOM_STRIP_KS, f),
                                  f.sources_only, f.elemental_tab);
  return mom_launch_lds(k, grid, kThreads, s2_lds_bytes(4 * MOM_STRIP_KS), st, *reinterpret_cast<const LayerArgs *>(layer_args));
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
