// mom_images.hpp -- the table of layer-kernel images (host only).
//
// An IMAGE is a layer kernel compiled for ONE operator edge N = 4 KS and one workgroup shape, in an object of its own
// (momcore_strip.hip, momcore_strip2.hip, momcore_lean6.hip, momcore_q4.hip; one Makefile rule per family).  Each object
// defines one MomLayerImage per image it holds; MOM_IMAGE_LIST below enumerates them.  The launch path (momcore.hip:
// launch_layer, momcore_f32.hip: momf_rt_run) asks mom_find_image(family, N) and knows no size by name.
//
// To add an image: its object in the Makefile's OBJS, its line in MOM_IMAGE_LIST.  These are the only two places that name
// sizes; an entry without its object (or the reverse) fails at link time, not as a silently slower route.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

struct MomLayerImage {
  int N;  // operator edge the image was compiled for
  // layer_args: the LayerArgs of the image's build (layout-identical in every namespace of a precision); iface: the interface
  // code the kernel is instantiated for (finishers; the first-stage images handle code 3 only and ignore it).  The dynamic LDS
  // size is the image's own business
  hipError_t (*launch)(const void *layer_args, int iface, int grid, hipStream_t st);
  // LDS bytes of one workgroup for ns Stokes components per stream of the elemental layer's stream-pair tables, nS per stream
  // entry of the scene, K phase-matrix bases; 0: the image does not apply to such a scene
  size_t (*lds_bytes)(int ns, int nS, int K);
  int (*per_cu)();  // workgroups of the image one CU holds (the grid of a persistent launch is per_cu() * CUs at most)
};

// finishers run every layer of every unit that no first-stage image has completed (LayerArgs::resume); a first-stage image runs
// in front of one, on more workgroups per CU, and leaves the units (or layers) it does not handle to it
enum MomImageFamily {
  MOM_IMG_STRIP8,      // 8-wave strip-chained k_layer (mom_strip.hpp), namespace mom: finisher, one workgroup per CU
  MOM_IMG_STRIP4,      // its 4-wave build, namespace mom4: finisher, two per CU
  MOM_IMG_LEAN,        // first stage: the lean image (mom_lean.hpp; three operator buffers, 4 waves, three per CU)
  MOM_IMG_LEAN6,       // first stage: the six-wave lean image (half-strip doubling chains, two per CU)
  MOM_IMG_STRIP2,      // first stage: the two-buffer 4-wave strip image (mom_strip2.hpp, two per CU)
  MOM_IMG_QUAD,        // first stage: the quad-block image (mom_q4.hpp; one wavefront per unit, occupancy from the runtime)
  MOM_IMG_F32_STRIP8,  // Float32 builds of the strip-chained k_layer: namespace momf ...
  MOM_IMG_F32_STRIP4,  // ... and momf4 (4 waves, two per CU)
};

// X(family, KS) for every image linked into libmomcore.so (N = 4 KS); keep in step with OBJS in the Makefile
#define MOM_IMAGE_LIST(X)                                                                                \
  X(STRIP8, 11) X(STRIP8, 13) X(STRIP8, 14) X(STRIP8, 15)                                               \
  X(STRIP4, 9) X(STRIP4, 10) X(STRIP4, 11)                                                              \
  X(LEAN, 9) X(LEAN, 10)                                                                                \
  X(LEAN6, 9) X(LEAN6, 10)                                                                              \
  X(STRIP2, 13) X(STRIP2, 14) X(STRIP2, 15)                                                             \
  X(QUAD, 5) X(QUAD, 6) X(QUAD, 7) X(QUAD, 8) X(QUAD, 9) X(QUAD, 10)                                    \
  X(F32_STRIP8, 11) X(F32_STRIP8, 13) X(F32_STRIP8, 14) X(F32_STRIP8, 15)                               \
  X(F32_STRIP4, 9) X(F32_STRIP4, 10) X(F32_STRIP4, 11) X(F32_STRIP4, 13) X(F32_STRIP4, 14) X(F32_STRIP4, 15)

// The descriptor of (family, KS) is defined by the image's own object: MOM_DEFINE_IMAGE(family, KS, launch, lds_bytes, per_cu).
// (Behind a host function: a const object at namespace scope would be emitted into the device code object as well.  The
// two-step form expands macro arguments such as MOM_STRIP_KS before pasting.)
#define MOM_IMAGE_SYM_(F, KS) mom_image_##F##_##KS
#define MOM_IMAGE_SYM(F, KS) MOM_IMAGE_SYM_(F, KS)
#define MOM_DEFINE_IMAGE(F, KS, ...)                                 \
  const MomLayerImage *MOM_IMAGE_SYM(F, KS)() {                      \
    static const MomLayerImage image = {4 * (KS), __VA_ARGS__};      \
    return &image;                                                   \
  }

#define MOM_IMAGE_DECL(F, KS) const MomLayerImage *MOM_IMAGE_SYM_(F, KS)();
MOM_IMAGE_LIST(MOM_IMAGE_DECL)
#undef MOM_IMAGE_DECL

// the image of `family` for operator edge N, nullptr if there is none
inline const MomLayerImage *mom_find_image(MomImageFamily family, int N) {
  struct Entry { MomImageFamily family; const MomLayerImage *image; };
#define MOM_IMAGE_ENTRY(F, KS) {MOM_IMG_##F, MOM_IMAGE_SYM_(F, KS)()},
  static const Entry all[] = {MOM_IMAGE_LIST(MOM_IMAGE_ENTRY)};
#undef MOM_IMAGE_ENTRY
  for (const Entry &e : all)
    if (e.family == family && e.image->N == N) return e.image;
  return nullptr;
}

// MOM_OPT_SOURCES_ONLY: a flag in LayerArgs::nbw beside the count (<= 15) and the two-buffer image's kS2RowBlocks (0x100), read by
// the host only.  mom_rt_run sets it on a first-stage launch whose moments no caller can observe; the two-buffer strip image and
// the quad-block image then take their instantiation that leaves the composite R-+ and T++ out (mom_strip2.hpp)
constexpr int kMomNbwSourcesOnly = 0x200;
// MOM_OPT_ELEMENTAL: likewise a host-only flag beside the count.  The two-buffer strip image (default scheduling mode) and the
// quad-block image then take their instantiation with the table form of the elemental layer (mom_elemental_tab.hpp); the host sets
// it only together with LayerArgs::etab
constexpr int kMomNbwElemental = 0x400;

// ints of LayerArgs::sched of the two-buffer images (the unit queue's counter + the arrival tickets per CU: kS2SchedInts of
// mom_strip2.hpp, momcore_strip2.hip checks the two against each other), zeroed on the stream before each of their launches
constexpr size_t kMomStrip2SchedInts = 1 + 2048;
