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

// What the host knows about a launch and no kernel reads: which of the instantiations an image holds the launch takes
// (mom_image_variants.hpp has the rules).  An image ignores what it has no instantiation for; a default-constructed form is the
// plain kernel, which is what the finishers and the Float32 driver pass.
struct MomLaunchForm {
  // MOM_OPT_ZERO_SKIP: block rows of four entries that hold a weighted stream entry (mom_host.hpp mom_q4_nbw) -- the entries from
  // 4 nbw on are zero-weight streams, whose exact-zero blocks (quad-block image) or k-steps (two-buffer strip image) the products
  // leave out; 0 (or N / 4): no such rule
  int nbw = 0;
  bool row_blocks = false;     // MOM_OPT_ZERO_SKIP bit 2: the row-block rule of the two-buffer strip image (mom_strip.hpp strip_mul)
  // MOM_OPT_SOURCES_ONLY: no caller can observe a moment of this launch; the two-buffer strip image and the quad-block image then
  // leave the composite R-+ and T++ out (mom_strip2.hpp)
  bool sources_only = false;
  // MOM_OPT_ELEMENTAL: the table form of the elemental layer (mom_elemental_tab.hpp; the two-buffer strip image in its default
  // scheduling mode and the quad-block image); the host sets it only together with LayerArgs::etab
  bool elemental_tab = false;
  int sched_mode = 0;          // MOM_OPT_STRIP2_SCHED: the scheduling mode of the two-buffer strip image (mom_strip2.hpp), 1 = default
};

struct MomLayerImage {
  int N;  // operator edge the image was compiled for
  // layer_args: the LayerArgs of the image's build (layout-identical in every namespace of a precision); the finishers read the
  // interface code their kernel is instantiated for from it (LayerArgs::iface; the first-stage images handle code 3 only).  The
  // dynamic LDS size is the image's own business
  hipError_t (*launch)(const void *layer_args, const MomLaunchForm &form, int grid, hipStream_t st);
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

// ints of LayerArgs::sched of the two-buffer images (the unit queue's counter + the arrival tickets per CU: kS2SchedInts of
// mom_strip2.hpp, momcore_strip2.hip checks the two against each other), zeroed on the stream before each of their launches
constexpr size_t kMomStrip2SchedInts = 1 + 2048;
