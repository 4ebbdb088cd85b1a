// mom_image_variants.hpp -- which instantiation of the two-buffer strip image's and the quad-block image's kernel a launch takes for its
// MomLaunchForm (host only; no kernel code, so that tools/image_variant_check.hip can test the choice on its own).
//
// MOM_OPT_ZERO_SKIP bits 0 and 1: the stream entries from 4 nbw on (MomLaunchForm::nbw) are zero-weight streams.  The quad-block image
// k_layer_q4<KS, NBW> multiplies NBW = KS - kQ4Skip[v] block rows (mom_q4.hpp q4_mul_c), the two-buffer image k_layer_s2<KS, 1, KW> runs
// KW = KS - kS2Skip[v] k-steps per strip product (mom_strip.hpp strip_mul).  Any NBW, KW >= nbw is exact, and a rule for FEWER zero
// blocks than the problem has is still exact: a launch takes the largest instantiated skip with KS - skip >= nbw.
// rt_set_streams gives: IQU with three view angles and the Sun KS - 2; IQUV of 13 .. 15 streams and IQU with four view angles KS - 3;
// IQU with one view angle KS - 1; the scalar 60-stream scene KS (no skip).
//
// MOM_OPT_ZERO_SKIP bit 2: the row-block rule (mom_strip.hpp strip_mul<KS, KW, RB>), MomLaunchForm::row_blocks.
// k_layer_s2<KS, 1, KW, true> exists where the rule changes a row tile, i.e. where a block of four rows is a passenger (KW < KS) or
// dead (past the riding block KS): everywhere but (KS = 15, KW = 15).
#pragma once
#include "mom_images.hpp"

constexpr int kSkipVariants = 4;
constexpr int kS2Skip[kSkipVariants] = {0, 1, 2, 3};
constexpr int kQ4Skip[kSkipVariants] = {0, 1, 2, 4};

// index into `skip` for nbw blocks of four entries that hold a weighted one; 0 (nothing left out) if nbw is 0 or out of range
inline int mom_skip_variant(const int (&skip)[kSkipVariants], int KS, int nbw) {
  if (nbw < 1 || nbw > KS) return 0;
  int v = 0;
  for (int c = 1; c < kSkipVariants; ++c)
    if (KS - skip[c] >= nbw) v = c;
  return v;
}
// does the row-block rule change a product of KW k-steps: is some block row 0 .. 4 NT - 1 neither < KW nor the riding block KS?
constexpr bool s2_row_blocks_change(int KS, int KW) { return KW < KS || 4 * ((KS + 3) / 4) - 1 > KS; }
// the RB a launch takes: the option, where the rule changes the variant the count selects
inline bool s2_row_blocks_for(int KS, const MomLaunchForm &f) {
  return f.row_blocks && s2_row_blocks_change(KS, KS - kS2Skip[mom_skip_variant(kS2Skip, KS, f.nbw)]);
}
