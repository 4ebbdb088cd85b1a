// mom_strip2_variants.hpp -- which instantiation of the two-buffer strip image's kernel a launch takes (host only; no kernel code, so
// that tools/strip2_variant_check.hip can test the choice on its own).
//
// MOM_OPT_ZERO_SKIP bit 1: k_layer_s2<KS, 1, KW> runs KW = KS - kS2Skip[v] k-steps per strip product (mom_strip.hpp strip_mul).  The
// stream entries from 4 nbw on (LayerArgs::nbw) are zero-weight streams, so any KW >= nbw is exact, and a rule for FEWER skipped
// k-steps than the problem allows is still exact: a launch takes the largest instantiated skip with KS - skip >= nbw.
// rt_set_streams gives: IQU with three view angles and the Sun KS - 2; IQUV of 13 .. 15 streams and IQU with four view angles KS - 3;
// IQU with one view angle KS - 1; the scalar 60-stream scene KS (no skip).
#pragma once

constexpr int kS2Skip[] = {0, 1, 2, 3};
constexpr int kS2Variants = (int)(sizeof kS2Skip / sizeof kS2Skip[0]);

// index into kS2Skip for nbw blocks of four entries that hold a weighted one; 0 (every k-step) if nbw is 0 or out of range
inline int s2_variant_for(int KS, int nbw) {
  if (nbw < 1 || nbw > KS) return 0;
  int v = 0;
  for (int c = 1; c < kS2Variants; ++c)
    if (KS - kS2Skip[c] >= nbw) v = c;
  return v;
}
