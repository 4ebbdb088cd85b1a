// mom_strip2_variants.hpp -- which instantiation of the two-buffer strip image's kernel a launch takes (host only; no kernel code, so
// that tools/strip2_variant_check.hip can test the choice on its own).
//
// MOM_OPT_ZERO_SKIP bit 1: k_layer_s2<KS, 1, KW> runs KW = KS - kS2Skip[v] k-steps per strip product (mom_strip.hpp strip_mul).  The
// stream entries from 4 nbw on (LayerArgs::nbw) are zero-weight streams, so any KW >= nbw is exact, and a rule for FEWER skipped
// k-steps than the problem allows is still exact: a launch takes the largest instantiated skip with KS - skip >= nbw.
// rt_set_streams gives: IQU with three view angles and the Sun KS - 2; IQUV of 13 .. 15 streams and IQU with four view angles KS - 3;
// IQU with one view angle KS - 1; the scalar 60-stream scene KS (no skip).
//
// MOM_OPT_ZERO_SKIP bit 2: the row-block rule (mom_strip.hpp strip_mul<KS, KW, RB>).  The host hands it to the launch as the flag
// kS2RowBlocks in LayerArgs::nbw (a host-only field: no kernel reads it); k_layer_s2<KS, 1, KW, true> exists where the rule changes
// a row tile, i.e. where a block of four rows is a passenger (KW < KS) or dead (past the riding block KS): everywhere but
// (KS = 15, KW = 15).
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

constexpr int kS2RowBlocks = 0x100;  // flag in LayerArgs::nbw beside the count (<= 15)
// the count without the flags beside it (kS2RowBlocks and, above it, MOM_OPT_SOURCES_ONLY's kMomNbwSourcesOnly and MOM_OPT_ELEMENTAL's
// kMomNbwElemental of mom_images.hpp)
inline int s2_nbw_count(int nbw) { return nbw & (kS2RowBlocks - 1); }
// does the row-block rule change a product of KW k-steps: is some block row 0 .. 4 NT - 1 neither < KW nor the riding block KS?
constexpr bool s2_row_blocks_change(int KS, int KW) { return KW < KS || 4 * ((KS + 3) / 4) - 1 > KS; }
// the RB a launch takes: the flag, where the rule changes the variant the count selects
inline bool s2_row_blocks_for(int KS, int nbw) {
  return (nbw & kS2RowBlocks) != 0 && s2_row_blocks_change(KS, KS - kS2Skip[s2_variant_for(KS, s2_nbw_count(nbw))]);
}
