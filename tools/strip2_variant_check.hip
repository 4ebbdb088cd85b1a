// tools/strip2_variant_check.hip -- host-only check of s2_variant_for and s2_row_blocks_for (mom_strip2_variants.hpp): the instantiation
// of the two-buffer strip image a launch takes for LayerArgs::nbw under MOM_OPT_ZERO_SKIP bits 1 and 2.  Expected: the largest
// instantiated skip (0 .. 3 k-steps) that still keeps every block of four entries with a weighted one, and no skip for nbw = 0 or
// nbw > KS; the row-block kernel (RB) never without the flag kS2RowBlocks, and with it exactly where some block of four rows of the
// 4 NT of a strip is neither weighted (< KS - skip) nor the riding block (KS) -- counted here block by block; the flag must not
// change the skip.  Built and run by tests/test_gpu_strip_zero_skip.py.  Prints one line per case; exit code 1 on a mismatch.
#include <cstdio>

#include "mom_strip2_variants.hpp"

static int check(int KS, int nbw, int skip) {
  const int v = s2_variant_for(KS, nbw);
  bool ok = v >= 0 && v < kS2Variants && kS2Skip[v] == skip && (skip == 0 || KS - skip >= nbw);
  int idle = 0;  // blocks of four rows the rule leaves out
  for (int bi = 0; bi < 4 * ((KS + 3) / 4); ++bi)
    if (!(bi < KS - skip || bi == KS)) ++idle;
  const bool rb = s2_row_blocks_for(KS, nbw | kS2RowBlocks);
  ok = ok && !s2_row_blocks_for(KS, nbw) && rb == (idle > 0) && s2_variant_for(KS, s2_nbw_count(nbw | kS2RowBlocks)) == v &&
       s2_row_blocks_change(KS, KS - skip) == rb;
  printf("KS = %2d nbw = %2d: variant %d, skip %d (%d), row blocks %d (%d idle) %s\n", KS, nbw, v,
         (v >= 0 && v < kS2Variants) ? kS2Skip[v] : -1, skip, (int)rb, idle, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  for (int KS = 13; KS <= 15; ++KS) {
    bad += check(KS, 0, 0);       // MOM_OPT_ZERO_SKIP without bit 1, or no count
    bad += check(KS, KS + 1, 0);  // out of range
    bad += check(KS, KS - 4, 3);  // more zero blocks than the largest instantiated skip: still exact with 3
    bad += check(KS, KS - 3, 3);
    bad += check(KS, KS - 2, 2);
    bad += check(KS, KS - 1, 1);
    bad += check(KS, KS, 0);
  }
  return bad ? 1 : 0;
}
