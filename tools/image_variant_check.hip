// tools/image_variant_check.hip -- host-only check of mom_skip_variant and s2_row_blocks_for (mom_image_variants.hpp): the instantiation
// of the two-buffer strip image and of the quad-block image a launch takes for its MomLaunchForm under MOM_OPT_ZERO_SKIP.  Expected: the
// largest instantiated skip (two-buffer: 0 .. 3 k-steps, quad-block: 0, 1, 2, 4 block rows) that still keeps every block of four
// entries with a weighted one, and no skip for nbw = 0 or nbw > KS; the two-buffer image's row-block kernel (RB) never without
// MomLaunchForm::row_blocks, and with it exactly where some block of four rows of the 4 NT of a strip is neither weighted
// (< KS - skip) nor the riding block (KS) -- counted here block by block; row_blocks must not change the skip.  Built and run by
// tests/test_gpu_strip_zero_skip.py.  Prints one line per case; exit code 1 on a mismatch.
#include <cstdio>

#include "mom_image_variants.hpp"

static int check_s2(int KS, int nbw, int skip) {
  MomLaunchForm f, frb;
  f.nbw = frb.nbw = nbw;
  frb.row_blocks = true;
  const int v = mom_skip_variant(kS2Skip, KS, f.nbw);
  bool ok = v >= 0 && v < kSkipVariants && kS2Skip[v] == skip && (skip == 0 || KS - skip >= nbw);
  int idle = 0;  // blocks of four rows the rule leaves out
  for (int bi = 0; bi < 4 * ((KS + 3) / 4); ++bi)
    if (!(bi < KS - skip || bi == KS)) ++idle;
  const bool rb = s2_row_blocks_for(KS, frb);
  ok = ok && !s2_row_blocks_for(KS, f) && rb == (idle > 0) && mom_skip_variant(kS2Skip, KS, frb.nbw) == v &&
       s2_row_blocks_change(KS, KS - skip) == rb;
  printf("two-buffer KS = %2d nbw = %2d: variant %d, skip %d (%d), row blocks %d (%d idle) %s\n", KS, nbw, v,
         (v >= 0 && v < kSkipVariants) ? kS2Skip[v] : -1, skip, (int)rb, idle, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}

static int check_q4(int KS, int nbw, int skip) {
  const int v = mom_skip_variant(kQ4Skip, KS, nbw);
  const bool ok = v >= 0 && v < kSkipVariants && kQ4Skip[v] == skip && (skip == 0 || KS - skip >= nbw);
  printf("quad-block KS = %2d nbw = %2d: variant %d, skip %d (%d) %s\n", KS, nbw, v, (v >= 0 && v < kSkipVariants) ? kQ4Skip[v] : -1,
         skip, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  for (int KS = 13; KS <= 15; ++KS) {
    bad += check_s2(KS, 0, 0);       // MOM_OPT_ZERO_SKIP without bit 1, or no count
    bad += check_s2(KS, KS + 1, 0);  // out of range
    bad += check_s2(KS, KS - 4, 3);  // more zero blocks than the largest instantiated skip: still exact with 3
    bad += check_s2(KS, KS - 3, 3);
    bad += check_s2(KS, KS - 2, 2);
    bad += check_s2(KS, KS - 1, 1);
    bad += check_s2(KS, KS, 0);
  }
  for (int KS = 5; KS <= 10; ++KS) {
    bad += check_q4(KS, 0, 0);       // MOM_OPT_ZERO_SKIP without bit 0, or no count
    bad += check_q4(KS, KS + 1, 0);  // out of range
    bad += check_q4(KS, KS, 0);
    bad += check_q4(KS, KS - 1, 1);
    bad += check_q4(KS, KS - 2, 2);
    bad += check_q4(KS, KS - 3, 2);  // no instantiation leaves out three block rows: still exact with 2
    bad += check_q4(KS, KS - 4, 4);
    if (KS - 5 >= 1) bad += check_q4(KS, KS - 5, 4);  // more zero blocks than the largest instantiated skip
  }
  return bad ? 1 : 0;
}
