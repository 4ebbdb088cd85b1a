// tools/strip2_variant_check.hip -- host-only check of s2_variant_for (mom_strip2_variants.hpp): the instantiation of the two-buffer
// strip image a launch takes for LayerArgs::nbw under MOM_OPT_ZERO_SKIP bit 1.  Expected: the largest instantiated skip (0 .. 3
// k-steps) that still keeps every block of four entries with a weighted one, and no skip for nbw = 0 or nbw > KS.  Built and run by
// tests/test_gpu_strip_zero_skip.py.  Prints one line per case; exit code 1 on a mismatch.
#include <cstdio>

#include "mom_strip2_variants.hpp"

static int check(int KS, int nbw, int skip) {
  const int v = s2_variant_for(KS, nbw);
  const bool ok = v >= 0 && v < kS2Variants && kS2Skip[v] == skip && (skip == 0 || KS - skip >= nbw);
  printf("KS = %2d nbw = %2d: variant %d, skip %d (%d) %s\n", KS, nbw, v, (v >= 0 && v < kS2Variants) ? kS2Skip[v] : -1, skip, ok ? "ok" : "WRONG");
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
