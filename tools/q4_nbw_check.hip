// tools/q4_nbw_check.hip -- host-only check of mom_q4_nbw / mom_weighted_edge (mom_host.hpp): the number of blocks of four entries
// that hold a weighted stream entry, which MOM_OPT_ZERO_SKIP hands to the quad-block image.  Only a TRAILING run of weights that
// are exactly 0.0 counts.  Built and run by tests/test_gpu_q4_zero_skip.py.  Prints one line per case; exit code 1 on a mismatch.
#include <cstdio>
#include <vector>

#include "mom_host.hpp"

static int check(const char *what, const std::vector<double> &wt, int edge, int nbw) {
  const int e = mom_weighted_edge(wt.data(), (int)wt.size()), b = mom_q4_nbw(wt.data(), (int)wt.size());
  const bool ok = (e == edge && b == nbw);
  printf("%-44s N=%2d weighted edge %2d (%2d) nbw %2d (%2d) %s\n", what, (int)wt.size(), e, edge, b, nbw, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  std::vector<double> w(40, 0.05);
  bad += check("no zero weight", w, 40, 10);
  for (int i = 37; i < 40; ++i) w[i] = 0.0;
  bad += check("3 trailing zeros", w, 37, 10);
  w[36] = 0.0;
  bad += check("4 trailing zeros: one block free", w, 36, 9);
  w[36] = 1.e-9;  // below the kernel's 1e-8 test, but not exactly zero: it ends the run
  bad += check("a tiny weight is not a zero", w, 37, 10);
  w[36] = 0.0;
  w[10] = 0.0;
  bad += check("a zero between weighted entries", w, 36, 9);
  // the headline's sub-problem: 17 Gauss nodes x (I,Q), then three view angles and the Sun x (I,Q)
  std::vector<double> c2(40, 0.0);
  for (int i = 0; i < 34; ++i) c2[i] = 0.03;
  bad += check("N0 = 40, 34 weighted: block 8 mixed", c2, 34, 9);
  // IQUV, 15 streams: 11 nodes x (I,Q) = 22 weighted, 8 zero-weight entries, one dummy stream (two entries) to N0 = 32
  std::vector<double> p(30, 0.0);
  for (int i = 0; i < 22; ++i) p[i] = 0.04;
  p.resize(32, 0.0);
  bad += check("N0 = 30 + 2 dummy entries, 22 weighted", p, 22, 6);
  bad += check("no weighted entry: at least one block", std::vector<double>(20, 0.0), 0, 1);
  return bad ? 1 : 0;
}
