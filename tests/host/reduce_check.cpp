// reduce_check.cpp -- the m = 0 reduction of csrc/mom_reduce.hpp as a stand-alone host program (tests/test_host_reduce.py
// builds it with the host compiler and the address / undefined-behaviour sanitizers, and compares its output with numpy).
// stdin:  N nS K M N0 | I0[4] | mu[N] | wt[N] | Zpp[N,N,K,M] | Zmp[N,N,K,M] | Rsurf[N,N]      (column-major, whitespace-separated)
// stdout: "reducible b", then the cut for N0 ("mu", "wt", "sg", "Zpp", "Zmp": one line each), "brdf b", "r0"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "mom_reduce.hpp"

static std::vector<double> read(size_t n) {
  std::vector<double> v(n);
  for (double &x : v)
    if (!(std::cin >> x)) { std::fprintf(stderr, "reduce_check: short input\n"); std::exit(2); }
  return v;
}
static void show(const char *name, const std::vector<double> &v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %.17g", x);
  std::printf("\n");
}

int main() {
  int N, nS, K, M, N0;
  if (!(std::cin >> N >> nS >> K >> M >> N0)) return 2;
  const std::vector<double> I0 = read(4), mu = read(N), wt = read(N);
  const std::vector<double> Zpp = read((size_t)N * N * K * M), Zmp = read((size_t)N * N * K * M), Rsurf = read((size_t)N * N);
  std::printf("reducible %d\n", mom_m0_reducible(I0.data(), N, nS, K, Zpp.data(), Zmp.data()) ? 1 : 0);
  const MomM0Cut c = mom_m0_cut(mu.data(), wt.data(), N, nS, K, N0, Zpp.data(), Zmp.data());
  show("mu", c.mu); show("wt", c.wt); show("sg", c.sg); show("Zpp", c.Zpp); show("Zmp", c.Zmp);
  std::vector<double> r0;
  std::printf("brdf %d\n", mom_m0_cut_brdf(Rsurf.data(), N, nS, N0, r0) ? 1 : 0);
  show("r0", r0);
  return 0;
}
