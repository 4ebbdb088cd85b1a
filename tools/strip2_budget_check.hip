// tools/strip2_budget_check.hip -- host-only check of the two-buffer strip image's LDS budget (mom_strip2.hpp): for every edge
// N = 52, 56, 60 and every number of Stokes components per stream ns that divides N, where s2_applies admits the image, two
// workgroups (image + 1 KB allowance each) must fit the CU's 160 KiB and the elemental tables at the front of t's buffer must end
// below the first t entry elemental_build<true> stores directly.  Built by tests/test_gpu_strip2.py with the image's flags
// (-DMOM_WAVES=4 -DMOM_TJ=4 -DMOM_NO_STRAIGHT -DMOM_NS=mom2).  Prints one line per (N, ns); exit code 1 on a violation.
#include <hip/hip_runtime.h>
#include <cstdio>

#include "mom_strip2.hpp"

using namespace MOM_NS;

int main() {
  int bad = 0;
  const int sizes[] = {52, 56, 60};
  for (int N : sizes)
    for (int ns = 1; ns <= 4; ++ns) {
      if (N % ns != 0) continue;
      const bool on = s2_applies(N, ns, ns);
      const size_t img = s2_lds_bytes(N);
      const int tab = s2_table_reals(N, ns, ns), direct = s2_direct_offset(N);
      const bool ok = !on || (2 * (img + 1024) <= kLdsPerCU && tab <= direct && (size_t)tab <= mat_elems(N));
      printf("N=%d ns=%d image=%zu two=%zu tables=%d direct=%d %s %s\n", N, ns, img, 2 * (img + 1024), tab, direct,
             on ? "admitted" : "8-wave-only", ok ? "ok" : "OVER");
      bad += !ok;
    }
  return bad ? 1 : 0;
}
