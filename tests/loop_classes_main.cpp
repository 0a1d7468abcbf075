// Stand-alone driver of nk_loop_classes.h for tests/test_loop_classes_host.py.  Standard input holds problems, each
//   "n with_lds" and then n records "ktype shape waves" (with_lds = 1: "ktype shape waves lds"),
// and for each the program prints
//   "perm p_0 .. p_{n-1}"                      the stable permutation (sorted position -> the caller's index)
//   "run begin end ktype shape waves lds"      one line per run of equal keys, in order (lds = 0 without needs)
//   "end"
#include <cstdio>
#include <vector>

#include "nk_loop_classes.h"

int main() {
  int n, with_lds;
  while (std::scanf("%d %d", &n, &with_lds) == 2) {
    if (n < 1) return 2;
    std::vector<nk::LoopClass> keys((size_t)n);
    std::vector<long> lds((size_t)n, 0L);
    for (int u = 0; u < n; ++u) {
      if (std::scanf("%d %d %d", &keys[(size_t)u].ktype, &keys[(size_t)u].shape, &keys[(size_t)u].waves) != 3) return 3;
      if (with_lds && std::scanf("%ld", &lds[(size_t)u]) != 1) return 3;
    }
    const nk::LoopClassPlan plan = nk::plan_loop_classes(keys.data(), n, with_lds ? lds.data() : nullptr);
    std::printf("perm");
    for (int p : plan.perm) std::printf(" %d", p);
    std::printf("\n");
    for (const nk::LoopRun& r : plan.runs)
      std::printf("run %d %d %d %d %d %ld\n", r.begin, r.end, r.key.ktype, r.key.shape, r.key.waves, r.lds);
    std::printf("end\n");
  }
  return 0;
}
