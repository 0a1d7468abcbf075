// Stand-alone driver of nk_sqrt_schedule.h for tests/test_sqrt_schedule_host.py: reads "estimate true_lower_bound" pairs
// from standard input and prints, per pair, three lines: kmax, then s2[0 .. kmax-1] (hexadecimal floats: exact), then
// check[0 .. kmax-1] as 0 / 1.
#include <cstdio>

#include "nk_sqrt_schedule.h"

int main() {
  double a = 0.0, lower = 0.0;
  while (std::scanf("%lf %lf", &a, &lower) == 2) {
    const nk::NsSchedule sch = nk::ns_queued_schedule(a, lower);
    std::printf("%d\n", sch.kmax);
    for (int k = 0; k < sch.kmax; ++k) std::printf("%a%c", sch.s2[k], k + 1 < sch.kmax ? ' ' : '\n');
    for (int k = 0; k < sch.kmax; ++k) std::printf("%d%c", sch.check[k] ? 1 : 0, k + 1 < sch.kmax ? ' ' : '\n');
  }
  return 0;
}
