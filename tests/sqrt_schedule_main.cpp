// Stand-alone driver of nk_sqrt_schedule.h for tests/test_sqrt_schedule_host.py: reads "estimate true_lower_bound" pairs
// from standard input and prints, per pair, three lines: kmax, then s2[0 .. kmax-1] (hexadecimal floats: exact), then
// check[0 .. kmax-1] as 0 / 1.  With an argument it prints the other functions of the header (tests/test_sqrtm_reference_host.py):
// "estimate" reads "fro trace m" triples and prints ns_interval_estimate; "host" reads "a steps" pairs and prints the scales
// s2 of the host-checked recurrence (ns_scale, then ns_advance with the upper end b carried) on one line.
#include <cstdio>
#include <cstring>

#include "nk_sqrt_schedule.h"

int main(int argc, char** argv) {
  double a = 0.0, lower = 0.0;
  if (argc > 1 && std::strcmp(argv[1], "estimate") == 0) {
    double fro = 0.0, tr = 0.0;
    int m = 0;
    while (std::scanf("%lf %lf %d", &fro, &tr, &m) == 3) std::printf("%a\n", nk::ns_interval_estimate(fro, tr, m));
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) {
    int steps = 0;
    while (std::scanf("%lf %d", &a, &steps) == 2) {
      double b = 1.0;
      for (int k = 0; k < steps; ++k) {
        const double s2 = nk::ns_scale(a, b);
        nk::ns_advance(s2, a, b);
        std::printf("%a%c", s2, k + 1 < steps ? ' ' : '\n');
      }
    }
    return 0;
  }
  while (std::scanf("%lf %lf", &a, &lower) == 2) {
    const nk::NsSchedule sch = nk::ns_queued_schedule(a, lower);
    std::printf("%d\n", sch.kmax);
    for (int k = 0; k < sch.kmax; ++k) std::printf("%a%c", sch.s2[k], k + 1 < sch.kmax ? ' ' : '\n');
    for (int k = 0; k < sch.kmax; ++k) std::printf("%d%c", sch.check[k] ? 1 : 0, k + 1 < sch.kmax ? ' ' : '\n');
  }
  return 0;
}
