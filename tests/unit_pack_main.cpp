// Stand-alone driver of nk_unit_pack.h for tests/test_unit_pack_host.py.  Standard input: one unit per line,
//   "plant m d fold"   or   "loop m p d steps has_target has_u_init"   (all units of a run are of one kind).
// The operands of unit u are filled with value(u, piece, i) = 1 + 100000 u + 10000 piece + i (pieces in the order of the
// layout), packed with pack_plant_unit / pack_loop_unit, and the program prints one line of offsets per unit, the two
// totals, and the block of the staging pack as hexadecimal floats (exact, the sign of a zero included).
#include <cstdio>
#include <cstring>
#include <vector>

#include "nk_unit_pack.h"

static std::vector<double> values(size_t unit, int piece, size_t count) {
  std::vector<double> v(count);
  for (size_t i = 0; i < count; ++i) v[i] = 1.0 + 100000.0 * (double)unit + 10000.0 * piece + (double)i;
  return v;
}

int main() {
  nk::UnitPack in, dev;
  std::vector<std::vector<double>> keep;  // the sources are read by block()
  auto make = [&](size_t unit, int piece, size_t count) {
    keep.push_back(values(unit, piece, count));
    return keep.back().data();
  };
  char kind[16];
  size_t unit = 0;
  while (std::scanf("%15s", kind) == 1) {
    if (std::strcmp(kind, "plant") == 0) {
      size_t m = 0, d = 0;
      int fold = 0;
      if (std::scanf("%zu %zu %d", &m, &d, &fold) != 3) return 2;
      const double *K = make(unit, 0, m), *x0 = make(unit, 1, d), *xr = make(unit, 2, d);
      const nk::PlantUnitOffsets o = nk::pack_plant_unit(in, dev, K, x0, xr, m, d, fold != 0);
      std::printf("%zu %zu %zu %zu %zu\n", o.K, o.x0, o.x_ref, o.w, nk::gain_row_reserve(m));
    } else if (std::strcmp(kind, "loop") == 0) {
      size_t m = 0, p = 0, d = 0, steps = 0;
      int has_target = 0, has_u = 0;
      if (std::scanf("%zu %zu %zu %zu %d %d", &m, &p, &d, &steps, &has_target, &has_u) != 6) return 2;
      const double *K = make(unit, 0, p * m), *f0 = make(unit, 1, m), *fr = make(unit, 2, m);
      const double* tg = has_target ? make(unit, 3, d) : nullptr;
      const double* ui = has_u ? make(unit, 4, p) : nullptr;
      const nk::LoopUnitOffsets o = nk::pack_loop_unit(in, dev, K, f0, fr, tg, ui, m, p, d, steps);
      std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", o.K, o.phi0, o.phi_ref, o.target, o.u_init, o.Phi, o.usq, o.sse);
    } else {
      return 2;
    }
    ++unit;
  }
  std::printf("%zu %zu\n", in.doubles(), dev.doubles());
  const double* b = in.block();
  for (size_t i = 0; i < in.doubles(); ++i) std::printf("%a%c", b[i], i + 1 < in.doubles() ? ' ' : '\n');
  return 0;
}
