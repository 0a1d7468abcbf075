// Stand-alone driver of pack_mpc_out_unit (nk_unit_pack.h) for tests/test_mpc_out_unit_pack_host.py.  Standard input: one
// unit per line, "m nv ny d p fold has_u_init" (fold = 0: a spline model, [F; T] dense m x nt); m = 0: a unit that shares the
// prepared pieces of the unit before it (pack_mpc_out_unit_state: its own x0, x_ref, u_init alone).  The operands of unit u
// are filled with value(u, piece, i) = 1 + 100000 u + 10000 piece + i, pieces: 0 = the constants [Kb | S0' | lo hi dlo dhi
// ycomp], 1 = [F; T], 2 = x0, 3 = x_ref, 4 = u_init.  The program prints one line of offsets per unit, the two totals, and
// the block of the staging pack as hexadecimal floats (exact, the sign of a zero included).
#include <cstdio>
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
  size_t m = 0, nv = 0, ny = 0, d = 0, p = 0, unit = 0;
  int fold = 0, has_u = 0;
  nk::MpcOutUnitOffsets last;
  while (std::scanf("%zu %zu %zu %zu %zu %d %d", &m, &nv, &ny, &d, &p, &fold, &has_u) == 7) {
    if (m == 0) {
      const double *x0 = make(unit, 2, d), *xr = make(unit, 3, d), *ui = has_u ? make(unit, 4, p) : nullptr;
      nk::pack_mpc_out_unit_state(in, last, x0, xr, ui, d, p);
      std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", last.Kb, last.S0t, last.bnd, last.FT, last.x0, last.x_ref,
                  last.u_init, last.w, (size_t)0);
      ++unit;
      continue;
    }
    const size_t nt = nv + ny;
    const double *c = make(unit, 0, nt * nt + nv * nt + 5 * nt), *FT = make(unit, 1, m * nt), *x0 = make(unit, 2, d),
                 *xr = make(unit, 3, d);
    const double* ui = has_u ? make(unit, 4, p) : nullptr;
    const nk::MpcOutUnitOffsets o = last = nk::pack_mpc_out_unit(in, dev, c, FT, x0, xr, ui, m, nv, ny, d, p, fold != 0);
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", o.Kb, o.S0t, o.bnd, o.FT, o.x0, o.x_ref, o.u_init, o.w,
                nk::gain_row_reserve(m));
    ++unit;
  }
  std::printf("%zu %zu\n", in.doubles(), dev.doubles());
  const double* b = in.block();
  for (size_t i = 0; i < in.doubles(); ++i) std::printf("%a%c", b[i], i + 1 < in.doubles() ? ' ' : '\n');
  return 0;
}
