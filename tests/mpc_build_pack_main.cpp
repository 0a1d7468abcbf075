// Stand-alone driver of pack_mpc_build_unit (nk_mpc_build_pack.h) for tests/test_mpc_build_pack_host.py.  Standard input: one
// unit per line, "m p N nc Ny host_ops have_R have_P want_P host_C extra_ld".  The operands of unit u have the leading
// dimension cols + extra_ld; entry (r, c) of piece k holds value(u, k, r cols + c) = 1 + 100000 u + 10000 k + (r cols + c),
// pieces: 0 = A, 1 = B, 2 = Q, 3 = R, 4 = P, 5 = C_rows, and the entries between the rows hold -1.  The program prints one
// line of offsets per unit (-1: the unit has no such piece), the three totals (in, out, ws), and the block of the staging
// pack as hexadecimal floats (exact, the sign of a zero included).
#include <cstdio>
#include <vector>

#include "nk_mpc_build_pack.h"

int main() {
  nk::UnitPack in, out, ws;
  std::vector<std::vector<double>> keep;  // the sources are read by block()
  size_t unit = 0;
  auto make = [&](int piece, size_t rows, size_t cols, size_t extra) {
    std::vector<double> v(rows * (cols + extra), -1.0);
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < cols; ++c) v[r * (cols + extra) + c] = 1.0 + 100000.0 * (double)unit + 10000.0 * piece + (double)(r * cols + c);
    keep.push_back(v);
    return keep.back().data();
  };
  auto show = [](size_t o) { return o == nk::MPC_BUILD_NONE ? -1ll : (long long)o; };
  size_t m, p, N, nc, Ny, extra;
  int host_ops, have_R, have_P, want_P, host_C;
  while (std::scanf("%zu %zu %zu %zu %zu %d %d %d %d %d %zu", &m, &p, &N, &nc, &Ny, &host_ops, &have_R, &have_P, &want_P,
                    &host_C, &extra) == 11) {
    nk::MpcBuildShape s;
    s.m = m; s.p = p; s.N = N; s.nc = nc; s.Ny = Ny;
    s.host_ops = host_ops != 0; s.have_R = have_R != 0; s.have_P = have_P != 0; s.want_P = want_P != 0; s.host_C = host_C != 0;
    const double* A = s.host_ops ? make(0, m, m, extra) : nullptr;
    const double* B = s.host_ops ? make(1, m, p, extra) : nullptr;
    const double* Q = s.host_ops ? make(2, m, m, extra) : nullptr;
    const double* R = s.have_R ? make(3, p, p, extra) : nullptr;
    const double* P = s.have_P ? make(4, m, m, extra) : nullptr;
    const double* C = (s.host_C && nc) ? make(5, nc, m, extra) : nullptr;
    const nk::MpcBuildOffsets o = nk::pack_mpc_build_unit(in, out, ws, s, A, m + extra, B, p + extra, Q, m + extra, R, p + extra,
                                                          P, m + extra, C, m + extra);
    std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", show(o.A), show(o.B),
                show(o.Q), show(o.R), show(o.P), show(o.C), show(o.H), show(o.F), show(o.K), show(o.outP), show(o.G), show(o.T),
                show(o.rK), show(o.rP), show(o.sq), show(o.wide));
    ++unit;
  }
  std::printf("%zu %zu %zu\n", in.doubles(), out.doubles(), ws.doubles());
  const double* b = in.block();
  for (size_t i = 0; i < in.doubles(); ++i) std::printf("%a%c", b[i], i + 1 < in.doubles() ? ' ' : '\n');
  if (in.doubles() == 0) std::printf("\n");
  return 0;
}
