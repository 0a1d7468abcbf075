// Stand-alone driver of nk_mpc.h for tests/test_mpc_host.py: nothing of the GPU is included.  Standard input: one case after
// another,
//   "N p m iters rho tol"  then  "nH nF nlo nhi ndlo ndhi nK ne nup"  (how many numbers follow per array; 0 = a NULL pointer)
//   then the arrays in that order: H, F, lo, hi, dlo, dhi, K, e, u_prev
// (floating-point numbers as strtod reads them: hexadecimal floats, "nan", "inf").  Every case goes through the validation
// and, when the description is valid, through one solve.  Output, one line per case:
//   "ok u (p) | z (nv; none for iters = 0) | iterations residual"  (hexadecimal floats)  or  "bad <message>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nk_mpc.h"

static bool read_double(double* v) {
  char tok[64];
  if (std::scanf("%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

int main() {
  int N = 0, p = 0, m = 0, iters = 0;
  while (std::scanf("%d %d %d %d", &N, &p, &m, &iters) == 4) {
    nk_mpc_desc ds = {};
    ds.N = N; ds.p = p; ds.m = m; ds.iters = iters;
    if (!read_double(&ds.rho) || !read_double(&ds.tol)) return 2;
    int cnt[9];
    std::vector<double> arr[9];
    for (int& c : cnt)
      if (std::scanf("%d", &c) != 1 || c < 0 || c > (1 << 20)) return 2;
    for (int a = 0; a < 9; ++a) {
      arr[a].resize((size_t)cnt[a]);
      for (double& v : arr[a])
        if (!read_double(&v)) return 2;
    }
    auto ptr = [&](int a) -> const double* { return cnt[a] ? arr[a].data() : nullptr; };
    ds.H = ptr(0); ds.F = ptr(1); ds.lo = ptr(2); ds.hi = ptr(3); ds.dlo = ptr(4); ds.dhi = ptr(5); ds.K = ptr(6);
    char msg[200];
    // the output arrays have exactly the sizes the interface promises for a VALID description: a write past them is reported
    const bool sizes_ok = p >= 1 && p <= nk::MPC_MAX_P && N >= 1 && (long)N * p <= NK_MPC_MAX_NV;
    std::vector<double> u((size_t)(sizes_ok ? p : 1)), z((size_t)(sizes_ok ? N * p : 1));
    double info[2] = {-1.0, -1.0};
    if (nk::mpc_qp_host(&ds, ptr(7), ptr(8), u.data(), z.data(), info, msg, sizeof msg) != 0) {
      std::printf("bad %s\n", msg);
      continue;
    }
    std::printf("ok");
    for (double v : u) std::printf(" %a", v);
    std::printf(" |");
    if (iters > 0)
      for (double v : z) std::printf(" %a", v);
    std::printf(" | %a %a\n", info[0], info[1]);
  }
  return 0;
}
