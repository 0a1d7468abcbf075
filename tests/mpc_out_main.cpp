// Stand-alone driver of nk_mpc_out.h for tests/test_mpc_out_host.py: nothing of the GPU is included.  Standard input: one case
// after another,
//   "N p m iters rho tol ny y_weight"  then  15 counts (how many numbers follow per array; 0 = a NULL pointer)
//   then the arrays in that order: H, F, lo, hi, dlo, dhi, K, G, T, ylo, yhi, ycomp, e, x_ref, u_prev
// (floating-point numbers as strtod reads them: hexadecimal floats, "nan", "inf"; ycomp as integers written the same way).
// Every case goes through the validation and, when the pair of descriptions is valid, through one solve.  Output, one line
// per case:  "ok u (p) | z (nv + ny) | iterations residual"  (hexadecimal floats)  or  "bad <message>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nk_mpc_out.h"

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
    nk_mpc_out out = {};
    ds.N = N; ds.p = p; ds.m = m; ds.iters = iters;
    if (!read_double(&ds.rho) || !read_double(&ds.tol)) return 2;
    if (std::scanf("%d", &out.ny) != 1 || !read_double(&out.y_weight)) return 2;
    constexpr int NA = 15;
    int cnt[NA];
    std::vector<double> arr[NA];
    for (int& c : cnt)
      if (std::scanf("%d", &c) != 1 || c < 0 || c > (1 << 20)) return 2;
    for (int a = 0; a < NA; ++a) {
      arr[a].resize((size_t)cnt[a]);
      for (double& v : arr[a])
        if (!read_double(&v)) return 2;
    }
    auto ptr = [&](int a) -> const double* { return cnt[a] ? arr[a].data() : nullptr; };
    ds.H = ptr(0); ds.F = ptr(1); ds.lo = ptr(2); ds.hi = ptr(3); ds.dlo = ptr(4); ds.dhi = ptr(5); ds.K = ptr(6);
    out.G = ptr(7); out.T = ptr(8); out.ylo = ptr(9); out.yhi = ptr(10);
    std::vector<int32_t> yc(arr[11].begin(), arr[11].end());
    out.ycomp = cnt[11] ? yc.data() : nullptr;
    char msg[200];
    // the output arrays have exactly the sizes the interface promises for a VALID pair: a write past them is reported
    const bool sizes_ok = p >= 1 && p <= nk::MPC_MAX_P && N >= 1 && (long)N * p <= NK_MPC_MAX_NV && out.ny >= 1 &&
                          (long)N * p + out.ny <= NK_MPC_MAX_NV;
    std::vector<double> u((size_t)(sizes_ok ? p : 1)), z((size_t)(sizes_ok ? N * p + out.ny : 1));
    double info[2] = {-1.0, -1.0};
    if (nk::mpc_out_qp_host(&ds, &out, ptr(12), ptr(13), ptr(14), u.data(), z.data(), info, msg, sizeof msg) != 0) {
      std::printf("bad %s\n", msg);
      continue;
    }
    std::printf("ok");
    for (double v : u) std::printf(" %a", v);
    std::printf(" |");
    for (double v : z) std::printf(" %a", v);
    std::printf(" | %a %a\n", info[0], info[1]);
  }
  return 0;
}
