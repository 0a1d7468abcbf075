// Stand-alone driver of nk_gemm_plan.h for tests/test_gemm_plan_host.py.  The first argument names what to print for every
// record read from standard input, one line per record:
//   splitk    "ntiles ktiles_total num_cu"           -> the generic, fp64 TN and fp32 TN choices
//   tiles     "tri tiles_m tiles_n"                  -> tile count of one problem
//   layout    "nprob  M N tri  (nprob times)"        -> tile_begin[0..3], tiles_n of the live problems, total tiles
//   slice     "K bk splitk"                          -> k-steps, slice length
//   slab      "ntiles splitk"                        -> slab elements
//   kmat      "tiles_m tiles_n"                      -> workgroups of a kernel-matrix launch
//   resid     "splitk want_resid"                    -> slices of a launch that may need the residual partials
//   contract  "per16 offA offB lda ldb M N"          -> 1 / 0 (operands at byte offsets offA / offB of a 16-byte aligned block)
//   constants (no input)                             -> TBM TN_MAXP TILE_UNUSED
#include <cstdio>
#include <cstring>

#include "nk_gemm_plan.h"

struct Shape {
  int M, N, tri;
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char* what = argv[1];
  auto is = [&](const char* s) { return std::strcmp(what, s) == 0; };
  if (is("constants")) {
    std::printf("%d %d %d\n", nk::TBM, nk::TN_MAXP, nk::TILE_UNUSED);
  } else if (is("splitk")) {
    int ntiles, kt, cu;
    while (std::scanf("%d %d %d", &ntiles, &kt, &cu) == 3)
      std::printf("%d %d %d\n", nk::plan_splitk_generic(ntiles, kt, cu), nk::plan_splitk_tn_f64(ntiles, kt, cu),
                  nk::plan_splitk_tn_f32(ntiles, kt, cu));
  } else if (is("tiles")) {
    int tri, tm, tn;
    while (std::scanf("%d %d %d", &tri, &tm, &tn) == 3) std::printf("%d\n", nk::plan_tile_count(tri, tm, tn));
  } else if (is("layout")) {
    int nprob;
    while (std::scanf("%d", &nprob) == 1 && nprob >= 1 && nprob <= nk::TN_MAXP) {
      Shape s[nk::TN_MAXP] = {};
      for (int q = 0; q < nprob; ++q)
        if (std::scanf("%d %d %d", &s[q].M, &s[q].N, &s[q].tri) != 3) return 3;
      const nk::TileLayout L = nk::plan_layout(s, nprob);
      for (int q = 0; q < nk::TN_MAXP; ++q) std::printf("%d ", L.tile_begin[q]);
      for (int q = 0; q < nprob; ++q) std::printf("%d ", L.tiles_n[q]);
      std::printf("%d\n", L.ntiles);
    }
  } else if (is("slice")) {
    long long K;
    int bk, splitk;
    while (std::scanf("%lld %d %d", &K, &bk, &splitk) == 3) {
      const int kt = nk::plan_ktiles(K, bk);
      std::printf("%d %d\n", kt, nk::plan_slice_len(kt, splitk, bk));
    }
  } else if (is("slab")) {
    int ntiles, splitk;
    while (std::scanf("%d %d", &ntiles, &splitk) == 2) std::printf("%zu\n", nk::plan_slab_elems(ntiles, splitk));
  } else if (is("kmat")) {
    int tm, tn;
    while (std::scanf("%d %d", &tm, &tn) == 2) std::printf("%u\n", nk::plan_kmat_grid(tm, tn));
  } else if (is("resid")) {
    int splitk, want;
    while (std::scanf("%d %d", &splitk, &want) == 2) std::printf("%d\n", nk::plan_splitk_with_resid(splitk, want != 0));
  } else if (is("contract")) {
    alignas(16) static char block[64];
    int per16, offa, offb, M, N;
    long long lda, ldb;
    while (std::scanf("%d %d %d %lld %lld %d %d", &per16, &offa, &offb, &lda, &ldb, &M, &N) == 7)
      std::printf("%d\n", nk::plan_operands_ok(block + offa, block + offb, lda, ldb, M, N, per16) ? 1 : 0);
  } else {
    return 2;
  }
  return 0;
}
