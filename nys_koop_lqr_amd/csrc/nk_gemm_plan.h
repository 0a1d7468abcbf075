// Launch plan of the three matrix-product engines (nk_gemm.hip, nk_gemm_tn.hip, nk_gemm_tn_f32.hip): how many 128 x 128
// tiles a problem has, where the problems of a fused launch begin, how many K slices a launch takes and how long a slice
// is.  Host only, no HIP include, so that a plain C++17 compiler builds it (tests/gemm_plan_main.cpp): pure functions of
// integers and one double cost model.  Every rule below is known here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>

namespace nk {

// TRI_UPPER_MIRROR: compute tiles with tn >= tm and mirror; TRI_LOWER (generic engine only): tiles tn <= tm only
enum { TRI_FULL = 0, TRI_UPPER_MIRROR = 1, TRI_LOWER = 2 };

constexpr int TBM = 128;               // edge of an output tile, all engines
constexpr int TN_MAXP = 4;             // problems per launch of the TN engines
constexpr int TILE_UNUSED = 1 << 30;   // tile_begin of an unused problem slot: no tile index reaches it

inline int plan_tiles(int64_t n) { return (int)((n + TBM - 1) / TBM); }
inline int plan_ktiles(int64_t K, int bk) { return (int)((K + bk - 1) / bk); }

// tiles of one problem (TRI_UPPER_MIRROR: square, TRI_LOWER: tiles_m >= tiles_n)
inline int plan_tile_count(int tri, int tiles_m, int tiles_n) {
  if (tri == TRI_UPPER_MIRROR) return tiles_m * (tiles_m + 1) / 2;
  if (tri == TRI_LOWER) return tiles_n * (tiles_n + 1) / 2 + (tiles_m - tiles_n) * tiles_n;
  return tiles_m * tiles_n;
}

// The problems of one launch, laid end to end in tile index: problem q owns [tile_begin[q], tile_begin[q + 1]).
struct TileLayout {
  int tiles_n[TN_MAXP];
  int tile_begin[TN_MAXP];
  int ntiles;
};
template <class Problem>  // anything with M, N, tri
inline TileLayout plan_layout(const Problem* probs, int nprob) {
  TileLayout L{};
  for (int q = 0; q < TN_MAXP; ++q) {
    L.tile_begin[q] = q < nprob ? L.ntiles : TILE_UNUSED;
    if (q >= nprob) continue;
    L.tiles_n[q] = plan_tiles(probs[q].N);
    L.ntiles += plan_tile_count(probs[q].tri, plan_tiles(probs[q].M), L.tiles_n[q]);
  }
  return L;
}

// contraction rows per K slice: whole k-steps of bk rows, at least one
inline int plan_slice_len(int ktiles_total, int splitk, int bk) {
  const int klen = ((ktiles_total + splitk - 1) / splitk) * bk;
  return klen == 0 ? bk : klen;
}
// doubles of the slab [tile][slice][128][128] of a TN launch
inline size_t plan_slab_elems(int ntiles, int splitk) { return (size_t)ntiles * splitk * TBM * TBM; }
// workgroups of a kernel-matrix launch: every XCD (blockIdx & 7) owns the tile columns xcd, xcd + 8, ... for all tile rows
inline unsigned plan_kmat_grid(int tiles_m, int tiles_n) { return 8u * (unsigned)tiles_m * (unsigned)((tiles_n + 7) / 8); }

// ---- K slices.  Three policies for three kernels (ntiles output tiles, ktiles_total k-steps, num_cu compute units); their
// arithmetic decides grids and, through the summation order, result bits: keep the order of every operation. ---------------

// generic engine (k-steps of 16 rows)
inline int plan_splitk_generic(int ntiles, int ktiles_total, int num_cu) {
  const int target = 4 * num_cu;  // two resident workgroups per CU, two rounds
  int splitk = ntiles >= target / 2 ? 1 : (target + ntiles - 1) / ntiles;
  if (splitk >= 6) splitk = ((splitk + 7) / 8) * 8;  // align slices with the 8 XCDs
  const int max_split = ktiles_total / 8 > 0 ? ktiles_total / 8 : 1;  // at least 8 k-steps per slice
  if (splitk > max_split) splitk = max_split;
  if (splitk > 64) splitk = 64;
  if (splitk < 1) splitk = 1;
  return splitk;
}

// fp64 TN engine (k-steps of 16 rows)
inline int plan_splitk_tn_f64(int ntiles, int ktiles_total, int num_cu) {
  // Pick the number of K slices with a small cost model calibrated on MI355X (profiles/r01_*): a k-step costs
  // 1.22 units per workgroup when two workgroups share a CU and 2.35 when a workgroup is alone on its CU (one wave
  // per SIMD cannot hide the barrier + DMA latency); workgroups beyond 2/CU run as further rounds.  The slab
  // round trip (write + read of ntiles*splitk tiles) is charged at ~4 TB/s.  Multiples of 8 keep one K range per
  // XCD (panels shared through that XCD's L2) and get a small bonus.
  const int slots = 2 * num_cu;
  const int max_split = ktiles_total / 8 > 1 ? ktiles_total / 8 : 1;
  double best = 1e300;
  int splitk = 1;
  for (int c = 1; c <= 64 && c <= max_split; ++c) {
    const int64_t wgs = (int64_t)ntiles * c;
    const double steps = (double)((ktiles_total + c - 1) / c);
    const int64_t full = wgs / slots, rem = wgs % slots;
    double t = full * 2.44 * steps;
    if (rem > 0) t += (rem <= num_cu ? 2.35 : 2.44) * steps;
    t *= 4096.0;                                                      // cycles of MFMA per k-step and wave
    if (c > 1) t += (double)wgs * (TBM * TBM * 8.0 * 2.0) / 4.0e12 * 2.4e9;  // slab write + read, in cycles
    t += 2000.0 * c / 8.0;                                            // mild preference for fewer slices
    if (c % 8 == 0) t *= 0.97;
    if (t < best) { best = t; splitk = c; }
  }
  return splitk;
}
// the residual partials of a launch come out of the reduce kernel: such a launch has at least 2 slices
inline int plan_splitk_with_resid(int splitk, bool want_resid) { return want_resid && splitk < 2 ? 2 : splitk; }

// fp32 TN engine (k-steps of 32 rows)
inline int plan_splitk_tn_f32(int ntiles, int ktiles_total, int num_cu) {
  // K slices: the fewest (1, 2, 4, then multiples of 8: one K range per XCD) that fill at least 95 % of the workgroup
  // slots of the rounds they need, while a slice keeps at least 8 k-steps
  const int64_t slots = 2 * num_cu;
  int splitk = 1;
  double best_eff = 0.0;
  for (int c : {1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64}) {
    if (c > 1 && ktiles_total / c < 8) break;
    const int64_t wgs = (int64_t)ntiles * c;
    const int64_t rounds = (wgs + slots - 1) / slots;
    const double eff = (double)wgs / (double)(rounds * slots);
    if (eff > best_eff + 1e-9) { best_eff = eff; splitk = c; }
    if (eff >= 0.95) break;
  }
  return splitk;
}

// ---- operand contract of the LDS-DMA engines: one lane moves 16 bytes = per16 elements (2 fp64, 4 fp32), so operands are
// 16-byte aligned, leading dimensions whole 16-byte units that cover the columns rounded up to one, at least one unit wide
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool plan_operands_ok(const void* A, const void* B, int64_t lda, int64_t ldb, int M, int N, int per16) {
  const int r = per16 - 1;
  return M >= per16 && N >= per16 && aligned16(A) && aligned16(B) && lda % per16 == 0 && ldb % per16 == 0 &&
         lda >= ((M + r) & ~r) && ldb >= ((N + r) & ~r);
}

}  // namespace nk
