// Block plan of the blocked Cholesky (nk_chol.hip, nk_trail.hip, nk_potrf.hip, nk_trsm.hip, nk_chol_flow.hip): the blocks of a
// system, the shape of every block step, the workgroup counts of its launches, the look-ahead split, the counts of the
// dataflow launch and the route between the two.  Host only, no HIP include, so that a plain C++17 compiler builds it
// (tests/chol_plan_main.cpp): pure functions of integers.  Every rule below is stated here and nowhere else;
// tests/test_chol_plan_host.py recomputes each of them, and tests/chol_reference.py::flow_items mirrors chol_flow_counts.
#pragma once
#include <stddef.h>

namespace nk {

constexpr int CHOL_BLOCK = 64;        // order of a diagonal block = columns of a panel = contraction length of a trailing update
constexpr int CHOL_TRAIL_TILE = 128;  // a workgroup of the trailing update owns one 128 x 128 tile
constexpr int CHOL_PANEL_ROWS = 64;   // rows per workgroup of the panel solve
constexpr int CHOL_TRSM_ROWS = 16;    // rows per workgroup of the backward substitution
constexpr int CHOL_FLOW_MIN_M = 256;  // the dataflow launch takes systems from this order on
constexpr int CHOL_FLOW_HDR = 16;     // words ahead of the flags of a dataflow launch: [0] ticket, [1] status

inline int chol_ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- blocks of a system of order m
inline int chol_blocks(int m) { return chol_ceil_div(m, CHOL_BLOCK); }
// order of diagonal block jb (0: the system has no such block)
inline int chol_block_order(int m, int jb) {
  const int left = m - jb * CHOL_BLOCK;
  return left <= 0 ? 0 : (left < CHOL_BLOCK ? left : CHOL_BLOCK);
}

// ---- block step jb of a system of order m with `extra` rows riding along below it (0: the plain factorisation)
struct CholStepShape {
  int j0 = 0;       // first row and column of the diagonal block
  int nbj = 0;      // its order; 0: the system has no step jb and everything below is empty
  int rem = 0;      // rows of the square part below the diagonal block
  int rows = 0;     // ... plus the extra rows: rows of the panel and of the trailing matrix
  bool panel = false;  // panel solve  (rows x nbj) <- (rows x nbj) L_jj^-T
  bool trail = false;  // trailing update  (rows x rem) -= panel panel^T, contraction length nbj == CHOL_BLOCK
  int nb_next = 0;  // order of diagonal block jb + 1, the top left corner of the trailing matrix (0: none)
};
inline CholStepShape chol_step_shape(int m, int extra, int jb) {
  CholStepShape s;
  s.nbj = chol_block_order(m, jb);
  if (s.nbj == 0) return s;
  s.j0 = jb * CHOL_BLOCK;
  s.rem = m - s.j0 - s.nbj;
  s.rows = s.rem + extra;
  s.panel = s.rows > 0;
  s.trail = s.rem > 0;  // (then nbj == CHOL_BLOCK: only the last block is short, and nothing lies below it)
  s.nb_next = chol_block_order(m, jb + 1);
  return s;
}

// ---- workgroups
// Trailing update of a rows x rem matrix (rows >= rem): the 128-tiles that meet the lower triangle of the leading rem x rem
// part, plus all tiles of the rows below it.  Tile row r of the lower set holds min(r + 1, tiles_n) tiles.
struct CholTrailTiles {
  int tiles_n = 0, tiles_m = 0, workgroups = 0;
};
inline CholTrailTiles chol_trail_tiles(int rows, int rem) {
  CholTrailTiles t;
  if (rows <= 0 || rem <= 0) return t;
  t.tiles_n = chol_ceil_div(rem, CHOL_TRAIL_TILE);
  t.tiles_m = chol_ceil_div(rows, CHOL_TRAIL_TILE);
  t.workgroups = t.tiles_n * (t.tiles_n + 1) / 2 + (t.tiles_m - t.tiles_n) * t.tiles_n;
  return t;
}
inline int chol_panel_workgroups(int rows) { return rows > 0 ? chol_ceil_div(rows, CHOL_PANEL_ROWS) : 0; }
// backward substitution E <- E L^-1 on the extra rows: one workgroup per band of rows
inline int chol_trsm_workgroups(int extra) { return extra > 0 ? chol_ceil_div(extra, CHOL_TRSM_ROWS) : 0; }

// ---- look-ahead: the trailing update (rows x rem) split into the next block column (all rows) and everything to the right of
// it.  Offsets count from the first row of the panel and from the top left corner of the trailing matrix; each part is a
// trailing update of its own (lower tiles of its leading cols x cols part, full tiles below).
struct CholTrailPart {
  int row0 = 0, col0 = 0;  // first panel row (= first row of the trailing matrix) and first column of the part
  int rows = 0, cols = 0;  // cols == 0: the part is empty
};
struct CholLookahead {
  CholTrailPart next, rest;
};
inline CholLookahead chol_lookahead_split(int rows, int rem) {
  CholLookahead la;
  if (rows <= 0 || rem <= 0) return la;
  const int nbn = rem < CHOL_BLOCK ? rem : CHOL_BLOCK;
  la.next.rows = rows; la.next.cols = nbn;
  if (rem > nbn) {
    la.rest.row0 = la.rest.col0 = nbn;
    la.rest.rows = rows - nbn; la.rest.cols = rem - nbn;
  }
  return la;
}

// ---- the dataflow launch (nk_chol_flow.hip): 64 x 64 tiles (i, k), i >= k, of the square part and of the extra rows
struct CholFlowCounts {
  int nblk = 0;   // block columns = tile rows of the square part
  int nex = 0;    // tile rows of the extra rows
  int flags = 0;  // one word per tile of the (nblk + nex) x nblk grid
  int items = 0;  // work items: per block column one diagonal item (which also owns the tile under the diagonal), the square
                  // tiles from two below the diagonal on, and the tiles of the extra rows
};
inline CholFlowCounts chol_flow_counts(int m, int extra) {
  CholFlowCounts f;
  f.nblk = chol_blocks(m);
  f.nex = chol_ceil_div(extra, CHOL_BLOCK);
  f.flags = (f.nblk + f.nex) * f.nblk;
  for (int c = 0; c < f.nblk; ++c) f.items += 1 + (f.nblk - c - 2 > 0 ? f.nblk - c - 2 : 0) + f.nex;
  return f;
}
// one launch for systems 0 .. nsys - 1: its flag words behind the header, and its work items
inline size_t chol_flow_words(const int* m, const int* extra, int nsys) {
  size_t words = CHOL_FLOW_HDR;
  for (int q = 0; q < nsys; ++q) words += (size_t)chol_flow_counts(m[q], extra[q]).flags;
  return words;
}
inline int chol_flow_items(const int* m, const int* extra, int nsys) {
  int items = 0;
  for (int q = 0; q < nsys; ++q) items += chol_flow_counts(m[q], extra[q]).items;
  return items;
}

// ---- the route: the dataflow launch iff every system has m >= CHOL_FLOW_MIN_M; allowed: the conditions that are no
// arithmetic (the switch is on, the context is not recording a lock-step group, no re-run after a give-up is under way)
inline bool chol_route_is_flow(const int* m, int nsys, bool allowed) {
  if (!allowed || nsys < 1) return false;
  for (int q = 0; q < nsys; ++q)
    if (m[q] < CHOL_FLOW_MIN_M) return false;
  return true;
}

// ---- substitutions with the finished factor (cholesky_solve_pair): rows [row0, row0 + rows) of the right-hand sides receive
// -= L[those rows, block jb] X_jb, contraction length k.  Forward (L T = R): the rows below block jb, after its solve;
// backward (L^T X = T): the rows above it, with the block of the factor transposed.
struct CholSolveUpdate {
  int row0 = 0, rows = 0, k = 0;  // rows == 0: no update
};
inline CholSolveUpdate chol_solve_forward(int m, int jb) {
  CholSolveUpdate u;
  const CholStepShape s = chol_step_shape(m, 0, jb);
  if (s.rem > 0) { u.row0 = s.j0 + s.nbj; u.rows = s.rem; u.k = s.nbj; }
  return u;
}
inline CholSolveUpdate chol_solve_backward(int m, int jb) {
  CholSolveUpdate u;
  const CholStepShape s = chol_step_shape(m, 0, jb);
  if (s.nbj > 0 && s.j0 > 0) { u.rows = s.j0; u.k = s.nbj; }
  return u;
}

}  // namespace nk
