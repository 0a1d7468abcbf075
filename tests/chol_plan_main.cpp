// Stand-alone driver of nk_chol_plan.h for tests/test_chol_plan_host.py.  Standard input holds lines of two kinds:
//   "sys m extra"                         -> the plan of one system:
//        "blocks nblk"
//        "flow nblk nex flags items"
//        "trsm workgroups"
//        per block step jb = 0 .. nblk (one past the last, which must come out empty):
//        "step jb j0 nbj rem rows panel trail nb_next | panel_wgs | tiles_n tiles_m trail_wgs |
//              next.row0 next.col0 next.rows next.cols  rest.row0 rest.col0 rest.rows rest.cols |
//              fwd.row0 fwd.rows fwd.k  bwd.row0 bwd.rows bwd.k"
//        "end"
//   "pair nsys m0 extra0 m1 extra1 allowed" -> "launch words items route"   (one dataflow launch for the systems; the route)
#include <cstdio>
#include <cstring>

#include "nk_chol_plan.h"

int main() {
  char kind[8];
  while (std::scanf("%7s", kind) == 1) {
    if (std::strcmp(kind, "sys") == 0) {
      int m, extra;
      if (std::scanf("%d %d", &m, &extra) != 2) return 3;
      const int nblk = nk::chol_blocks(m);
      const nk::CholFlowCounts f = nk::chol_flow_counts(m, extra);
      std::printf("blocks %d\nflow %d %d %d %d\ntrsm %d\n", nblk, f.nblk, f.nex, f.flags, f.items, nk::chol_trsm_workgroups(extra));
      for (int jb = 0; jb <= nblk; ++jb) {
        const nk::CholStepShape s = nk::chol_step_shape(m, extra, jb);
        const nk::CholTrailTiles t = s.trail ? nk::chol_trail_tiles(s.rows, s.rem) : nk::CholTrailTiles{};
        const nk::CholLookahead la = s.trail ? nk::chol_lookahead_split(s.rows, s.rem) : nk::CholLookahead{};
        const nk::CholSolveUpdate fw = nk::chol_solve_forward(m, jb), bw = nk::chol_solve_backward(m, jb);
        std::printf("step %d %d %d %d %d %d %d %d | %d | %d %d %d | %d %d %d %d %d %d %d %d | %d %d %d %d %d %d\n", jb, s.j0,
                    s.nbj, s.rem, s.rows, s.panel ? 1 : 0, s.trail ? 1 : 0, s.nb_next,
                    s.panel ? nk::chol_panel_workgroups(s.rows) : 0, t.tiles_n, t.tiles_m, t.workgroups, la.next.row0,
                    la.next.col0, la.next.rows, la.next.cols, la.rest.row0, la.rest.col0, la.rest.rows, la.rest.cols, fw.row0,
                    fw.rows, fw.k, bw.row0, bw.rows, bw.k);
      }
      std::printf("end\n");
    } else if (std::strcmp(kind, "pair") == 0) {
      int nsys, m[2], extra[2], allowed;
      if (std::scanf("%d %d %d %d %d %d", &nsys, &m[0], &extra[0], &m[1], &extra[1], &allowed) != 6) return 3;
      if (nsys < 1 || nsys > 2) return 2;
      std::printf("launch %zu %d %d\n", nk::chol_flow_words(m, extra, nsys), nk::chol_flow_items(m, extra, nsys),
                  nk::chol_route_is_flow(m, nsys, allowed != 0) ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
