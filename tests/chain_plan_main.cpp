// Stand-alone driver of nk_chain_plan.h for tests/test_rollout_reference_host.py: reads lines
// "m p d_lift T batch num_cu batch_invariant per_trajectory_bias mw_allowed" from standard input and prints, per line,
// "route lift_in_kernel tb blocks kpt nt groups launches launches_per_step score_tile chain_ok mw_fits lds_bytes".
#include <cstdio>

#include "nk_chain_plan.h"

int main() {
  int m, p, dl, T, batch, cu, inv, ptb, allowed;
  while (std::scanf("%d %d %d %d %d %d %d %d %d", &m, &p, &dl, &T, &batch, &cu, &inv, &ptb, &allowed) == 9) {
    const nk::ChainPlan pl = nk::chain_plan(m, p, dl, T, batch, cu, inv != 0, ptb != 0, allowed != 0);
    const int pu = T > 1 ? p : 0;
    const size_t bytes = pl.route == nk::ROUTE_CHAIN ? nk::chain_lds_bytes(pu, pl.lift_in_kernel ? dl : 0, pl.tb) : 0;
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %zu\n", pl.route, pl.lift_in_kernel ? 1 : 0, pl.tb, pl.blocks, pl.kpt,
                pl.nt, pl.groups, pl.launches, pl.launches_per_step, nk::traj_err_tile(m),
                nk::lifted_chain_ok(m, pu, dl) ? 1 : 0, nk::chain_mw_fits(m, pu, cu) ? 1 : 0, bytes);
  }
  return 0;
}
