// Launch classes of the multi-model closed loops (nk_plant_loop.hip, nk_mpc_loop.hip): the units of one call are sorted into
// classes of (kernel family, shape, waves per workgroup) -- shape = landmarks per lane in the plant loops, padded QP lanes in the
// MPC loops -- and every class runs as one launch.  Host only, no HIP include, so that a plain C++17 compiler builds it
// (tests/loop_classes_main.cpp): the order of the classes and of the units inside them is known here and nowhere else.
#pragma once
#include <algorithm>
#include <vector>

namespace nk {

struct LoopClass {
  int ktype, shape, waves;
};
inline bool operator<(const LoopClass& a, const LoopClass& b) {
  if (a.ktype != b.ktype) return a.ktype < b.ktype;
  if (a.shape != b.shape) return a.shape < b.shape;
  return a.waves < b.waves;
}

// units [begin, end) of the sorted order share `key`; lds: the largest need among them (0 when none was given)
struct LoopRun {
  int begin, end;
  LoopClass key;
  long lds;
};
struct LoopClassPlan {
  std::vector<int> perm;      // sorted position -> the caller's index; stable: inside a class the order is the caller's
  std::vector<LoopRun> runs;  // in ascending key order
};

// keys[u]: the class of unit u; lds[u]: its LDS need, or lds = nullptr
inline LoopClassPlan plan_loop_classes(const LoopClass* keys, int n, const long* lds = nullptr) {
  LoopClassPlan plan;
  plan.perm.resize((size_t)n);
  for (int u = 0; u < n; ++u) plan.perm[(size_t)u] = u;
  std::stable_sort(plan.perm.begin(), plan.perm.end(), [&](int a, int b) { return keys[a] < keys[b]; });
  for (int b = 0; b < n;) {
    LoopRun run{b, b + 1, keys[plan.perm[(size_t)b]], lds ? lds[plan.perm[(size_t)b]] : 0L};
    for (; run.end < n && !(run.key < keys[plan.perm[(size_t)run.end]]); ++run.end)
      if (lds) run.lds = std::max(run.lds, lds[plan.perm[(size_t)run.end]]);
    plan.runs.push_back(run);
    b = run.end;
  }
  return plan;
}

}  // namespace nk
