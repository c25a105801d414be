// Tree search on the TRUE environment (stove_amd/mcts/mcts_env.py: EnvForest -- that file and stove_amd/envs/envs.py are the
// specification, quirks included) on ONE tree's rows, as plain inline functions: __host__ __device__ under hipcc (the kernel of
// env_search.hip calls them), unmarked under a host compiler (tests/abi/env_search_driver.cpp runs the same text on the CPU under
// sanitizers).  The tree layout is plan_tree.h's (first, parent, depth, Ns, Nsa int32, Qsa double; slot 0 the root; A consecutive child
// slots per expansion; `used` the next free slot): slot first[s] + a holds the edge (s, a) -- its Qsa and Nsa -- and the node s + a -- its
// Ns, first, parent, depth.  The environment step is env_step.h's, unchanged.
//
// One iteration replays its path from the root state, so it is a fixed schedule of D steps: at step k a tree that is still walking
// either descends (action from the tree), expands (action from the table, then a rollout from the table) or meets a terminal node (no
// step, and none after it).  Nothing of the tree is written before the whole iteration is known to count: a refused iteration leaves the
// tree as it stood.  Qsa must equal the host forest's bit for bit: every operation on it is an IEEE double add, multiply or divide, and
// none may be contracted; rewards are minus collision counts, so every value is an integer.  log (UCT) is the one library call.
#pragma once
#include <math.h>

#include "env_step.h"
#include "plan_tree.h"

#define ENV_SEARCH_FN ENV_STEP_FN
#define ENV_SEARCH_NO_CONTRACT ENV_STEP_NO_CONTRACT

namespace env_search {

constexpr int kActions = env_step::kActions;
// status of a tree: searched / out of slots (an expansion with used + A > cap), frozen / a draw outside [0, A) or a failed index check,
// frozen as it stood at the start of that iteration
constexpr int kOk = plan_tree::kOk, kFull = plan_tree::kFull, kBad = plan_tree::kBad;
constexpr double kC = 1.0;        // the reference's exploration constant (MCTS.c)

using plan_tree::Tree;

// One Descend level at node `cur` (children from slot fc): the first-index argmax of u with strict >, from -inf fresh at this level;
// *gap is lowered to u[best] - the largest u among candidates whose (Qsa, Nsa) differ from the best's (equal inputs tie exactly on
// every side and do not count).
ENV_SEARCH_FN int choose(const Tree& t, int cur, int fc, double* gap) {
  ENV_SEARCH_NO_CONTRACT
  double u[kActions];
  double best_u = -INFINITY;
  int best = 0;
  for (int a = 0; a < kActions; ++a) {
    u[a] = plan_tree::uct(t, cur, fc, a, kC);
    if (u[a] > best_u) {
      best_u = u[a];
      best = a;
    }
  }
  const double q = t.Qsa[fc + best];
  const int n = t.Nsa[fc + best];
  for (int a = 0; a < kActions; ++a) {
    if (t.Qsa[fc + a] == q && t.Nsa[fc + a] == n) continue;
    const double g = best_u - u[a];
    if (g < *gap) *gap = g;
  }
  return best;
}

// One iteration of one tree.  x0, v0, r, m: the root state's rows (read only); x, v: 2 N doubles of working room; draws: this
// iteration's row of the table, D entries.  -> status; on kOk the tree, *used and *min_gap are updated, otherwise nothing is written.
ENV_SEARCH_FN int iterate(const Tree& t, int* used, const double* x0, const double* v0, const double* r, const double* m, double* x, double* v,
                          const env_step::Params& p, const int* draws, double* min_gap) {
  ENV_SEARCH_NO_CONTRACT
  const int A = kActions, D = t.D;
  for (int k = 0; k < 2 * p.N; ++k) {
    x[k] = x0[k];
    v[k] = v0[k];
  }
  enum { kWalk, kRoll, kDone };
  int mode = kWalk, cur = 0, col = 0, fresh = -1, edge_a = 0, hits = 0;
  double value = 0.0, gap = INFINITY;
  for (int k = 0; k < D && mode != kDone; ++k) {
    int a;
    if (mode == kWalk) {
      if (t.depth[cur] != k) return kBad;                // (the walk stands on a node of key length k + 1)
      const int fc = t.first[cur];
      if (fc < 0) {                                      // Expand: len(s) < D always holds here
        if (k + 1 >= D) return kBad;
        const int u = *used;
        if (u < 1 || u > t.cap) return kBad;
        if (u > t.cap - A) return kFull;
        fresh = u;
        a = draws[col++];
        edge_a = a;
        mode = kRoll;
      } else {
        if (fc < 1 || fc > t.cap - A) return kBad;
        if (k + 2 != D) {                                // Descend
          a = choose(t, cur, fc, &gap);
          if (t.parent[fc + a] != cur) return kBad;
        } else {                                         // Terminal: the value is a drawn edge's Q, the counted edge is (s, 0)
          a = draws[0];
          if (a < 0 || a >= A) return kBad;
          value = t.Qsa[fc + a];
          mode = kDone;
          break;
        }
      }
    } else {
      a = draws[col++];
    }
    int hit = 0;
    if (env_step::step(x, v, r, m, p, &a, &hit) != env_step::kOk) return kBad;
    if (mode == kRoll) hits += hit;
    else cur = t.first[cur] + a;
  }
  if (mode == kWalk) return kBad;
  // ---- the iteration counts: expansion, then the counts and means from the node where the walk ended up to the root
  const bool terminal = mode == kDone;
  int edge;
  if (!terminal) {
    for (int a = 0; a < A; ++a) {
      const int s = fresh + a;
      t.first[s] = -1;
      t.parent[s] = cur;
      t.depth[s] = t.depth[cur] + 1;
      t.Qsa[s] = -1.0;
      t.Nsa[s] = 0;
      t.Ns[s] = 0;
    }
    t.first[cur] = fresh;
    t.Ns[cur] = 0;
    *used = fresh + A;
    edge = fresh + edge_a;
    value = (double)(-hits);
  } else {
    edge = t.first[cur];
  }
  t.Ns[cur] += 1;
  {
    const int n = t.Nsa[edge] + 1;
    t.Nsa[edge] = n;
    if (!terminal) {
      const double scaled = t.Qsa[edge] * (double)(n - 1);
      const double sum = scaled + value;
      t.Qsa[edge] = sum / (double)n;
    }
  }
  for (int node = cur; t.depth[node] >= 1;) {            // (every parent link of this path was checked on the way down)
    const int par = t.parent[node];
    t.Ns[par] += 1;
    const int n = t.Nsa[node] + 1;
    t.Nsa[node] = n;
    const double scaled = t.Qsa[node] * (double)(n - 1);
    const double sum = scaled + value;
    t.Qsa[node] = sum / (double)n;
    node = par;
  }
  if (gap < *min_gap) *min_gap = gap;
  return kOk;
}

// the visit counts of one tree's root edges (rows first, Nsa of `cap` entries) added to counts[0 .. A); a root without (or with
// out-of-range) children adds nothing
ENV_SEARCH_FN void add_root_counts(const int* first, const int* Nsa, int cap, int* counts) {
  const int fc = first[0];
  if (fc < 1 || fc > cap - kActions) return;
  for (int a = 0; a < kActions; ++a) counts[a] += Nsa[fc + a];
}

// first-index argmax
ENV_SEARCH_FN int best_of(const int* counts) {
  int best = 0;
  for (int a = 1; a < kActions; ++a)
    if (counts[a] > counts[best]) best = a;
  return best;
}

}  // namespace env_search
