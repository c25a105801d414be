// The search tree's arithmetic (stove_amd/mcts/mcts_stove.py: Forest.select, Forest.child_slots, Forest.backpropagate -- that file is
// the specification, quirks included) on ONE tree's rows of the forest arrays, as plain inline functions: __host__ __device__ under
// hipcc (the kernels of plan_tree.hip call them), unmarked under a host compiler (tests/abi/plan_tree_driver.cpp runs the same text
// on the CPU under sanitizers).  Per tree, `cap` entries: first, parent, depth, Ns, Nsa (int32), Qsa (double); slot 0 is the root;
// `used` is the next free slot.
// Qsa must equal the host forest's bit for bit: every operation on it is an IEEE double add, multiply or divide, and none may be
// contracted into a fused multiply-add.  Under clang (hipcc) each function switches contraction off for its body; a host compiler
// gets -ffp-contract=off on its command line.  sqrt and the divisions are correctly rounded on both sides; log is the one library call.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PLAN_TREE_FN __host__ __device__ inline
#else
#define PLAN_TREE_FN inline
#endif
#if defined(__clang__)
#define PLAN_TREE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PLAN_TREE_NO_CONTRACT
#endif

namespace plan_tree {

constexpr int kMaxActions = 64;
// status of a tree: fine / out of slots (a fresh leaf with used + A > cap) / a walk or an index check failed
constexpr int kOk = 0, kFull = 1, kBad = 2;

struct Tree {        // one tree's rows
  int* first;
  int* parent;
  int* depth;
  int* Ns;
  int* Nsa;
  double* Qsa;
  int cap, A, D;
};

// where the descent stands: the node, and the scan's best value and action, carried from level to level
struct Walk {
  int cur, best_act;
  double cur_best, min_gap;
};
PLAN_TREE_FN Walk walk_start() { return Walk{0, 0, -INFINITY, INFINITY}; }

// first child slot of `cur` if the descent goes on below it, -1 if `cur` is the leaf, -2 if its children lie outside the arrays
PLAN_TREE_FN int descend(const Tree& t, int cur) {
  const int fc = t.first[cur];
  if (!(fc >= 0 && t.depth[cur] + 1 != t.D)) return -1;
  return fc > t.cap - t.A ? -2 : fc;
}

// UCT value of child a of `cur` (children from slot fc).  Ns[cur] == 0: log = -inf, sqrt of it NaN, and NaN never wins.
PLAN_TREE_FN double uct(const Tree& t, int cur, int fc, int a, double c) {
  PLAN_TREE_NO_CONTRACT
  const double explore = sqrt(log((double)t.Ns[cur]) / (double)(1 + t.Nsa[fc + a]));
  const double scaled = c * explore;
  return t.Qsa[fc + a] + scaled;
}

// One level: the gap between the two largest of {cur_best, u_0 .. u_{A-1}} (numpy's sort puts NaN last, so a level with a NaN
// candidate has a NaN gap and contributes nothing), then the reference's scan in action order with strict >.
PLAN_TREE_FN void scan(const double* u, int A, Walk& w) {
  PLAN_TREE_NO_CONTRACT
  double top = w.cur_best, second = -INFINITY;
  bool any_nan = false, have_second = false;
  for (int a = 0; a < A; ++a) {
    const double v = u[a];
    if (v != v) {
      any_nan = true;
    } else if (v > top) {
      second = top;
      top = v;
      have_second = true;
    } else if (!have_second || v > second) {
      second = v;
      have_second = true;
    }
  }
  if (!any_nan && have_second) {
    const double gap = top - second;
    if (isfinite(gap) && gap < w.min_gap) w.min_gap = gap;
  }
  for (int a = 0; a < A; ++a)
    if (u[a] > w.cur_best) {
      w.cur_best = u[a];
      w.best_act = a;
    }
}

// the parent chain of `leaf` reaches a node of depth 0 inside the arrays within D steps (what backpropagate will walk)
PLAN_TREE_FN bool path_ok(const Tree& t, int leaf) {
  int node = leaf;
  for (int step = 0; step <= t.D; ++step) {
    if (t.depth[node] < 1) return true;
    const int par = t.parent[node];
    if (par < 0 || par >= t.cap) return false;
    node = par;
  }
  return false;
}

// Forest.child_slots and len_s for the selected leaf -> status.  Only a fresh leaf advances `used`; nothing is changed on failure.
PLAN_TREE_FN int child_slots(const Tree& t, int leaf, int* used, int* child, int* len_s) {
  const int ls = t.depth[leaf] + 1;
  if (ls < 1 || ls > t.D || !path_ok(t, leaf)) return kBad;
  const int have = t.first[leaf];
  if (have >= 0) {
    if (have > t.cap - t.A) return kBad;
    *child = have;
  } else {
    const int u = *used;
    if (u < 1 || u > t.cap) return kBad;
    if (u > t.cap - t.A) return kFull;
    *child = u;
    *used = u + t.A;
  }
  *len_s = ls;
  return kOk;
}

// Forest.select for one tree, serially: -> status; the leaf in *leaf, the smallest gap of this walk in *min_gap
PLAN_TREE_FN int select(const Tree& t, double c, int* leaf, double* min_gap) {
  Walk w = walk_start();
  double u[kMaxActions];
  for (int level = 0;; ++level) {
    const int fc = descend(t, w.cur);
    if (fc == -1) break;
    if (fc < 0 || level >= t.D) return kBad;
    for (int a = 0; a < t.A; ++a) u[a] = uct(t, w.cur, fc, a, c);
    scan(u, t.A, w);
    w.cur = fc + w.best_act;
  }
  *leaf = w.cur;
  *min_gap = w.min_gap;
  return kOk;
}

// ---- Forest.backpropagate, in its order: the children (re)initialised, Ns[leaf] += 1, the mean value up to the root's child
PLAN_TREE_FN void init_child(const Tree& t, int leaf, int child, int a, double q) {
  const int s = child + a;
  t.first[s] = -1;
  t.parent[s] = leaf;
  t.depth[s] = t.depth[leaf] + 1;
  t.Qsa[s] = q;
  t.Nsa[s] = 1;
  t.Ns[s] = 0;
}

// (((q_0 + q_1) + ...) + q_{A-1}) / A, a running sum from 0.0; q as the device wrote it (float32), widened
PLAN_TREE_FN double mean_value(const float* q, int A) {
  PLAN_TREE_NO_CONTRACT
  double total = 0.0;
  for (int a = 0; a < A; ++a) total = total + (double)q[a];
  return total / (double)A;
}

PLAN_TREE_FN void walk_up(const Tree& t, int leaf, int child, double value) {
  PLAN_TREE_NO_CONTRACT
  t.first[leaf] = child;
  t.Ns[leaf] += 1;
  int node = leaf;
  for (int step = 0; step <= t.D && t.depth[node] >= 1; ++step) {        // (path_ok has walked this chain)
    const int par = t.parent[node];
    t.Ns[par] += 1;
    const int n = t.Nsa[node] + 1;
    t.Nsa[node] = n;
    const double scaled = t.Qsa[node] * (double)(n - 1);
    const double sum = scaled + value;
    t.Qsa[node] = sum / (double)n;
    node = par;
  }
}

PLAN_TREE_FN void backpropagate(const Tree& t, int leaf, int child, const float* q) {
  for (int a = 0; a < t.A; ++a) init_child(t, leaf, child, a, (double)q[a]);
  walk_up(t, leaf, child, mean_value(q, t.A));
}

// the first-index argmax of Nsa over the root's children, 0 for a root without (or with out-of-range) children
PLAN_TREE_FN int best_action(const Tree& t) {
  const int fc = t.first[0];
  if (fc < 0 || fc > t.cap - t.A) return 0;
  int best = 0;
  for (int a = 1; a < t.A; ++a)
    if (t.Nsa[fc + a] > t.Nsa[fc + best]) best = a;
  return best;
}

}  // namespace plan_tree
