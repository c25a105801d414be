// The search trees on the device (stove_plan_search, capi.hip): per iteration plan_tree_select_k produces the leaf / child / len_s
// vectors stove_plan_expand's launches read, and plan_tree_backprop_k consumes the q they wrote; plan_tree_action_k reads the root's
// visit counts at the end.  The arithmetic is csrc/plan_tree.h's, the text the CPU driver runs.  One wave per tree: a descent is a
// chain of dependent loads D levels deep and the scan is a handful of compares, so the lanes only share the A evaluations of
// log / sqrt / divide of a level (lane a computes u_a into LDS) and lane 0 scans them serially in the reference's order.
// A tree whose status is not 0 is frozen: select hands plan_prep_k the indices (-1, -1, 0), which it flags, so the tree's pool slots
// are neither read nor written, and backprop leaves its arrays alone.  Plain vector loads and stores, no atomics.
#include "common.h"
#include "plan_tree.h"

namespace stove {

__device__ inline plan_tree::Tree plan_tree_rows(int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int m, int cap, int A,
                                                 int D) {
  const size_t o = (size_t)m * cap;
  return plan_tree::Tree{first + o, parent + o, depth + o, Ns + o, Nsa + o, Qsa + o, cap, A, D};
}

// grid M, block 64.  leaf / child / len_s (M,) and gap (M,), the smallest gap of this walk, out; used, status (M,) in and out;
// sel_trace row (M,) or NULL.  min_gap is lowered by plan_tree_backprop_k, once the iteration is known to count.
__global__ __launch_bounds__(64) void plan_tree_select_k(int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used,
                                                         double* gap, int* status, int* leaf, int* child, int* len_s, int* sel_trace,
                                                         double c, int cap, int A, int D) {
  __shared__ double u[plan_tree::kMaxActions];
  __shared__ int next[2];          // cur, first child (-1: cur is the leaf, -2: out of range)
  const int m = blockIdx.x, lane = threadIdx.x;
  const plan_tree::Tree t = plan_tree_rows(first, parent, depth, Ns, Nsa, Qsa, m, cap, A, D);
  int st = status[m];
  plan_tree::Walk w = plan_tree::walk_start();         // (lane 0's copy is the one that counts)
  if (st == plan_tree::kOk) {
    for (int level = 0;; ++level) {
      if (lane == 0) {
        next[0] = w.cur;
        next[1] = plan_tree::descend(t, w.cur);
      }
      __syncthreads();
      const int cur = next[0], fc = next[1];
      if (fc == -1) break;
      if (fc < 0 || level >= D) {
        st = plan_tree::kBad;
        break;
      }
      if (lane < A) u[lane] = plan_tree::uct(t, cur, fc, lane, c);
      __syncthreads();
      if (lane == 0) {
        plan_tree::scan(u, A, w);
        w.cur = fc + w.best_act;
      }
    }
  }
  if (lane != 0) return;
  int lf = -1, ch = -1, ls = 0;
  if (st == plan_tree::kOk) {
    int us = used[m];
    st = plan_tree::child_slots(t, w.cur, &us, &ch, &ls);
    if (st == plan_tree::kOk) {
      lf = w.cur;
      used[m] = us;
      gap[m] = w.min_gap;
    } else {
      ch = -1;
      ls = 0;
    }
  }
  status[m] = st;
  leaf[m] = lf;
  child[m] = ch;
  len_s[m] = ls;
  if (sel_trace != nullptr) sel_trace[m] = lf;
}

// grid M, block 64.  q (M, A) float32 and ok (M,) as plan_finish_k / plan_prep_k wrote them.  A tree plan_prep_k flagged (an action
// index out of range) gets status 2 and its slot allocation back, and its walk's gap does not enter min_gap.
__global__ __launch_bounds__(64) void plan_tree_backprop_k(int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used,
                                                           double* min_gap, int* status, const int* __restrict__ leaf,
                                                           const int* __restrict__ child, const double* __restrict__ gap,
                                                           const float* __restrict__ q, const int* __restrict__ ok, int cap, int A, int D) {
  const int m = blockIdx.x, lane = threadIdx.x;
  if (status[m] != plan_tree::kOk) return;
  const plan_tree::Tree t = plan_tree_rows(first, parent, depth, Ns, Nsa, Qsa, m, cap, A, D);
  const int lf = leaf[m], ch = child[m];
  if (!ok[m]) {
    if (lane == 0) {
      status[m] = plan_tree::kBad;
      if (t.first[lf] < 0) used[m] -= A;
    }
    return;
  }
  const float* qm = q + (size_t)m * A;
  if (lane < A) plan_tree::init_child(t, lf, ch, lane, (double)qm[lane]);
  if (lane == 0) {
    plan_tree::walk_up(t, lf, ch, plan_tree::mean_value(qm, A));
    if (gap[m] < min_gap[m]) min_gap[m] = gap[m];
  }
}

// (best_action reads first and Nsa only)
__global__ __launch_bounds__(64) void plan_tree_action_k(int* first, int* Nsa, int* __restrict__ action, int M, int cap, int A) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  const size_t o = (size_t)m * cap;
  action[m] = plan_tree::best_action(plan_tree::Tree{first + o, nullptr, nullptr, nullptr, Nsa + o, nullptr, cap, A, 0});
}

}  // namespace stove
