// Tree search on the true environment, one launch per planning step (stove_env_search, capi.hip).  The arithmetic is
// csrc/env_search.h's and csrc/env_step.h's, the text the CPU driver runs.  One lane per tree, 64 trees per wave, all `runs`
// iterations in the launch: an iteration replays its path from the root, so every tree of a wave is at step k of iteration i at the
// same time and the wave diverges only on what kind of step it is and inside `collide`.  Templated on N so that the root state, the
// working state and r, m are registers (N is a constant in every loop over the balls); the tree arrays live in global memory, each tree
// read and written by its own lane only, with plain vector loads and stores.  No atomics, no LDS.
#include "common.h"
#include "env_search.h"

namespace stove {

constexpr int kEnvSearchThreads = 64;

// grid ceil(T / 64), block 64; T = M R trees, tree t searches from environment t / R.  x, v (M, N, 2), r, m (M, N) double (read only);
// draws (T, runs, D); first .. Qsa (T, cap); used, status (T,) int; min_gap (T,) double.  A tree whose status is not 0 is left alone.
template <int N>
__global__ __launch_bounds__(kEnvSearchThreads) void env_search_k(const double* __restrict__ x, const double* __restrict__ v,
                                                                  const double* __restrict__ r, const double* __restrict__ m,
                                                                  const int* __restrict__ draws, int* first, int* parent, int* depth, int* Ns,
                                                                  int* Nsa, double* Qsa, int* used, double* min_gap, int* status,
                                                                  env_step::Params p, int T, int R, int runs, int cap, int D) {
  const int t = blockIdx.x * kEnvSearchThreads + threadIdx.x;
  if (t >= T) return;
  int st = status[t];
  if (st != env_search::kOk) return;
  const size_t e = (size_t)(t / R);
  double x0[2 * N], v0[2 * N], xw[2 * N], vw[2 * N], rr[N], mm[N];
#pragma unroll
  for (int k = 0; k < 2 * N; ++k) {
    x0[k] = x[e * 2 * N + k];
    v0[k] = v[e * 2 * N + k];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rr[i] = r[e * N + i];
    mm[i] = m[e * N + i];
  }
  p.N = N;
  const size_t o = (size_t)t * cap;
  const env_search::Tree tree{first + o, parent + o, depth + o, Ns + o, Nsa + o, Qsa + o, cap, env_search::kActions, D};
  int us = used[t];
  double gap = min_gap[t];
  const int* row = draws + (size_t)t * runs * D;
  for (int i = 0; i < runs && st == env_search::kOk; ++i) st = env_search::iterate(tree, &us, x0, v0, rr, mm, xw, vw, p, row + (size_t)i * D, &gap);
  used[t] = us;
  min_gap[t] = gap;
  status[t] = st;
}

// the launch of env_search_k<N> (capi.hip picks N)
template <int N>
void env_search_launch(hipStream_t st, int T, const double* x, const double* v, const double* r, const double* m, const int* draws, int* first,
                       int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap, int* status,
                       const env_step::Params& p, int R, int runs, int cap, int D) {
  STOVE_LAUNCH(env_search_k<N>, dim3((T + kEnvSearchThreads - 1) / kEnvSearchThreads), dim3(kEnvSearchThreads), 0, st, x, v, r, m, draws, first,
               parent, depth, Ns, Nsa, Qsa, used, min_gap, status, p, T, R, runs, cap, D);
}

// grid ceil(M / 64), block 64: action[e] = first-index argmax of the root counts summed over environment e's R trees
__global__ __launch_bounds__(kEnvSearchThreads) void env_search_action_k(const int* __restrict__ first, const int* __restrict__ Nsa,
                                                                         int* __restrict__ action, int M, int R, int cap) {
  const int e = blockIdx.x * kEnvSearchThreads + threadIdx.x;
  if (e >= M) return;
  int counts[env_search::kActions];
#pragma unroll
  for (int a = 0; a < env_search::kActions; ++a) counts[a] = 0;
  for (int k = 0; k < R; ++k) {
    const size_t o = ((size_t)e * R + k) * cap;
    env_search::add_root_counts(first + o, Nsa + o, cap, counts);
  }
  action[e] = env_search::best_of(counts);
}

}  // namespace stove
