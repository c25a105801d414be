// Starts and action rows of B training sequences drawn in one launch (stove_env_draw_starts, capi.hip) from the counter-based
// stream of csrc/env_draw.h, the text the CPU driver runs.  One wave per sequence, four sequences per workgroup.  A start is the
// good attempt with the LOWEST index, and a six-ball billiards start needs thousands of attempts: the 64 lanes test 64 consecutive
// attempts per round, each lane its own (N Philox blocks, the inside and the pair tests, in registers), and a ballot's lowest set
// bit names the attempt taken.  The lane that holds it then draws the velocities (it has the positions in registers: gravity's
// velocities need them) and writes the sequence's x0, v0, tries and status.  For the action row the lanes take steps in chunks of
// 64: each lane draws its step's uniform and tabulates next_state(c, p, u) for the nine states c in 36 bits; the chain over the
// current state then is 64 lane reads and table lookups, and every lane stores its own step.  No LDS, no barrier, no atomics;
// plain vector loads and stores.
#include "common.h"
#include "env_draw.h"

namespace stove {

constexpr int kDrawThreads = 256, kDrawWaves = kDrawThreads / 64;

// grid ceil(B / 4), block kDrawThreads.  r (B, N) double; x0, v0 (B, N, 2) double; actions (B, T) or NULL; tries, status (B,)
template <int N>
__global__ __launch_bounds__(kDrawThreads) void env_draw_starts_k(const double* __restrict__ r, double* __restrict__ x0,
                                                                  double* __restrict__ v0, int* __restrict__ actions,
                                                                  int* __restrict__ tries, int* __restrict__ status, uint64_t seed0, int B,
                                                                  int T, int kind, int max_tries, double hw, double factor) {
  const int lane = threadIdx.x & 63;
  const size_t e = (size_t)blockIdx.x * kDrawWaves + (threadIdx.x >> 6);
  if (e >= (size_t)B) return;          // (whole waves leave: a wave shares its sequence)
  const uint64_t seed = seed0 + e;
  double rr[N], x[2 * N];
#pragma unroll
  for (int i = 0; i < N; ++i) rr[i] = r[e * N + i];
  const uint32_t limit = kind == 1 ? (uint32_t)env_draw::kGravityTries : (uint32_t)max_tries;
  int taken = -1;
  bool mine = false;
  for (uint32_t base = 0; base < limit; base += 64) {          // (limit < 2^31: base + 64 does not wrap)
    const uint32_t k = base + (uint32_t)lane;
    bool good = kind == 1 ? env_draw::gravity_attempt<N>(seed, k, hw, x) : env_draw::billiards_attempt<N>(seed, k, rr, hw, x);
    good = good && k < limit;
    const unsigned long long vote = __ballot(good);
    if (vote != 0ull) {
      const int win = __ffsll(vote) - 1;
      taken = (int)base + win;
      mine = lane == win;
      break;
    }
  }
  if (taken < 0 && kind == 1) {          // GravityEnv.init_x keeps its last attempt: the last round left it in lane 999 % 64
    taken = env_draw::kGravityTries - 1;
    mine = lane == (env_draw::kGravityTries - 1) % 64;
  }
  double* xrow = x0 + e * 2 * N;
  double* vrow = v0 + e * 2 * N;
  if (taken >= 0) {
    if (mine) {
      double v[2 * N];
      if (kind == 1)
        env_draw::gravity_velocity<N>(seed, x, factor, v);
      else
        env_draw::billiards_velocity<N>(seed, factor, v);
#pragma unroll
      for (int c = 0; c < 2 * N; ++c) {
        xrow[c] = x[c];
        vrow[c] = v[c];
      }
      tries[e] = taken + 1;
      status[e] = env_draw::kOk;
    }
  } else if (lane < 2 * N) {
    xrow[lane] = 0.0;
    vrow[lane] = 0.0;
    if (lane == 0) {
      tries[e] = max_tries;
      status[e] = env_draw::kNoStart;
    }
  }
  if (actions == nullptr) return;
  const double p = env_draw::change_prob(seed);
  int cur = env_draw::first_state(seed);
  for (int base = 0; base < T; base += 64) {
    const int s = base + lane;
    const double u = env_draw::action_uniform(seed, (uint32_t)s);
    uint32_t lo = 0u, hi = 0u;          // next_state(c, p, u) of c = 0 .. 7 in four bits each, of c = 8 in `hi`
#pragma unroll
    for (int c = 0; c < 8; ++c) lo |= (uint32_t)env_draw::next_state(c, p, u) << (4 * c);
    hi = (uint32_t)env_draw::next_state(8, p, u);
    const int n = T - base < 64 ? T - base : 64;
    int my = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t tl = (uint32_t)__shfl((int)lo, j), th = (uint32_t)__shfl((int)hi, j);
      cur = cur < 8 ? (int)((tl >> (4 * cur)) & 15u) : (int)th;
      if (lane == j) my = cur;
    }
    if (s < T) actions[e * T + s] = my;
  }
}

}  // namespace stove
