// The PPO arm's collection on states, one launch per batch of trajectories (stove_ppo_collect, capi.hip).  The arithmetic is
// csrc/ppo_policy.h's and csrc/env_step.h's, the text the CPU driver runs.  One wave per environment, kPpoWaves environments per block,
// all S steps, next_value and the returns in the launch.  The chain of one environment is serial -- observation, six small layers, the
// draw, the step -- and latency-bound, so a layer's neurons are spread over the wave's lanes (neuron j on lane j % 64, its sum whole and
// in order on that lane) and the activations go from layer to layer through the wave's LDS rows; the draw and the float64 environment
// step run on lane 0 on the wave's state rows in LDS.  The parameter image is transposed (ppo_policy.h), so the lanes of a wave read
// neighbouring words of it.  kStaged: the block copies the image into LDS once and every step reads it there; otherwise (an image
// that does not fit beside the rows) it is read from global memory through the cache at every step.
// Every wave of a block walks the same S + 1 rounds and meets every barrier, whether its environment exists, stopped or runs; what a
// wave does between two barriers is guarded by a wave-uniform flag.  Plain vector stores only, no atomics.
#include "common.h"
#include "ppo_policy.h"

namespace stove {

constexpr int kPpoWaves = 4, kPpoThreads = kPpoWaves * kWave;
constexpr int kPpoStateDoubles = 6 * env_step::kMaxObjects;                        // x, v (2 N each), r, m (N each)
constexpr int kPpoObsFloats = 32, kPpoHeadFloats = 16;                             // (4 N <= 24 and 10, padded)
constexpr int kPpoWaveFloats = kPpoObsFloats + 2 * ppo_policy::kMaxWidth + kPpoHeadFloats;
constexpr size_t kPpoRowBytes = (size_t)kPpoWaves * (kPpoStateDoubles * sizeof(double) + kPpoWaveFloats * sizeof(float));
constexpr size_t kPpoLdsLimit = 160 * 1024;                                        // one CU's LDS, all of which one block may take
static_assert(4 * env_step::kMaxObjects <= kPpoObsFloats && ppo_policy::kHeads <= kPpoHeadFloats, "the rows hold the widest case");
static_assert(ppo_policy::kBase0 <= ppo_policy::kMaxWidth && ppo_policy::kMaxHidden <= ppo_policy::kMaxWidth, "so do the activations");

// the image is staged when it fits beside the blocks' rows
inline bool ppo_staged(size_t n_params) { return kPpoRowBytes + n_params * sizeof(float) <= kPpoLdsLimit; }
inline size_t ppo_lds_bytes(size_t n_params) { return kPpoRowBytes + (ppo_staged(n_params) ? n_params * sizeof(float) : 0); }

// grid ceil(B / kPpoWaves), block kPpoThreads, dynamic LDS ppo_lds_bytes.  x, v (B, N, 2) double in/out; r, m (B, N) double; params the
// image; u (B, S); obs (B, S + 1, 4 N); actions, rewards, values, logp, returns (B, S); next_value, status (B,).
template <bool kStaged>
__global__ __launch_bounds__(kPpoThreads) void ppo_collect_k(double* x, double* v, const double* __restrict__ r, const double* __restrict__ m,
                                                             const float* __restrict__ params, const float* __restrict__ u, float* obs,
                                                             int* actions, float* rewards, float* values, float* logp, float* next_value,
                                                             float* returns, int* status, env_step::Params p, ppo_policy::Shape sh, int B, int S,
                                                             float discount, int n_params) {
  extern __shared__ __attribute__((aligned(16))) double ppo_lds[];
  const int w = wave_id(), lane = lane_id();
  float* rows = reinterpret_cast<float*>(ppo_lds + kPpoWaves * kPpoStateDoubles);
  const float* wts = params;
  if (kStaged) {
    float* img = rows + kPpoWaves * kPpoWaveFloats;
    for (int i = (int)threadIdx.x; i < n_params; i += kPpoThreads) img[i] = params[i];
    wts = img;
  }
  const int N = p.N, W = 4 * N, L = ppo_policy::layers(sh);
  double* xs = ppo_lds + w * kPpoStateDoubles;
  double *vs = xs + 2 * N, *rs = xs + 4 * N, *ms = xs + 5 * N;
  float* o = rows + w * kPpoWaveFloats;
  float *a = o + kPpoObsFloats, *b = a + ppo_policy::kMaxWidth, *heads = b + ppo_policy::kMaxWidth;
  const int e = (int)blockIdx.x * kPpoWaves + w;
  const bool live = e < B;
  const size_t env = live ? (size_t)e : 0;
  if (live) {
    if (lane < 2 * N) {
      xs[lane] = x[env * 2 * N + lane];
      vs[lane] = v[env * 2 * N + lane];
    }
    if (lane < N) {
      rs[lane] = r[env * N + lane];
      ms[lane] = m[env * N + lane];
    }
  }
  __syncthreads();
  bool going = live;
  for (int t = 0; t <= S; ++t) {
    if (going && lane < W) o[lane] = ppo_policy::observe(xs, vs, lane);
    __syncthreads();
    const float* in = o;
    for (int l = 0; l < L; ++l) {
      const int K = ppo_policy::width_in(sh, l), J = ppo_policy::width_out(sh, l);
      const float* wT = wts + ppo_policy::offset(sh, l);
      float* out = l == L - 1 ? heads : (l & 1) ? b : a;
      if (going)
        for (int j = lane; j < J; j += kWave) out[j] = ppo_policy::neuron(wT, wT + (size_t)K * J, in, K, J, j, l != L - 1);
      __syncthreads();
      in = out;
    }
    if (going && !ppo_policy::heads_finite(heads)) going = false;          // (every lane reads the same ten words)
    if (going) {
      if (lane < W) obs[(env * (S + 1) + t) * W + lane] = o[lane];
      if (lane == 0) {
        if (t < S) {
          const size_t at = env * S + t;
          float lp, rew;
          double margin;
          values[at] = heads[0];
          actions[at] = ppo_policy::act(xs, vs, rs, ms, p, heads, u[at], &lp, &rew, &margin);
          logp[at] = lp;
          rewards[at] = rew;
        } else {
          next_value[env] = heads[0];
          ppo_policy::discounted(rewards + env * S, heads[0], discount, S, returns + env * S);
        }
      }
    }
    __syncthreads();
  }
  if (live) {
    if (lane < 2 * N) {
      x[env * 2 * N + lane] = xs[lane];
      v[env * 2 * N + lane] = vs[lane];
    }
    if (lane == 0) status[env] = going ? ppo_policy::kOk : ppo_policy::kNonFinite;
  }
}

}  // namespace stove
