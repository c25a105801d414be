// A batch of avoidance / billiards environments stepped and rendered in place (stove_env_step, capi.hip).  The arithmetic is
// csrc/env_step.h's, the text the CPU driver runs.  One workgroup per environment: a step is one chain of dependent float64
// operations over N <= 6 balls, so lane 0 runs it serially on an LDS copy of the environment's rows and writes them back; after a
// barrier all lanes render the frame from that copy, one pixel (three channels) per lane-iteration, each channel plane written with
// consecutive lanes on consecutive floats.  An environment whose action index is out of range gets status 2 and nothing else of it
// is written.  Plain vector loads and stores, no atomics.
#include "common.h"
#include "env_step.h"

namespace stove {

constexpr int kEnvThreads = 256;

// grid M, block kEnvThreads.  x, v (M, N, 2), r, m (M, N) double; action (M,) or NULL; collisions, status (M,); frames
// (M, 3, res, res) float or NULL
__global__ __launch_bounds__(kEnvThreads) void env_step_k(double* x, double* v, const double* __restrict__ r, const double* __restrict__ m,
                                                          const int* __restrict__ action, int* collisions, int* status, float* frames,
                                                          env_step::Params p, int res, int use_colors) {
  __shared__ double sx[2 * env_step::kMaxObjects], sv[2 * env_step::kMaxObjects], sr[env_step::kMaxObjects], sm[env_step::kMaxObjects];
  __shared__ int st;
  const size_t e = blockIdx.x;
  const int N = p.N;
  if (threadIdx.x == 0) {
    for (int k = 0; k < 2 * N; ++k) {
      sx[k] = x[e * 2 * N + k];
      sv[k] = v[e * 2 * N + k];
    }
    for (int i = 0; i < N; ++i) {
      sr[i] = r[e * N + i];
      sm[i] = m[e * N + i];
    }
    int hit = 0;
    const int s = env_step::step(sx, sv, sr, sm, p, action != nullptr ? action + e : nullptr, &hit);
    if (s == env_step::kOk) {
      for (int k = 0; k < 2 * N; ++k) {
        x[e * 2 * N + k] = sx[k];
        v[e * 2 * N + k] = sv[k];
      }
      collisions[e] = hit;
    }
    status[e] = s;
    st = s;
  }
  __syncthreads();
  if (frames == nullptr || st != env_step::kOk) return;
  const size_t plane = (size_t)res * res;
  float* out = frames + e * 3 * plane;
  for (size_t px = threadIdx.x; px < plane; px += kEnvThreads) {
    const int a = (int)(px / res), b = (int)(px % res);
    float rgb[3];
    env_step::pixel(sx, sr, N, use_colors, env_step::centre(b, res, p.hw), env_step::centre(a, res, p.hw), rgb);
    out[px] = rgb[0];
    out[plane + px] = rgb[1];
    out[2 * plane + px] = rgb[2];
  }
}

}  // namespace stove
