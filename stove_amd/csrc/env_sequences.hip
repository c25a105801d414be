// Whole training sequences in one launch (stove_env_sequences, capi.hip): B environments, billiards / avoidance (kind 0) or gravity
// (kind 1), each stepped T times from its start state with every state, frame, collision flag and the acceptance count written out.
// The arithmetic is csrc/env_step.h's and csrc/env_gravity.h's, the text the CPU driver runs.  One workgroup of four waves per
// sequence.  The physics of a sequence is one chain of dependent float64 operations, a frame is res^2 N independent exp evaluations,
// so the two overlap: the state lives in two LDS buffers, and in round q wave 0 computes state q + 1 into buffer (q + 1) & 1 while
// waves 1 .. 3 paint frame q - 1 from state q in buffer q & 1.  One barrier per round, T + 1 rounds, no flags between waves.  Wave 0
// also writes y, collisions and the running in_bounds.  Billiards steps on lane 0 (env_step::step); gravity holds one ball per lane of
// wave 0 in registers and exchanges positions by lane shuffles, every sum still taken in ball order (env_gravity.h's pieces).
// A sequence with an action index outside [0, 9) anywhere in its row gets status 2 and nothing else of it is written.  Plain vector
// loads and stores, no atomics.
#include "common.h"
#include "env_gravity.h"
#include "env_step.h"

namespace stove {

constexpr int kSeqThreads = 256;

// one gravity step of ball `i` held in this lane's registers (x0, x1, v0, v1, m); lanes 0 .. N - 1 of the wave hold balls 0 .. N - 1
// and the lanes beyond repeat ball N - 1, so that every shuffle reads a live lane
__device__ inline void gravity_step_lanes(double& x0, double& x1, double& v0, double& v1, double m, int i, const env_step::Params& p) {
  const int N = p.N;
  const double eps = 1.0 / (double)p.granularity, te = p.t * eps;
  for (int s = 0; s < p.granularity; ++s) {
    x0 = env_gravity::moved(x0, v0, te);
    x1 = env_gravity::moved(x1, v1, te);
    double xs[2 * env_gravity::kMaxObjects], ms[env_gravity::kMaxObjects];
#pragma unroll
    for (int j = 0; j < env_gravity::kMaxObjects; ++j) {
      const int src = j < N ? j : N - 1;
      xs[2 * j] = __shfl(x0, src);
      xs[2 * j + 1] = __shfl(x1, src);
      ms[j] = __shfl(m, src);
    }
    double s0, s1, sm;
    env_gravity::mass_sums(xs, ms, N, &s0, &s1, &sm);
    const double d0 = env_gravity::shift(p.hw, s0, sm), d1 = env_gravity::shift(p.hw, s1, sm);
    x0 = env_gravity::shifted(x0, d0);
    x1 = env_gravity::shifted(x1, d1);
    v0 = env_gravity::slowed(v0, m, p.fric, p.t, eps);
    v1 = env_gravity::slowed(v1, m, p.fric, p.t, eps);
    double f[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < env_gravity::kMaxObjects; ++j) {
      if (j < N && j != i)
        env_gravity::attract(f, x0, x1, env_gravity::shifted(xs[2 * j], d0), env_gravity::shifted(xs[2 * j + 1], d1), m, ms[j]);
    }
    env_gravity::to_middle(f, x0, x1, p.hw);
    v0 = env_gravity::pushed(v0, env_gravity::clipped(f[0]), m, p.t, eps);
    v1 = env_gravity::pushed(v1, env_gravity::clipped(f[1]), m, p.t, eps);
  }
}

// frame of the state x (N, 2): lanes `first`, `first + step`, ... of the block take a pixel each
__device__ inline void paint(float* out, const double* x, const double* r, int N, int res, int use_colors, double hw, int first, int step) {
  const int plane = res * res;
  for (int px = first; px < plane; px += step) {
    const int a = px / res, b = px % res;
    float rgb[3];
    env_step::pixel(x, r, N, use_colors, env_step::centre(b, res, hw), env_step::centre(a, res, hw), rgb);
    out[px] = rgb[0];
    out[plane + px] = rgb[1];
    out[2 * plane + px] = rgb[2];
  }
}

// grid B, block kSeqThreads.  x0, v0 (B, N, 2), r, m (B, N) double; actions (B, T) or NULL; y (B, T, N, 4); frames (B, T, 3, res, res)
// float or NULL; collisions (B, T); in_bounds, status (B,)
__global__ __launch_bounds__(kSeqThreads) void env_sequences_k(const double* __restrict__ x0, const double* __restrict__ v0,
                                                               const double* __restrict__ r, const double* __restrict__ m,
                                                               const int* __restrict__ actions, double* y, float* frames, int* collisions,
                                                               int* in_bounds, int* status, env_step::Params p, int T, int res, int use_colors,
                                                               int kind) {
  constexpr int kRow = 2 * env_step::kMaxObjects;
  __shared__ double sx[2][kRow], sv[2][kRow], sr[env_step::kMaxObjects], sm[env_step::kMaxObjects];
  __shared__ int bad;
  const size_t e = blockIdx.x;
  const int N = p.N, tid = threadIdx.x;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (actions != nullptr) {
    int mine = 0;
    for (int t = tid; t < T; t += kSeqThreads) {
      const int a = actions[e * T + t];
      if (a < 0 || a >= env_step::kActions) mine = 1;
    }
    if (mine) bad = 1;          // (every writer stores the same word)
  }
  if (tid < 2 * N) {
    sx[0][tid] = x0[e * 2 * N + tid];
    sv[0][tid] = v0[e * 2 * N + tid];
  }
  if (tid < N) {
    sr[tid] = r[e * N + tid];
    sm[tid] = m[e * N + tid];
  }
  __syncthreads();
  if (bad) {
    if (tid == 0) status[e] = env_step::kBadAction;
    return;
  }
  const size_t plane3 = (size_t)3 * res * res;
  const bool physics = tid < 64;
  // gravity: lane i of wave 0 keeps ball min(i, N - 1)
  const int ball = tid < N ? tid : N - 1;
  double gx0 = 0.0, gx1 = 0.0, gv0 = 0.0, gv1 = 0.0, gm = 1.0;
  if (physics && kind == 1) {
    gx0 = sx[0][2 * ball];
    gx1 = sx[0][2 * ball + 1];
    gv0 = sv[0][2 * ball];
    gv1 = sv[0][2 * ball + 1];
    gm = sm[ball];
  }
  int count = 0;
  for (int q = 0; q <= T; ++q) {
    const int cur = q & 1, nxt = cur ^ 1;
    if (physics) {
      if (q < T) {
        double* yrow = y + (e * T + q) * 4 * N;
        if (kind == 1) {
          gravity_step_lanes(gx0, gx1, gv0, gv1, gm, ball, p);
          if (tid < N) {
            sx[nxt][2 * tid] = gx0;
            sx[nxt][2 * tid + 1] = gx1;
            yrow[4 * tid] = gx0;
            yrow[4 * tid + 1] = gx1;
            yrow[4 * tid + 2] = gv0;
            yrow[4 * tid + 3] = gv1;
            count += (gx0 > 0.0 && gx0 < p.hw ? 1 : 0) + (gx1 > 0.0 && gx1 < p.hw ? 1 : 0);
          }
          if (tid == 0) collisions[e * T + q] = 0;
        } else if (tid == 0) {
          for (int k = 0; k < 2 * N; ++k) {
            sx[nxt][k] = sx[cur][k];
            sv[nxt][k] = sv[cur][k];
          }
          int hit = 0;
          env_step::step(sx[nxt], sv[nxt], sr, sm, p, actions != nullptr ? actions + e * T + q : nullptr, &hit);
          for (int i = 0; i < N; ++i) {
            yrow[4 * i] = sx[nxt][2 * i];
            yrow[4 * i + 1] = sx[nxt][2 * i + 1];
            yrow[4 * i + 2] = sv[nxt][2 * i];
            yrow[4 * i + 3] = sv[nxt][2 * i + 1];
          }
          collisions[e * T + q] = hit;
          count += env_gravity::inside(sx[nxt], N, p.hw);
        }
      }
    } else if (q >= 1 && frames != nullptr) {
      paint(frames + (e * T + (q - 1)) * plane3, sx[cur], sr, N, res, use_colors, p.hw, tid - 64, kSeqThreads - 64);
    }
    __syncthreads();
  }
  if (physics) {
    if (kind == 1)          // the lanes' counts, summed in lane order (integers: any order gives the same)
      for (int j = 1; j < env_gravity::kMaxObjects; ++j) {
        const int other = __shfl(count, j);
        if (tid == 0 && j < N) count += other;
      }
    if (tid == 0) {
      in_bounds[e] = count;
      status[e] = env_step::kOk;
    }
  }
}

}  // namespace stove
