// The PPO arm's collection on images, one launch per batch of trajectories (stove_ppo_collect_images, capi.hip).  The arithmetic is
// csrc/ppo_image.h's, csrc/ppo_policy.h's and csrc/env_step.h's, the text the CPU driver runs.  One workgroup of kImgThreads threads per
// environment; the warm-up, all S steps, next_value and the returns run inside it.  Per step the chain is frame window -> conv1 ->
// conv2 -> head.main [-> two deep layers] -> heads -> draw -> float64 step -> render, each stage behind a barrier:
//   the convolutions' outputs are spread over the threads as tiles of kTile neighbouring maps of one position (the kTile sums side by
//   side give the ILP and share each input word; every sum stays whole and in order), reading the frame ring and BOTH convolutions'
//   transposed weight images from LDS, where the block copies them once;
//   head.main, the deep layers and the heads are one neuron per thread, their images read from global memory through the cache at every
//   step (the transposed layout makes a wave's lanes read neighbouring words) in batches of 32 loads, the next batch in flight while
//   this one is added up (ppo_image::neuron): the one serial sum waits for memory once per batch, not once per term;
//   the draw and the environment step run on thread 0 on the environment's float64 rows in LDS;
//   all threads render the 1024 pixels of the new frame, to global memory and, divided by 255, into the ring slot of the oldest frame.
// LDS (kImgLdsBytes): the rows, the position history of the first window, heads, two activation rows of 512, conv2's 1568 and conv1's
// 7200 outputs, the ring of F frames, the two weight images: 150752 bytes at F = 4, of the 160 KiB one workgroup may take.
// Every wave walks the same warm + S + 1 rounds and meets every barrier, whether its environment stopped or runs; what happens between
// two barriers is guarded by `going`, which every thread derives from the same LDS words and is therefore uniform over the workgroup.
// Plain vector stores only, no atomics.
#include "common.h"
#include "ppo_image.h"

namespace stove {

constexpr int kImgThreads = 512;
constexpr int kImgDoubles = 6 * env_step::kMaxObjects + ppo_image::kMaxFrames * 2 * env_step::kMaxObjects;          // rows, history
constexpr int kImgHeadFloats = 16;
static_assert(ppo_image::kMaxHidden <= kImgThreads, "head.main and the deep layers are one neuron per thread");
static_assert(ppo_image::kPlane % kImgThreads == 0 && ppo_policy::kHeads <= kImgHeadFloats, "the render and the heads' row");

__host__ __device__ inline size_t img_conv_floats(int F) { return (size_t)(48 * F + 1) * ppo_image::kMaps + (size_t)(9 * ppo_image::kMaps + 1) * ppo_image::kMaps; }
inline size_t img_lds_bytes(int F) {
  return kImgDoubles * sizeof(double) + (kImgHeadFloats + 2 * ppo_image::kMaxHidden + ppo_image::kFlat + ppo_image::kConv1Floats +
                                         (size_t)F * ppo_image::kFrameFloats + img_conv_floats(F)) * sizeof(float);
}

// grid B, block kImgThreads, dynamic LDS img_lds_bytes(F).  x, v (B, N, 2) double in/out; r, m (B, N) double; params the image; u (B, S);
// frames (B, F + S, 3, 32, 32); actions, rewards, values, logp, returns (B, S); next_value, status (B,).
__global__ __launch_bounds__(kImgThreads) void ppo_collect_images_k(double* x, double* v, const double* __restrict__ r, const double* __restrict__ m,
                                                                    const float* __restrict__ params, const float* __restrict__ u, float* frames,
                                                                    int* actions, float* rewards, float* values, float* logp, float* next_value,
                                                                    float* returns, int* status, env_step::Params p, ppo_image::Shape sh, int S,
                                                                    int warm, int use_colors, float discount) {
  using namespace ppo_image;
  extern __shared__ __attribute__((aligned(16))) double img_lds[];
  const int tid = (int)threadIdx.x, N = p.N, F = sh.F, L = layers(sh);
  double* xs = img_lds;
  double *vs = xs + 2 * N, *rs = xs + 4 * N, *ms = xs + 5 * N, *hist = img_lds + 6 * env_step::kMaxObjects;
  float* heads = reinterpret_cast<float*>(img_lds + kImgDoubles);
  float *a = heads + kImgHeadFloats, *b = a + kMaxHidden, *c2 = b + kMaxHidden, *c1 = c2 + kFlat, *ring = c1 + kConv1Floats;
  float* w1 = ring + (size_t)F * kFrameFloats;
  float* w2 = w1 + (size_t)(48 * F + 1) * kMaps;
  const float *b1 = w1 + (size_t)48 * F * kMaps, *b2 = w2 + (size_t)9 * kMaps * kMaps;
  const size_t env = blockIdx.x;
  float* rows = frames + env * (size_t)(F + S) * kFrameFloats;

  const int n_conv = (int)img_conv_floats(F);
  for (int i = tid; i < n_conv; i += kImgThreads) w1[i] = params[i];          // (the two images follow each other in `params` too)
  for (int i = tid; i < F * kFrameFloats; i += kImgThreads) ring[i] = 0.0f;
  if (tid < 2 * N) {
    xs[tid] = x[env * 2 * N + tid];
    vs[tid] = v[env * 2 * N + tid];
  }
  if (tid < N) {
    rs[tid] = r[env * N + tid];
    ms[tid] = m[env * N + tid];
  }
  __syncthreads();
  for (int w = 0; w < warm; ++w) {
    if (tid == 0) warm_step(xs, vs, rs, ms, p, F, warm, w, hist);
    __syncthreads();
    const int row = F - warm + w;
    if (row >= 0)
      for (int px = tid; px < kPlane; px += kImgThreads) render_pixel(xs, rs, N, use_colors, p.hw, px, nullptr, ring + (size_t)row * kFrameFloats);
    __syncthreads();
  }
  bool going = true;
  for (int t = 0; t <= S; ++t) {
    const int first = t % F;
    if (going)
      for (int i = tid; i < kConv1Items; i += kImgThreads) conv1_item(w1, b1, ring, first, F, i, c1);
    __syncthreads();
    if (going && tid < kConv2Items) conv2_item(w2, b2, c1, tid, c2);
    __syncthreads();
    const float* in = c2;
    for (int l = 2; l < L; ++l) {
      const int K = width_in(sh, l), J = width_out(sh, l);
      const float* wT = params + offset(sh, l);
      float* out = l == L - 1 ? heads : (l & 1) ? b : a;
      if (going && tid < J) out[tid] = neuron(wT, wT + (size_t)K * J, in, K, J, tid, l != L - 1);
      __syncthreads();
      in = out;
    }
    if (going && !ppo_policy::heads_finite(heads)) going = false;          // (every thread reads the same ten words)
    if (going) {
      if (t == 0)
        for (int q = 0; q < F; ++q)
          for (int px = tid; px < kPlane; px += kImgThreads) first_window_pixel(hist, rs, N, use_colors, p.hw, F, warm, q, px, rows);
      if (tid == 0) {
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
    if (going && t < S)
      for (int px = tid; px < kPlane; px += kImgThreads)
        render_pixel(xs, rs, N, use_colors, p.hw, px, rows + (size_t)(F + t) * kFrameFloats, ring + (size_t)first * kFrameFloats);
    __syncthreads();
  }
  if (tid < 2 * N) {
    x[env * 2 * N + tid] = xs[tid];
    v[env * 2 * N + tid] = vs[tid];
  }
  if (tid == 0) status[env] = going ? ppo_policy::kOk : ppo_policy::kNonFinite;
}

}  // namespace stove
