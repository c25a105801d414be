// The model-free PPO arm's collection on IMAGES (stove_amd/rl/collect.py: ImageForest -- that file is the specification) on ONE
// environment's rows, as plain inline functions on top of env_step.h and ppo_policy.h: __host__ __device__ under hipcc (the kernel of
// ppo_image.hip calls them), unmarked under a host compiler (tests/abi/ppo_image_driver.cpp runs the same text on the CPU under
// sanitizers).  Per step: the window of the last F rendered frames, the policy `Policy(obs_shape=(32, 32, 3F))` of
// stove_amd/rl/rl_model.py -- frame / 255, Conv2d(3F, 32, 4, stride 2), ReLU, Conv2d(32, 32, 3, stride 2), ReLU, flatten (1568),
// Linear(1568, H), ReLU [, Linear(H, H), ReLU, Linear(H, H), ReLU], then the value and the nine logits --, the draw of ppo_policy.h
// from a uniform the caller supplies, the environment step, the reward, the new frame.  The frame side is 32: the flattened width
// 32 * 7 * 7 fixes it.
//
// Everything but exp and log (the draw, the frame) must equal the numpy restatement bit for bit: a neuron or a convolution output is
// ONE float32 sum that starts at its bias and adds w[k] * in[k] for k ascending, multiply and add rounded separately (ppo_policy.h
// says how contraction is kept off).  The input of the first convolution is frame / 255.0f, one float32 division per pixel (the
// reference divides frames that are already in [0, 1]; kept).
//
// The parameter image (param_floats(shape) floats; Policy.flat_image_params() writes it): the layers in order, each as its TRANSPOSED
// weight wT[k * out + j] followed by its bias (out):
//   base.main.0 (48 F -> 32), k = (c * 4 + ky) * 4 + kx, input channel c = f * 3 + ch with f counted from the OLDEST frame of the window;
//   base.main.2 (288 -> 32), k = (c * 3 + ky) * 3 + kx;
//   head.main (1568 -> H), k = c * 49 + y * 7 + x (torch's flatten);
//   [head.in_between.0 (H -> H), head.in_between.2 (H -> H),]
//   heads (H -> 10): column 0 head.values_head, columns 1 .. 9 head.actor_head, as in ppo_policy.h.
//
// The frames of one environment are rows of (3, 32, 32) floats in the layout stove_env_step writes; row q of the F + S rows is kept, already
// divided, in slot q % F of a ring of F frames.  Rows 0 .. F - 1 are the first window: the last min(warm, F) of the `warm` frames
// rendered after the warm-up steps with action 0, zeros before them.  Row F + s is the frame after step s; step s reads rows s .. s + F - 1.
#pragma once
#include "ppo_policy.h"

namespace ppo_image {

using ppo_policy::kHeads;
using ppo_policy::kNonFinite;
using ppo_policy::kOk;

constexpr int kRes = 32, kPlane = kRes * kRes, kFrameFloats = 3 * kPlane, kMaxFrames = 4, kMaxHidden = 512;
constexpr int kMaps = 32, kSide1 = 15, kSide2 = 7;                                   // both convolutions' maps; their output sides
constexpr int kConv1Floats = kMaps * kSide1 * kSide1, kFlat = kMaps * kSide2 * kSide2;
constexpr int kTile = 4;                                                             // outputs one conv call computes side by side

struct Shape {
  int F, H, deep;
};

PPO_FN int layers(const Shape& s) { return s.deep ? 6 : 4; }
PPO_FN int width_in(const Shape& s, int l) { return l == 0 ? 48 * s.F : l == 1 ? 9 * kMaps : l == 2 ? kFlat : s.H; }
PPO_FN int width_out(const Shape& s, int l) { return l < 2 ? kMaps : l == layers(s) - 1 ? kHeads : s.H; }
// where layer l's transposed weight starts in the image; its bias follows at + in * out
PPO_FN size_t offset(const Shape& s, int l) {
  size_t o = 0;
  for (int k = 0; k < l; ++k) o += (size_t)(width_in(s, k) + 1) * (size_t)width_out(s, k);
  return o;
}
PPO_FN size_t param_floats(const Shape& s) { return offset(s, layers(s)); }
PPO_FN bool served(const Shape& s) { return s.F >= 1 && s.F <= kMaxFrames && s.H >= 1 && s.H <= kMaxHidden; }

PPO_FN float scaled(float pixel) { return pixel / 255.0f; }
PPO_FN float relu(float acc) { return acc < 0.0f ? 0.0f : acc; }          // (keeps a NaN)

// plane of input channel c of the window whose oldest frame sits in slot `first` of the ring
PPO_FN const float* channel(const float* ring, int first, int F, int c) {
  const int f = c / 3;
  int slot = first + f;
  if (slot >= F) slot -= F;
  return ring + (size_t)slot * kFrameFloats + (size_t)(c - 3 * f) * kPlane;
}

// outputs (o .. o + R - 1, y, x) of the first convolution: R sums side by side, each whole and in order
template <int R>
PPO_FN void conv1(const float* wT, const float* bias, const float* ring, int first, int F, int o, int y, int x, float* out) {
  PPO_NO_CONTRACT
  float acc[R];
  for (int q = 0; q < R; ++q) acc[q] = bias[o + q];
  const float* w = wT + o;
  for (int c = 0; c < 3 * F; ++c) {
    const float* in = channel(ring, first, F, c) + 2 * y * kRes + 2 * x;
    for (int ky = 0; ky < 4; ++ky)
      for (int kx = 0; kx < 4; ++kx) {
        const float pix = in[ky * kRes + kx];
        for (int q = 0; q < R; ++q) {
          const float p = w[q] * pix;
          acc[q] = acc[q] + p;
        }
        w += kMaps;
      }
  }
  for (int q = 0; q < R; ++q) out[q] = relu(acc[q]);
}

// outputs (o .. o + R - 1, y, x) of the second convolution on the first one's maps c1 (32, 15, 15)
template <int R>
PPO_FN void conv2(const float* wT, const float* bias, const float* c1, int o, int y, int x, float* out) {
  PPO_NO_CONTRACT
  float acc[R];
  for (int q = 0; q < R; ++q) acc[q] = bias[o + q];
  const float* w = wT + o;
  for (int c = 0; c < kMaps; ++c) {
    const float* in = c1 + (c * kSide1 + 2 * y) * kSide1 + 2 * x;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) {
        const float val = in[ky * kSide1 + kx];
        for (int q = 0; q < R; ++q) {
          const float p = w[q] * val;
          acc[q] = acc[q] + p;
        }
        w += kMaps;
      }
  }
  for (int q = 0; q < R; ++q) out[q] = relu(acc[q]);
}

// item i of the first / second convolution's kMaps / kTile * side * side tiles: kTile neighbouring maps of one position
PPO_FN void conv1_item(const float* wT, const float* bias, const float* ring, int first, int F, int i, float* c1) {
  const int o = (i % (kMaps / kTile)) * kTile, pos = i / (kMaps / kTile);
  float out[kTile];
  conv1<kTile>(wT, bias, ring, first, F, o, pos / kSide1, pos % kSide1, out);
  for (int q = 0; q < kTile; ++q) c1[(o + q) * kSide1 * kSide1 + pos] = out[q];
}
PPO_FN void conv2_item(const float* wT, const float* bias, const float* c1, int i, float* c2) {
  const int o = (i % (kMaps / kTile)) * kTile, pos = i / (kMaps / kTile);
  float out[kTile];
  conv2<kTile>(wT, bias, c1, o, pos / kSide2, pos % kSide2, out);
  for (int q = 0; q < kTile; ++q) c2[(o + q) * kSide2 * kSide2 + pos] = out[q];
}
constexpr int kConv1Items = kMaps / kTile * kSide1 * kSide1, kConv2Items = kMaps / kTile * kSide2 * kSide2;

// ppo_policy::neuron -- the same operations in the same order -- for an image that is read from far away: the weights come in batches
// of kBatch loads that do not depend on the sum, and the next batch is asked for before this one is added up, so that the one
// serial sum waits for memory once per batch and not once per term
constexpr int kBatch = 32;
PPO_FN float neuron(const float* wT, const float* bias, const float* x, int in, int out, int j, bool relu_after) {
  PPO_NO_CONTRACT
  float acc = bias[j];
  const float* col = wT + j;
  float w[kBatch] = {0.0f}, ahead[kBatch] = {0.0f};
  int k = 0;
  if (in >= kBatch)
    for (int q = 0; q < kBatch; ++q) w[q] = col[(size_t)q * out];
  for (; k + kBatch <= in; k += kBatch) {
    const bool more = k + 2 * kBatch <= in;
    if (more)
      for (int q = 0; q < kBatch; ++q) ahead[q] = col[(size_t)(k + kBatch + q) * out];
    for (int q = 0; q < kBatch; ++q) {
      const float p = w[q] * x[k + q];
      acc = acc + p;
    }
    if (more)
      for (int q = 0; q < kBatch; ++q) w[q] = ahead[q];
  }
  for (; k < in; ++k) {
    const float p = col[(size_t)k * out] * x[k];
    acc = acc + p;
  }
  return relu_after ? relu(acc) : acc;
}

// the whole policy on one window, one output after the other (the CPU driver; the kernel spreads them over the workgroup).
// c1: kConv1Floats, c2: kFlat, a, b: kMaxHidden floats of working room; heads[0] the value, heads[1 .. 9] the logits.
PPO_FN void forward(const float* params, const Shape& s, const float* ring, int first, float* c1, float* c2, float* a, float* b,
                    float* heads) {
  const float* w1 = params;
  const float* w2 = params + offset(s, 1);
  for (int i = 0; i < kConv1Items; ++i) conv1_item(w1, w1 + (size_t)width_in(s, 0) * kMaps, ring, first, s.F, i, c1);
  for (int i = 0; i < kConv2Items; ++i) conv2_item(w2, w2 + (size_t)width_in(s, 1) * kMaps, c1, i, c2);
  const int L = layers(s);
  const float* in = c2;
  for (int l = 2; l < L; ++l) {
    const int K = width_in(s, l), J = width_out(s, l);
    const float* wT = params + offset(s, l);
    float* out = l == L - 1 ? heads : (l & 1) ? b : a;
    for (int j = 0; j < J; ++j) out[j] = neuron(wT, wT + (size_t)K * J, in, K, J, j, l != L - 1);
    in = out;
  }
}

// pixel px of the frame of the state x: its three channels to `row` (3, 32, 32) as stove_env_step writes them, and divided to `slot`;
// either may be NULL
PPO_FN void render_pixel(const double* x, const double* r, int N, int use_colors, double hw, int px, float* row, float* slot) {
  const int a = px / kRes, b = px % kRes;
  float rgb[3];
  env_step::pixel(x, r, N, use_colors, env_step::centre(b, kRes, hw), env_step::centre(a, kRes, hw), rgb);
  for (int ch = 0; ch < 3; ++ch) {
    if (row != nullptr) row[ch * kPlane + px] = rgb[ch];
    if (slot != nullptr) slot[ch * kPlane + px] = scaled(rgb[ch]);
  }
}

// the warm-up step w of `warm`: action 0, the reward dropped.  Its frame is row F - warm + w of the first window where that is not
// negative: then the positions are kept in `hist` (kMaxFrames rows of 2 * kMaxObjects) for first_window_pixel.  -> that row, or -1
PPO_FN int warm_step(double* x, double* v, const double* r, const double* m, const env_step::Params& p, int F, int warm, int w, double* hist) {
  const int zero = 0;
  int hit = 0;
  env_step::step(x, v, r, m, p, &zero, &hit);
  const int row = F - warm + w;
  if (row < 0) return -1;
  for (int k = 0; k < 2 * p.N; ++k) hist[row * 2 * env_step::kMaxObjects + k] = x[k];
  return row;
}

// pixel px of row q < F of the first window, written once the first decision on it was finite: zeros before the warm-up's frames
PPO_FN void first_window_pixel(const double* hist, const double* r, int N, int use_colors, double hw, int F, int warm, int q, int px,
                               float* frames) {
  float* row = frames + (size_t)q * kFrameFloats;
  if (q < F - warm) {
    for (int ch = 0; ch < 3; ++ch) row[ch * kPlane + px] = 0.0f;
    return;
  }
  render_pixel(hist + q * 2 * env_step::kMaxObjects, r, N, use_colors, hw, px, row, nullptr);
}

// The whole collection of one environment, serially (the CPU driver): frames (F + S rows), actions, rewards, values, logp, returns
// (S,), *next_value; x, v in place.  ring: F * kFrameFloats, c1, c2, a, b as in forward: working room.  *min_margin is lowered to the
// smallest margin of its draws.  -> status; with kNonFinite at step s nothing of that step or after it is written (at s == 0 not even
// the first window) and x, v stand as the steps before -- the warm-up included -- left them.
PPO_FN int collect(double* x, double* v, const double* r, const double* m, const env_step::Params& p, int use_colors, const float* params,
                   const Shape& s, const float* u, float discount, int S, int warm, float* ring, float* c1, float* c2, float* a, float* b,
                   float* frames, int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns,
                   double* min_margin) {
  const int F = s.F;
  double hist[kMaxFrames * 2 * env_step::kMaxObjects] = {0.0};
  float heads[kHeads];
  for (int k = 0; k < F * kFrameFloats; ++k) ring[k] = 0.0f;
  for (int w = 0; w < warm; ++w) {
    const int row = warm_step(x, v, r, m, p, F, warm, w, hist);
    if (row >= 0)
      for (int px = 0; px < kPlane; ++px) render_pixel(x, r, p.N, use_colors, p.hw, px, nullptr, ring + (size_t)row * kFrameFloats);
  }
  for (int t = 0; t <= S; ++t) {
    forward(params, s, ring, t % F, c1, c2, a, b, heads);
    if (!ppo_policy::heads_finite(heads)) return kNonFinite;
    if (t == 0)
      for (int q = 0; q < F; ++q)
        for (int px = 0; px < kPlane; ++px) first_window_pixel(hist, r, p.N, use_colors, p.hw, F, warm, q, px, frames);
    if (t == S) break;
    double margin;
    values[t] = heads[0];
    actions[t] = ppo_policy::act(x, v, r, m, p, heads, u[t], &logp[t], &rewards[t], &margin);
    if (margin < *min_margin) *min_margin = margin;
    for (int px = 0; px < kPlane; ++px)
      render_pixel(x, r, p.N, use_colors, p.hw, px, frames + (size_t)(F + t) * kFrameFloats, ring + (size_t)(t % F) * kFrameFloats);
  }
  *next_value = heads[0];
  ppo_policy::discounted(rewards, heads[0], discount, S, returns);
  return kOk;
}

}  // namespace ppo_image
