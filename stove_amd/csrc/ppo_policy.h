// The model-free PPO arm's collection on states (stove_amd/rl/collect.py: PolicyForest -- that file is the specification) on ONE
// environment's rows, as plain inline functions on top of env_step.h: __host__ __device__ under hipcc (the kernel of ppo_collect.hip
// calls them), unmarked under a host compiler (tests/abi/ppo_collect_driver.cpp runs the same text on the CPU under sanitizers).
// Per step: the observation (x, v rounded to float32), the policy `Policy(base='control')` of stove_amd/rl/rl_model.py --
// Linear(4N, 128), ReLU, Linear(128, 32), ReLU, Linear(32, H), ReLU [, Linear(H, H), ReLU, Linear(H, H), ReLU], then the value and the
// nine logits --, a categorical draw from a uniform the caller supplies, the environment step, the reward.
//
// Everything but exp and log (the draw) must equal the numpy restatement bit for bit: a neuron is ONE float32 accumulation that starts
// at its bias and adds w[k] * x[k] for k ascending, multiply and add rounded separately; nothing may be contracted into a fused
// multiply-add.  Under clang (hipcc) each function switches contraction off for its body; a host compiler gets -ffp-contract=off on its
// command line.
//
// The parameter image (param_floats(shape) floats; Policy.flat_params() writes it): the layers in order, each as its TRANSPOSED weight
// wT[k * out + j] = weight[j][k] (in x out, so that the neurons j of one input k are neighbours) followed by its bias (out):
//   base.main.0 (4N -> 128), base.main.2 (128 -> 32), head.main (32 -> H), [head.in_between.0 (H -> H), head.in_between.2 (H -> H),]
//   heads (H -> 10): column 0 head.values_head, columns 1 .. 9 head.actor_head.
#pragma once
#include <math.h>
#include <stddef.h>

#include "env_step.h"

#define PPO_FN ENV_STEP_FN
#define PPO_NO_CONTRACT ENV_STEP_NO_CONTRACT

namespace ppo_policy {

constexpr int kActions = env_step::kActions, kHeads = 1 + kActions;
constexpr int kBase0 = 128, kBase1 = 32, kMaxHidden = 128, kMaxWidth = 128, kMaxLayers = 6;
// status of an environment after a call: collected / a logit or a value was not finite: the environment stopped at that step, nothing
// of that step (or of what follows it) was written and its state stands as the steps before left it
constexpr int kOk = 0, kNonFinite = 3;

struct Shape {
  int N, H, deep;
};

PPO_FN int layers(const Shape& s) { return s.deep ? 6 : 4; }
PPO_FN int width_in(const Shape& s, int l) { return l == 0 ? 4 * s.N : l == 1 ? kBase0 : l == 2 ? kBase1 : s.H; }
PPO_FN int width_out(const Shape& s, int l) { return l == 0 ? kBase0 : l == 1 ? kBase1 : l == layers(s) - 1 ? kHeads : s.H; }
// where layer l's transposed weight starts in the image; its bias follows at + in * out
PPO_FN size_t offset(const Shape& s, int l) {
  size_t o = 0;
  for (int k = 0; k < l; ++k) o += (size_t)(width_in(s, k) + 1) * (size_t)width_out(s, k);
  return o;
}
PPO_FN size_t param_floats(const Shape& s) { return offset(s, layers(s)); }

PPO_FN bool finite(float f) { return __builtin_isfinite(f); }

// obs[4 i .. 4 i + 3] = x[i][0], x[i][1], v[i][0], v[i][1] rounded to float32: entry k of the flattened concatenate([x, v], 1)
PPO_FN float observe(const double* x, const double* v, int k) {
  const int i = k >> 2, c = k & 3;
  return (float)(c < 2 ? x[2 * i + c] : v[2 * i + c - 2]);
}

// The model-based arm's observation (stove_ppo_collect_model; reference runners.py:241-243): entry c of a node's (x, y, vx, vy) from
// column 2 + c of its model state z, positions from [-1, 1] to [0, hw], velocities scaled alike; every operation rounded on its own
PPO_FN float observe_model(float z, int c, float hw) {
  PPO_NO_CONTRACT
  if (c < 2) {
    const float shifted = z + 1.0f;
    const float half = shifted / 2.0f;
    return half * hw;
  }
  const float half = z / 2.0f;
  return half * hw;
}

// neuron j of a layer (in -> out): bias, then + w[k] * x[k] for k ascending; relu keeps a NaN
PPO_FN float neuron(const float* wT, const float* bias, const float* x, int in, int out, int j, bool relu) {
  PPO_NO_CONTRACT
  float acc = bias[j];
  for (int k = 0; k < in; ++k) {
    const float p = wT[(size_t)k * out + j] * x[k];
    acc = acc + p;
  }
  return (relu && acc < 0.0f) ? 0.0f : acc;
}

// the whole policy on one observation, one neuron after the other (the CPU driver; the kernel spreads the neurons of a layer over the
// lanes of a wave).  a, b: kMaxWidth floats of working room each; heads[0] the value, heads[1 .. 9] the logits.
PPO_FN void forward(const float* params, const Shape& s, const float* obs, float* a, float* b, float* heads) {
  const int L = layers(s);
  const float* in = obs;
  for (int l = 0; l < L; ++l) {
    const int K = width_in(s, l), J = width_out(s, l);
    const float* wT = params + offset(s, l);
    float* out = l == L - 1 ? heads : (l & 1) ? b : a;
    for (int j = 0; j < J; ++j) out[j] = neuron(wT, wT + (size_t)K * J, in, K, J, j, l != L - 1);
    in = out;
  }
}

PPO_FN bool heads_finite(const float* heads) {
  bool ok = true;
  for (int a = 0; a < kHeads; ++a) ok = ok && finite(heads[a]);
  return ok;
}

// Categorical(logits).sample() from a uniform u in [0, 1): d_a = l_a - max l in float32, e_a = exp(d_a) in double, c_a their running
// sum; the action is the first a with c_a > u c_8 (8 if there is none), log_prob = d_a - log c_8 rounded to float32.  *margin is
// min_a |c_a - u c_8| / c_8: how far the uniform is from the nearest boundary, in probability.
PPO_FN int draw(const float* logits, float u, float* logp, double* margin) {
  PPO_NO_CONTRACT
  float top = logits[0];
  for (int a = 1; a < kActions; ++a)
    if (logits[a] > top) top = logits[a];
  float d[kActions];
  double c[kActions];
  double run = 0.0;
  for (int a = 0; a < kActions; ++a) {
    d[a] = logits[a] - top;
    run = run + exp((double)d[a]);
    c[a] = run;
  }
  const double thr = (double)u * run;
  int action = kActions - 1;
  for (int a = kActions - 1; a >= 0; --a)
    if (c[a] > thr) action = a;
  double gap = INFINITY;
  for (int a = 0; a < kActions; ++a) {
    const double g = fabs(c[a] - thr) / run;
    if (g < gap) gap = g;
  }
  *margin = gap;
  *logp = (float)((double)d[action] - log(run));
  return action;
}

// returns[s] = returns[s + 1] * discount + rewards[s] from returns[S] = next_value, in float32, multiply and add rounded separately
// (the reference's _calculate_returns with done == 0)
PPO_FN void discounted(const float* rewards, float next_value, float discount, int S, float* returns) {
  PPO_NO_CONTRACT
  float run = next_value;
  for (int s = S - 1; s >= 0; --s) {
    const float scaled = run * discount;
    run = scaled + rewards[s];
    returns[s] = run;
  }
}

// One step of one environment once the policy's ten outputs on its observation are known (and finite): the draw and the environment
// step.  -> the action; *reward = -collisions.
PPO_FN int act(double* x, double* v, const double* r, const double* m, const env_step::Params& p, const float* heads, float u, float* logp,
               float* reward, double* margin) {
  const int action = draw(heads + 1, u, logp, margin);
  int hit = 0;
  env_step::step(x, v, r, m, p, &action, &hit);
  *reward = (float)(-hit);
  return action;
}

// The whole collection of one environment, serially (the CPU driver): rows obs (S + 1, 4N), actions, rewards, values, logp, returns
// (S,), *next_value; x, v in place.  *min_margin is lowered to the smallest margin of its draws.  -> status
PPO_FN int collect(double* x, double* v, const double* r, const double* m, const env_step::Params& p, const float* params, const Shape& s,
                   const float* u, float discount, int S, float* obs, int* actions, float* rewards, float* values, float* logp,
                   float* next_value, float* returns, double* min_margin) {
  float o[4 * env_step::kMaxObjects], a[kMaxWidth], b[kMaxWidth], heads[kHeads];
  const int W = 4 * s.N;
  for (int t = 0; t <= S; ++t) {
    for (int k = 0; k < W; ++k) o[k] = observe(x, v, k);
    forward(params, s, o, a, b, heads);
    if (!heads_finite(heads)) return kNonFinite;
    for (int k = 0; k < W; ++k) obs[(size_t)t * W + k] = o[k];
    if (t == S) break;
    double margin;
    values[t] = heads[0];
    actions[t] = act(x, v, r, m, p, heads, u[t], &logp[t], &rewards[t], &margin);
    if (margin < *min_margin) *min_margin = margin;
  }
  *next_value = heads[0];
  discounted(rewards, heads[0], discount, S, returns);
  return kOk;
}

}  // namespace ppo_policy
