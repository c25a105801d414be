// One optimiser step of the PPO update (stove_amd/rl/agents.py: PPOAgent.update -- that file is the specification) in per-row and
// per-entry pieces, as plain inline functions on top of ppo_policy.h: __host__ __device__ under hipcc (the kernel of ppo_update.hip
// calls them), unmarked under a host compiler (tests/abi/ppo_update_driver.cpp runs the same text on the CPU under sanitizers).
// Contraction is off in every body, as in ppo_policy.h.
//
// A step on mb rows: the forward of each row with its activations kept; the head of the row (log-softmax, ratio, the clipped surrogate,
// the clipped value loss, the entropy) and the derivative of the step's loss by the row's ten outputs, in float64 and rounded once; the
// backward through the layers in float32; every weight and bias gradient as ONE float32 sum over the rows in ascending order; the
// gradient norm in float64, clip_grad_norm_'s coefficient, and Adam entry by entry.  torch's tie rule for min / max (equal arguments
// share the gradient) and its clamp rule (the bounds belong to the passing range) are kept.
//
// A row of working room (row_floats(shape) floats): for each layer l its INPUT, width_in(l) floats followed by a 1.0f -- the bias of the
// layer is its weight row number width_in(l), so weights and biases are one family of entries, local = k * out + j for k <= in, and the
// image entry is offset(l) + local --, then for each layer the derivative by its OUTPUT, width_out(l) floats (the last layer's room
// first receives the ten outputs themselves).
#pragma once
#include "ppo_policy.h"

namespace ppo_update {

using ppo_policy::Shape;
using ppo_policy::kActions;
using ppo_policy::kHeads;

// status[0] of an update: all steps taken / an index of perm or an action out of range / a loss or the gradient norm of some step
// was not finite.  Either way the offending step and everything after it change nothing.
constexpr int kOk = 0, kBadIndex = 2, kNonFinite = 3;
constexpr double kBeta1 = 0.9, kBeta2 = 0.999;

struct Hyper {
  float clip, value_coef, entropy_coef, lr, eps, max_grad_norm;
  int clipped_value_loss;
};

PPO_FN int entries(const Shape& s, int l) { return (ppo_policy::width_in(s, l) + 1) * ppo_policy::width_out(s, l); }
PPO_FN int act_offset(const Shape& s, int l) {
  int o = 0;
  for (int k = 0; k < l; ++k) o += ppo_policy::width_in(s, k) + 1;
  return o;
}
PPO_FN int delta_offset(const Shape& s, int l) {
  int o = act_offset(s, ppo_policy::layers(s));
  for (int k = 0; k < l; ++k) o += ppo_policy::width_out(s, k);
  return o;
}
PPO_FN int row_floats(const Shape& s) { return delta_offset(s, ppo_policy::layers(s)); }

PPO_FN bool finite(double d) { return __builtin_isfinite(d); }

// The sums below run in chunks of kChunk terms: the operands of a chunk are all read before the first of them is used, so that the
// reads (LDS on the device, a dependent round trip each otherwise) overlap; the terms are still added one after the other in
// ascending order, each multiply and add rounded separately.
constexpr int kChunk = 8;

// ppo_policy::neuron with the row stride of the transposed weight apart from its width: the same operations in the same order
PPO_FN float neuron(const float* wT, const float* bias, const float* x, int in, size_t stride, int j, bool relu) {
  PPO_NO_CONTRACT
  float acc = bias[j];
  int k = 0;
  for (; k + kChunk <= in; k += kChunk) {
    float w[kChunk], a[kChunk];
    for (int u = 0; u < kChunk; ++u) {
      w[u] = wT[(size_t)(k + u) * stride + j];
      a[u] = x[k + u];
    }
    for (int u = 0; u < kChunk; ++u) {
      const float p = w[u] * a[u];
      acc = acc + p;
    }
  }
  for (; k < in; ++k) {
    const float p = wT[(size_t)k * stride + j] * x[k];
    acc = acc + p;
  }
  return (relu && acc < 0.0f) ? 0.0f : acc;
}

// the derivative by input k of a layer (in -> J) from the derivative by its outputs: sum_j wT[k * stride + j] * delta[j], j ascending,
// through the ReLU that produced the input (act_k, kept from the forward)
PPO_FN float back_entry(const float* wT, size_t stride, const float* delta, int J, int k, float act_k) {
  PPO_NO_CONTRACT
  const float* row = wT + (size_t)k * stride;
  float acc = 0.0f;
  int j = 0;
  for (; j + kChunk <= J; j += kChunk) {
    float w[kChunk], d[kChunk];
    for (int u = 0; u < kChunk; ++u) {
      w[u] = row[j + u];
      d[u] = delta[j + u];
    }
    for (int u = 0; u < kChunk; ++u) {
      const float p = w[u] * d[u];
      acc = acc + p;
    }
  }
  for (; j < J; ++j) {
    const float p = row[j] * delta[j];
    acc = acc + p;
  }
  return act_k > 0.0f ? acc : 0.0f;
}

// n_rows rows' terms of a gradient entry, rows ascending: g + a[r * stride] * d[r * stride], multiply and add rounded separately
PPO_FN float grad_rows(float g, const float* a, const float* d, size_t stride, int n_rows) {
  PPO_NO_CONTRACT
  int r = 0;
  for (; r + kChunk <= n_rows; r += kChunk) {
    float x[kChunk], y[kChunk];
    for (int u = 0; u < kChunk; ++u) {
      x[u] = a[(size_t)(r + u) * stride];
      y[u] = d[(size_t)(r + u) * stride];
    }
    for (int u = 0; u < kChunk; ++u) {
      const float p = x[u] * y[u];
      g = g + p;
    }
  }
  for (; r < n_rows; ++r) {
    const float p = a[(size_t)r * stride] * d[(size_t)r * stride];
    g = g + p;
  }
  return g;
}

struct RowTerms {          // the row's terms of the three means
  double value, action, entropy;
};

// The head of a row.  heads: in, the value and the nine logits; out, the derivative of the step's loss (value_loss * value_coef +
// action_loss - entropy * entropy_coef, each a mean over mb rows) by them.  work: 2 * kActions doubles of working room (the kernel
// hands over LDS, so that the lookup of the taken action is no indexed register file).
PPO_FN RowTerms head_row(float* heads, int action, float ret, float v_old, float logp_old, float adv, const Hyper& h, int mb, double* work) {
  PPO_NO_CONTRACT
  const float* logits = heads + 1;
  float top = logits[0];
  for (int a = 1; a < kActions; ++a)
    if (logits[a] > top) top = logits[a];
  double *d = work, *p = work + kActions;
  double run = 0.0;
  for (int a = 0; a < kActions; ++a) {
    const float da = logits[a] - top;
    d[a] = (double)da;
    p[a] = (double)expf(da);                             // (float32, as the logits are; the sums from here on are float64)
    run = run + p[a];
  }
  const double log_run = log(run), inv_run = 1.0 / run;
  double entropy = 0.0;
  for (int a = 0; a < kActions; ++a) {
    p[a] = p[a] * inv_run;
    d[a] = d[a] - log_run;                               // the log-probability
    entropy = entropy - p[a] * d[a];
  }
  const double inv = 1.0 / (double)mb, c = (double)h.clip, A = (double)adv;
  // ---- the surrogate: -min(ratio A, clamp(ratio, 1 - c, 1 + c) A)
  const double ratio = exp(d[action] - (double)logp_old);
  const double lo = 1.0 - c, hi = 1.0 + c;
  const bool inside = ratio >= lo && ratio <= hi;
  const double clamped = ratio < lo ? lo : ratio > hi ? hi : ratio;        // (a NaN passes)
  const double s1 = ratio * A, s2 = clamped * A;
  const double least = s2 < s1 ? s2 : s1;                                  // (a NaN in s1 passes)
  const double w1 = s1 < s2 ? 1.0 : s1 == s2 ? 0.5 : 0.0, w2 = 1.0 - w1;
  const double d_ratio = w1 * A + (inside ? w2 * A : 0.0);
  const double g_logp = -(inv * d_ratio * ratio);
  // ---- the value loss: 0.5 max((v - R)^2, (v_old + clamp(v - v_old, -c, c) - R)^2), or 0.5 (v - R)^2
  const double v = (double)heads[0], R = (double)ret, vo = (double)v_old;
  const double e1 = v - R, l1 = e1 * e1;
  double value, g_value;
  if (h.clipped_value_loss) {
    const double dv = v - vo;
    const bool within = dv >= -c && dv <= c;
    const double e2 = vo + (dv < -c ? -c : dv > c ? c : dv) - R, l2 = e2 * e2;
    const double u1 = l1 > l2 ? 1.0 : l1 == l2 ? 0.5 : 0.0, u2 = 1.0 - u1;
    value = 0.5 * (l2 > l1 ? l2 : l1);
    g_value = inv * (u1 * e1 + (within ? u2 * e2 : 0.0));
  } else {
    value = 0.5 * l1;
    g_value = inv * e1;
  }
  heads[0] = (float)((double)h.value_coef * g_value);
  const double ec = (double)h.entropy_coef * inv;
  for (int a = 0; a < kActions; ++a)
    heads[1 + a] = (float)(g_logp * ((a == action ? 1.0 : 0.0) - p[a]) + ec * p[a] * (d[a] + entropy));
  return RowTerms{value, -least, entropy};
}

// clip_grad_norm_'s factor
PPO_FN double clip_coef(double norm, float max_grad_norm) {
  const double c = (double)max_grad_norm / (norm + 1e-6);
  return c < 1.0 ? c : 1.0;
}

struct AdamStep {          // step t (from 1): lr / (1 - beta1^t) and sqrt(1 - beta2^t)
  double step_size, root_bias2;
};
PPO_FN AdamStep adam_step(int t, float lr) {
  return AdamStep{(double)lr / (1.0 - pow(kBeta1, (double)t)), sqrt(1.0 - pow(kBeta2, (double)t))};
}

// torch.optim.Adam on one entry (no weight decay, eps outside the root): the clipped gradient rounded to float32 as clip_grad_norm_
// leaves it, the moments and the parameter each computed in float64 from their float32 values and rounded once.  -> the new parameter
PPO_FN float adam_entry(float param, float grad, float coef, float* m, float* v, const AdamStep& a, float eps) {
  PPO_NO_CONTRACT
  const double g = (double)(grad * coef);
  const double m1 = (double)*m + (g - (double)*m) * (1.0 - kBeta1);
  const double v1 = (double)*v * kBeta2 + (1.0 - kBeta2) * g * g;
  *m = (float)m1;
  *v = (float)v1;
  const double denom = sqrt((double)*v) / a.root_bias2 + (double)eps;
  return (float)((double)param - a.step_size * ((double)*m / denom));
}

// ---------------------------------------------------------------------------------------------- the whole update, serially (the CPU driver)
// the forward of a row with its activations kept: row as described at the top, the ten outputs in the last layer's derivative room
PPO_FN void forward_keep(const float* params, const Shape& s, const float* obs, float* row) {
  const int L = ppo_policy::layers(s), W = ppo_policy::width_in(s, 0);
  for (int k = 0; k < W; ++k) row[k] = obs[k];
  row[W] = 1.0f;
  for (int l = 0; l < L; ++l) {
    const int K = ppo_policy::width_in(s, l), J = ppo_policy::width_out(s, l);
    const float* wT = params + ppo_policy::offset(s, l);
    const float* in = row + act_offset(s, l);
    float* out = row + (l == L - 1 ? delta_offset(s, l) : act_offset(s, l + 1));
    for (int j = 0; j < J; ++j) out[j] = neuron(wT, wT + (size_t)K * J, in, K, (size_t)J, j, l != L - 1);
    if (l != L - 1) out[J] = 1.0f;
  }
}

// the backward of a row from the derivative by its ten outputs (in the last layer's room) down to the first layer's outputs
PPO_FN void backward_row(const float* params, const Shape& s, float* row) {
  for (int l = ppo_policy::layers(s) - 1; l >= 1; --l) {
    const int K = ppo_policy::width_in(s, l), J = ppo_policy::width_out(s, l);
    const float* wT = params + ppo_policy::offset(s, l);
    const float* act = row + act_offset(s, l);
    for (int k = 0; k < K; ++k) row[delta_offset(s, l - 1) + k] = back_entry(wT, (size_t)J, row + delta_offset(s, l), J, k, act[k]);
  }
}

// Up to max_steps of the E * M optimiser steps on n rows.  params, m, v: param_floats(s) floats in/out; *step in/out; obs (n, 4N),
// actions, returns, values, logp, adv (n,); perm (E, n); losses (E * M, 3) value / action / entropy, gnorm (E * M,): written for the
// steps taken; grad: param_floats(s) floats and row: row_floats(s) floats of working room.  -> status; *done = the steps taken.
PPO_FN int update(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns, const float* values,
                  const float* logp, const float* adv, const int* perm, float* losses, float* gnorm, int n, int E, int M, int max_steps,
                  const Shape& s, const Hyper& h, float* grad, float* row, int* done) {
  const int L = ppo_policy::layers(s), W = 4 * s.N, mb = n / M;
  const size_t P = ppo_policy::param_floats(s);
  double work[2 * kActions];
  *done = 0;
  for (int at = 0; at < max_steps; ++at) {
    const int* rows = perm + (size_t)(at / M) * n + (size_t)(at % M) * mb;
    for (int r = 0; r < mb; ++r)
      if (rows[r] < 0 || rows[r] >= n || actions[rows[r]] < 0 || actions[rows[r]] >= kActions) return kBadIndex;
    for (size_t e = 0; e < P; ++e) grad[e] = 0.0f;
    double value = 0.0, action = 0.0, entropy = 0.0;
    for (int r = 0; r < mb; ++r) {
      const int i = rows[r];
      forward_keep(params, s, obs + (size_t)i * W, row);
      const RowTerms t = head_row(row + delta_offset(s, L - 1), actions[i], returns[i], values[i], logp[i], adv[i], h, mb, work);
      value = value + t.value;
      action = action + t.action;
      entropy = entropy + t.entropy;
      backward_row(params, s, row);
      for (int l = 0; l < L; ++l) {
        const int K = ppo_policy::width_in(s, l), J = ppo_policy::width_out(s, l);
        float* g = grad + ppo_policy::offset(s, l);
        const float *a = row + act_offset(s, l), *d = row + delta_offset(s, l);
        for (int k = 0; k <= K; ++k)
          for (int j = 0; j < J; ++j) g[(size_t)k * J + j] = grad_rows(g[(size_t)k * J + j], a + k, d + j, 0, 1);
      }
    }
    value = value / (double)mb;
    action = action / (double)mb;
    entropy = entropy / (double)mb;
    double sq = 0.0;
    for (size_t e = 0; e < P; ++e) sq = sq + (double)grad[e] * (double)grad[e];
    const double norm = sqrt(sq);
    if (!finite(value) || !finite(action) || !finite(entropy) || !finite(norm)) return kNonFinite;
    const float coef = (float)clip_coef(norm, h.max_grad_norm);
    const AdamStep a = adam_step(*step + 1, h.lr);
    for (size_t e = 0; e < P; ++e) params[e] = adam_entry(params[e], grad[e], coef, &m[e], &v[e], a, h.eps);
    *step = *step + 1;
    losses[(size_t)at * 3] = (float)value;
    losses[(size_t)at * 3 + 1] = (float)action;
    losses[(size_t)at * 3 + 2] = (float)entropy;
    gnorm[at] = (float)norm;
    *done = at + 1;
  }
  return kOk;
}

}  // namespace ppo_update
