// The reward head of the action-conditioned model (reference dynamics.py:254-263, 62-70) at the state-code lengths CL = 16, 32, 64:
//     reward = sigmoid( head1( sum_objects head0(dynamic_pred) ) ),
//     head0 = Linear(CL, CL) - ReLU - Linear(CL, CL),   head1 = Linear(CL, CL/2) - ReLU - Linear(CL/2, CL/4) - ReLU - Linear(CL/4, 1)
// What its kernels share: RhCl<CL>, the one description of the parameter block (the ten tensors in module order, nn.Linear layout,
// weight (out, in) row-major), and a layer's sum in its two forms, against a table transposed in LDS (rh_dot_t) and against the
// block's own rows in global memory (rh_dot_rows): the same terms in the same order on the same two chains.
// The forward itself -- bias + dot per layer, the objects summed in order from 0.0f, head1.4 as one fmaf chain, 1 / (1 + expf(-z)) --
// is written out in each kernel that runs it (reward_head_fwd_k, plan_finish_k<CL>, ppo_collect_model_k, ppo_collect_model_one_k,
// ppo_collect_model_cl_k<CL>) and the copies are held to one another and to a recorded build bit for bit
// (tests/test_gpu_control_bits.py, the ties in tests/test_gpu_ppo_model*.py).  Written once as a function over table views it cost
// speed in every caller that is timed: about 1 % in plan_finish_k<16|32>, 1 to 5 % of a launch of the collections; the causes found
// (tables in one LDS array keep the compiler from hoisting their loads over the scratch stores; a by-value argument block is held in
// scalar registers) did not account for all of it.
#pragma once
#include "common.h"

namespace stove {

constexpr int kRhWaves = 4;          // waves (items in flight) per workgroup of reward_head_fwd_k / reward_head_bwd_k / plan_finish_k

// 2 CL^2 + 2 CL + CL^2/2 + CL/2 + CL^2/8 + CL/4 + CL/4 + 1 floats:
//   [W0a CL*CL | b0a CL | W0b CL*CL | b0b CL | W1a H1*CL | b1a H1 | W1b H2*H1 | b1b H2 | W1c H2 | b1c 1]
template <int CL>
struct RhCl {
  static_assert(CL == 16 || CL == 32 || CL == 64, "one wave holds a CL-wide vector; the dots take K in fours");
  static constexpr int H1 = CL / 2, H2 = CL / 4;
  static constexpr int W0A = 0, B0A = W0A + CL * CL, W0B = B0A + CL, B0B = W0B + CL * CL, W1A = B0B + CL, B1A = W1A + H1 * CL, W1B = B1A + H1,
                       B1B = W1B + H2 * H1, W1C = B1B + H2, B1C = W1C + H2, kParams = B1C + 1;
};
static_assert(RhCl<16>::kParams == 721 && RhCl<32>::kParams == 2785 && RhCl<64>::kParams == 10945, "reward-head block sizes");
constexpr int kRhParams = RhCl<32>::kParams;

// y[l] = sum_k Wt[k * OUT + l] x[k]  (lane l < OUT), x broadcast from the wave's LDS scratch
template <int K, int OUT>
__device__ __forceinline__ float rh_dot_t(const float* Wt, const float* xs, int l) {
  float a = 0.0f, b = 0.0f;
#pragma unroll
  for (int k = 0; k < K; k += 4) {
    const float4 x4 = *reinterpret_cast<const float4*>(xs + k);
    const int ll = l < OUT ? l : 0;
    a = fmaf(Wt[(k + 0) * OUT + ll], x4.x, a);
    b = fmaf(Wt[(k + 1) * OUT + ll], x4.y, b);
    a = fmaf(Wt[(k + 2) * OUT + ll], x4.z, a);
    b = fmaf(Wt[(k + 3) * OUT + ll], x4.w, b);
  }
  return a + b;
}
// rh_dot_t's sum (the same terms in the same order on the same two chains) on a weight (OUT, K) row-major as the parameter block holds it
template <int K, int OUT>
__device__ __forceinline__ float rh_dot_rows(const float* __restrict__ Wm, const float* xs, int l) {
  float a = 0.0f, b = 0.0f;
  const int ll = l < OUT ? l : 0;
#pragma unroll
  for (int k = 0; k < K; k += 4) {
    const float4 x4 = *reinterpret_cast<const float4*>(xs + k);
    a = fmaf(Wm[ll * K + k + 0], x4.x, a);
    b = fmaf(Wm[ll * K + k + 1], x4.y, b);
    a = fmaf(Wm[ll * K + k + 2], x4.z, a);
    b = fmaf(Wm[ll * K + k + 3], x4.w, b);
  }
  return a + b;
}

}  // namespace stove
