// What the kernels of the model-based PPO arm's collection share (ppo_collect_model_k and ppo_collect_model_one_k of ppo_model.hip,
// ppo_collect_model_cl_k<CL> of ppo_model_cl.hip) with each other, with their launch (capi.hip) and with planning (plan.hip): the
// argument block, the kernels' parameter list, the sizes of the policy's rows in LDS, and the embedding of one action.  The step
// between two dynamics steps is each kernel's own text: written once on helpers here it cost 1 to 5 % of a launch (measured; the
// policy block accounted for most of it, the cause was not found), and speed is a condition.
#pragma once
#include "common.h"
#include "ppo_policy.h"

namespace stove {

// z0 (B, N, cl/2 + 2); app (B, N, app_dim) or null; params the policy's image of n_params floats, `staged`: copied to LDS; emb_w (4N, 9),
// emb_b (4N); P the dynamics' image; rh the reward head's block; u (B, S); z_pred (B, S, N, cl/2 + 2); pred (B, S, N, cl) or null;
// obs (B, S + 1, 4N); actions, rewards, values, logp, returns (B, S); next_value, status (B,).
struct PmArgs {
  const float *z0, *app, *params, *emb_w, *emb_b, *P, *rh, *u;
  float *z_pred, *pred, *obs;
  int* actions;
  float *rewards, *values, *logp, *next_value, *returns;
  int* status;
  ppo_policy::Shape sh;
  int B, S, N, app_dim, lim_enc, elu;
  float hw, discount;
  int n_params, staged;
};

// The kernels take the block as flat __restrict__ parameters (PM_KERNEL_PARAMS), the launch unpacks it (PM_LAUNCH_ARGS).  Handed over
// as one by-value struct the whole block is loaded at kernel entry and held in scalar registers across the step: 41 more
// scalar-register spills in ppo_collect_model_k and 3 to 4 % on a launch, measured.  Beyond the two C entry points the list is
// spelled here only.
#define PM_KERNEL_PARAMS                                                                                                                        \
  const float *__restrict__ z0, const float *__restrict__ app, const float *__restrict__ params, const float *__restrict__ emb_w,              \
      const float *__restrict__ emb_b, const float *__restrict__ P, const float *__restrict__ rh, const float *__restrict__ u,                 \
      float *__restrict__ z_pred, float *__restrict__ pred, float *__restrict__ obs, int *__restrict__ actions, float *rewards,                \
      float *__restrict__ values, float *__restrict__ logp, float *__restrict__ next_value, float *__restrict__ returns,                       \
      int *__restrict__ status, ppo_policy::Shape sh, int B, int S, int N, int app_dim, int lim_enc, int elu, float hw, float discount,       \
      int n_params, int staged
#define PM_LAUNCH_ARGS(A)                                                                                                                       \
  (A).z0, (A).app, (A).params, (A).emb_w, (A).emb_b, (A).P, (A).rh, (A).u, (A).z_pred, (A).pred, (A).obs, (A).actions, (A).rewards, (A).values, \
      (A).logp, (A).next_value, (A).returns, (A).status, (A).sh, (A).B, (A).S, (A).N, (A).app_dim, (A).lim_enc, (A).elu, (A).hw, (A).discount,  \
      (A).n_params, (A).staged

// the policy's rows in LDS (observation, two hidden buffers of kMaxWidth, the ten outputs) and the embedding's rows
constexpr int kPmObsFloats = 32, kPmHeadFloats = 16, kPmEmbRows = 4 * env_step::kMaxObjects;
constexpr size_t kPmLdsLimit = 160 * 1024;                          // one CU's LDS, all of which one workgroup may take
static_assert(4 * env_step::kMaxObjects <= kPmObsFloats && ppo_policy::kHeads <= kPmHeadFloats, "the rows hold the widest case");

// element o of the action's embedding (o = 4 row + e): the Linear on a one-hot row, in small_linear_k's order of operations (the same bits)
__device__ __forceinline__ float pm_embed(const float* embw, const float* embb, int o, int action, int n_actions = ppo_policy::kActions) {
  float v = embb[o];
  for (int k = 0; k < n_actions; ++k) v = fmaf(k == action ? 1.0f : 0.0f, embw[o * n_actions + k], v);
  return v;
}

}  // namespace stove
