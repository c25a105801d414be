// The model-based PPO arm's collection, one launch per batch of imagined trajectories (stove_ppo_collect_model, capi.hip; reference
// runners.py: run_pretrained_batch).  The chain of one trajectory is serial -- observation of the model state, the policy, the draw, the
// action's embedding, one step of the action-conditioned dynamics -- and the composed loop pays about ten small launches for each of
// its S links.  Here one workgroup of kSmWaves waves owns one trajectory for all S steps, laid out as rollout_fwd_small_k
// (gnn_small.hip) lays out a sequence: a wave per node row (a half-wave per row for five and six objects), the state in the lanes from
// step to step, sm_step as it is.  Between two steps:
//   observation   lanes l < 4 of a row hold x, y, vx, vy: ppo_policy::observe_model into the trajectory's LDS row (the row obs[b][t] gets)
//   policy        ppo_policy::neuron, neuron j of a layer on thread j of the workgroup (its sum whole and in order on that thread), the
//                 activations from layer to layer through LDS, one workgroup barrier per layer; the image staged in LDS when it fits
//                 beside the dynamics' weights, else read from global memory through the cache
//   draw          ppo_policy::draw on thread 0; the action reaches the rows through LDS
//   extra inputs  lanes 16 .. 19 of row r: column `action` of the embedding Linear plus its bias in plan_prep_k's order of operations
//                 (the bits of stove_small_linear on a one-hot row); lanes 20 ..: the trajectory's appearance row, loaded once
//   reward        plan_finish_k's reward-head arithmetic on the step's `pred` rows (kept in LDS).  It does not feed back: wave 3 runs
//                 the head of step t - 1 while wave 0 walks the 128 inputs of the policy's second layer of step t, off the chain.
// One trajectory per workgroup: whether it goes on (a value or a logit not finite ends it) is the same for every wave, which all
// leave the loop at the same place, so every wave meets every barrier.  Plain vector stores only, no atomics; rewards are written
// and read back (the returns) by the same thread.  One object goes through a kernel of its own on gnn_forward (at the end of the file).
// This file is the cl = 32 arm.  Models of state-code length 16 and 64 are served by ppo_model_cl.hip (stove_ppo_collect_model_cl): the
// same chain around gnn_cl.hip's cl_forward<CL>, one kernel per width for every object count.
// The reward head's layout and dots (RhCl, rh_dot_t, rh_dot_rows: reward_head.h), the constants and the kernels' parameter list
// (ppo_model_step.h) are shared; the step between two dynamics steps and the reward head's forward are this file's own text, held bit
// for bit to reward_head.h's rh_forward by the tests: written on shared helpers the launch measured 1 to 1.5 % slower and the cause was
// not found.
#include "common.h"
#include "ppo_model_step.h"

namespace stove {

constexpr int kPmRhV = 104;                                        // the reward head's vectors (plan_finish_k's V), padded
// the launch's LDS beyond the dynamics' (SmShape::kLdsFloats): policy rows, the step's pred rows, the embedding, the reward head's tables
constexpr int kPmFloats = kPmObsFloats + 2 * ppo_policy::kMaxWidth + kPmHeadFloats + env_step::kMaxObjects * 32 +
                          kPmEmbRows * ppo_policy::kActions + kPmEmbRows + 1024 + 1024 + 512 + 128 + kPmRhV + 32 + 4;
// room for sm_step's and sm_dotw's own arrays (sbuf, sdx, an xb per form of the dot: 3584 bytes in the kernel for six objects), which
// the compiler places beside the dynamic part
constexpr size_t kPmStaticBytes = 4096;
static_assert(ppo_policy::kMaxWidth <= 64 * kSmWaves, "a layer's neurons have a thread each");
static_assert(kPmFloats % 4 == 0, "the image behind it stays 16-byte aligned");

struct PmLds {
  float *o, *a, *b, *heads, *pred, *embw, *embb, *Wt0a, *Wt0b, *Wt1a, *Wt1b, *V, *xs, *img;
  int* act;
};
__device__ __forceinline__ PmLds pm_carve(float* base) {
  PmLds M;
  M.o = base;
  M.a = M.o + kPmObsFloats;
  M.b = M.a + ppo_policy::kMaxWidth;
  M.heads = M.b + ppo_policy::kMaxWidth;
  M.pred = M.heads + kPmHeadFloats;                      // [N][32] dynamic_pred of the step just taken
  M.embw = M.pred + env_step::kMaxObjects * 32;          // [4N][9]
  M.embb = M.embw + kPmEmbRows * ppo_policy::kActions;   // [4N]
  M.Wt0a = M.embb + kPmEmbRows;
  M.Wt0b = M.Wt0a + 1024;
  M.Wt1a = M.Wt0b + 1024;
  M.Wt1b = M.Wt1a + 512;
  M.V = M.Wt1b + 128;
  M.xs = M.V + kPmRhV;
  M.act = reinterpret_cast<int*>(M.xs + 32);
  M.img = M.xs + 32 + 4;
  return M;
}

template <int NMX>
constexpr size_t pm_fixed_bytes() { return (size_t)(SmShape<NMX>::kLdsFloats + kPmFloats) * sizeof(float); }
static_assert(pm_fixed_bytes<4>() == 113328 && pm_fixed_bytes<6>() == 118048, "the launch's LDS is part of what `staged` decides");
// the image is staged when it fits beside everything else
template <int NMX>
inline bool pm_staged(size_t n_params) { return pm_fixed_bytes<NMX>() + kPmStaticBytes + n_params * sizeof(float) <= kPmLdsLimit; }
template <int NMX>
inline size_t pm_lds_bytes(size_t n_params) { return pm_fixed_bytes<NMX>() + (pm_staged<NMX>(n_params) ? n_params * sizeof(float) : 0); }

// the reward head on the N rows of M.pred, by one wave: plan_finish_k's arithmetic (reward_head_fwd_k's bits), nothing saved
__device__ __forceinline__ float pm_reward(const PmLds& M, int N, int lane) {
  const int l = lane & 31;
  const bool act = lane < 32;
  float* x = M.xs;
  const float *b0a = M.V, *b0b = M.V + 32, *b1a = M.V + 64, *b1b = M.V + 80, *w1c = M.V + 88, *b1c = M.V + 96;
  float h32 = 0.0f;
  for (int o = 0; o < N; ++o) {
    if (act) x[l] = M.pred[o * 32 + l];
    float h = b0a[l] + rh_dot_t<32, 32>(M.Wt0a, x, l);
    h = fmaxf(h, 0.0f);
    if (act) x[l] = h;
    h32 += b0b[l] + rh_dot_t<32, 32>(M.Wt0b, x, l);
  }
  if (act) x[l] = h32;
  const float a1 = fmaxf(b1a[l & 15] + rh_dot_t<32, 16>(M.Wt1a, x, l), 0.0f);
  if (lane < 16) x[l] = a1;
  const float a2 = fmaxf(b1b[l & 7] + rh_dot_t<16, 8>(M.Wt1b, x, l), 0.0f);
  if (lane < 8) x[l] = a2;
  float z = b1c[0];
#pragma unroll
  for (int k = 0; k < 8; ++k) z = fmaf(w1c[k], x[k], z);
  return 1.0f / (1.0f + expf(-z));
}

// grid B, block 64 kSmWaves, dynamic LDS pm_lds_bytes<NMX>.  z0 (B, N, 18); app (B, N, app_dim) or null; params the policy's image;
// emb_w (4N, 9), emb_b (4N); P the dynamics' image; rh the reward head's; u (B, S); z_pred (B, S, N, 18); pred (B, S, N, 32) or null;
// obs (B, S + 1, 4N); actions, rewards, values, logp, returns (B, S); next_value, status (B,).
template <int NMX, bool ELU, int NT>
__global__ __launch_bounds__(64 * kSmWaves) void ppo_collect_model_k(PM_KERNEL_PARAMS) {
  constexpr int RP = SmShape<NMX>::RP, ET = SmShape<NMX>::ET;
  static_assert(NT <= NMX, "object count beyond what the kernel is built for");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const SmLds L = sm_carve<NMX>(lds);
  const PmLds M = pm_carve(lds + SmShape<NMX>::kLdsFloats);
  const int b = blockIdx.x, tid = (int)threadIdx.x;
  const int wv = wave_id(), lane = lane_id(), l = lane & 31;
  elu = ELU ? 1 : 0;      // compile-time activation, as in rollout_fwd_small_k
  if (NT > 0) N = NT;
  const int sin_dim = 20 + app_dim;
  SmCfg cf{N, sin_dim, lim_enc, elu};
  cf.stamps = nullptr;
  SmEdgeLane el[ET];
#pragma unroll
  for (int t = 0; t < ET; ++t) el[t] = sm_edge_lane(N, 0, t);
  sm_setup(L, P);
  // the reward head's tables, transposed as plan_finish_k keeps them
  for (int i = tid; i < 1024; i += blockDim.x) {
    const int o = i >> 5, k = i & 31;                    // W (out o, in k) -> Wt[k][o]
    M.Wt0a[k * 32 + o] = rh[RhCl<32>::W0A + i];
    M.Wt0b[k * 32 + o] = rh[RhCl<32>::W0B + i];
  }
  for (int i = tid; i < 512; i += blockDim.x) M.Wt1a[(i & 31) * 16 + (i >> 5)] = rh[RhCl<32>::W1A + i];
  for (int i = tid; i < 128; i += blockDim.x) M.Wt1b[(i & 15) * 8 + (i >> 4)] = rh[RhCl<32>::W1B + i];
  for (int i = tid; i < 32; i += blockDim.x) { M.V[i] = rh[RhCl<32>::B0A + i]; M.V[32 + i] = rh[RhCl<32>::B0B + i]; }
  for (int i = tid; i < 16; i += blockDim.x) M.V[64 + i] = rh[RhCl<32>::B1A + i];
  for (int i = tid; i < 8; i += blockDim.x) { M.V[80 + i] = rh[RhCl<32>::B1B + i]; M.V[88 + i] = rh[RhCl<32>::W1C + i]; }
  if (tid == 0) M.V[96] = rh[RhCl<32>::B1C];
  const int W = 4 * N, Ly = ppo_policy::layers(sh);
  for (int i = tid; i < W * ppo_policy::kActions; i += blockDim.x) M.embw[i] = emb_w[i];
  if (tid < W) M.embb[tid] = emb_b[tid];
  const float* wts = params;
  if (staged) {
    for (int i = tid; i < n_params; i += blockDim.x) M.img[i] = params[i];
    wts = M.img;
  }
  // the lane's node row r: lane l < 16 of its half holds z[r][2 + l], lanes 16 .. the extra inputs
  float sinv = 0.0f, scale = 0.0f, appv = 0.0f;
  const int r = RP == 2 ? wv + 4 * (lane >> 5) : wv;
  const bool row = r < N;
  const bool own = RP == 2 ? row : (lane < 32 && row);
  if (row) {
    if (l < 16) sinv = z0[((size_t)b * N + r) * 18 + 2 + l];
    else if (l < 18) scale = z0[((size_t)b * N + r) * 18 + (l - 16)];       // sx, sy stay constant
    if (l >= 20 && l < sin_dim) appv = app[((size_t)b * N + r) * app_dim + (l - 20)];
  }
  __syncthreads();
  SmChainW cw;
  sm_chain_wbuild(L, cw);
  bool going = true;
  for (int t = 0; t <= S; ++t) {
    if (own && l < 4) M.o[4 * r + l] = ppo_policy::observe_model(sinv, l, hw);
    __syncthreads();
    const float* in = M.o;
    for (int ly = 0; ly < Ly; ++ly) {
      const int K = ppo_policy::width_in(sh, ly), J = ppo_policy::width_out(sh, ly);
      const float* wT = wts + ppo_policy::offset(sh, ly);
      float* out = ly == Ly - 1 ? M.heads : (ly & 1) ? M.b : M.a;
      if (tid < J) out[tid] = ppo_policy::neuron(wT, wT + (size_t)K * J, in, K, J, tid, ly != Ly - 1);
      if (ly == 1 && wv == 3 && t > 0) {          // the reward of the step before, beside the widest layer's 32 neurons on wave 0
        const float rw = pm_reward(M, N, lane);
        if (lane == 0) rewards[(size_t)b * S + t - 1] = rw - 1.0f;
      }
      __syncthreads();
      in = out;
    }
    if (!ppo_policy::heads_finite(M.heads)) {      // (every thread reads the same ten words)
      going = false;
      break;
    }
    if (tid < W) obs[((size_t)b * (S + 1) + t) * W + tid] = M.o[tid];
    if (t == S) break;
    if (tid == 0) {
      const size_t at = (size_t)b * S + t;
      float lp;
      double margin;
      values[at] = M.heads[0];
      const int action = ppo_policy::draw(M.heads + 1, u[at], &lp, &margin);
      actions[at] = action;
      logp[at] = lp;
      M.act[0] = action;
    }
    __syncthreads();
    if (row && l >= 16) {
      if (l < 20) {       // the embedding Linear on a one-hot row, in small_linear_k's order of operations (the same bits)
        const int action = M.act[0], o = r * 4 + (l - 16);
        float v = M.embb[o];
        for (int k = 0; k < ppo_policy::kActions; ++k) v = fmaf(k == action ? 1.0f : 0.0f, M.embw[o * ppo_policy::kActions + k], v);
        sinv = v;
      } else {
        sinv = appv;
      }
    }
    const size_t o = ((size_t)b * S + t) * N + r;
    SmAct a{};
    float res = 0.0f, prd = 0.0f;
    SmNodeOut no{};
    sm_step<false, NMX>(L, cf, sinv, a, res, prd, el, cw, no);
    if (wv < N) {
      float zv = 0.0f;
      if (l < 16) {
        zv = 2.0f * sigmoidf_(res) - 1.0f + (l < 2 ? sinv : 0.0f);
        if (own) z_pred[o * 18 + 2 + l] = zv;
      } else if (l < 18 && own) {
        z_pred[o * 18 + (l - 16)] = scale;
      }
      if (own) {
        if (pred != nullptr) pred[o * 32 + l] = prd;
        M.pred[r * 32 + l] = prd;
      }
      sinv = zv;
    }
  }
  if (going && wv == 3 && lane == 0) {          // (the thread that wrote the rewards)
    next_value[b] = M.heads[0];
    ppo_policy::discounted(rewards + (size_t)b * S, M.heads[0], discount, S, returns + (size_t)b * S);
  }
  if (tid == 0) status[b] = going ? ppo_policy::kOk : ppo_policy::kNonFinite;
}

// =================================================================================================
// one object: the small-graph kernels start at two (stove_rollout_fwd sends N = 1 to rollout_fwd_k of gnn.hip), so a trajectory of one
// object steps through gnn_forward, with G = 1, to the same bits.  No edges and a 4-wide observation: nothing here is tuned.  The LDS
// of gnn_forward leaves no room for the reward head's tables or the policy's image, which are read from global memory.
// =================================================================================================
constexpr int kPm1Floats = kPmObsFloats + 2 * ppo_policy::kMaxWidth + kPmHeadFloats + 32 + 4 * ppo_policy::kActions + 4 + 4;
constexpr size_t kPm1LdsBytes = (size_t)(kGnnLdsFloats + kPm1Floats) * sizeof(float);
static_assert(kPm1LdsBytes == 155184, "the launch's LDS");
static_assert(kPm1LdsBytes + 1024 <= kPmLdsLimit, "gnn_forward's LDS and the policy's rows fit one CU");

// grid B, block 256, dynamic LDS kPm1LdsBytes; the arguments of ppo_collect_model_k with N = 1
__global__ __launch_bounds__(256) void ppo_collect_model_one_k(PM_KERNEL_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GnnLds L = carve(lds);
  float* o = lds + kGnnLdsFloats;
  float *a = o + kPmObsFloats, *bb = a + ppo_policy::kMaxWidth, *heads = bb + ppo_policy::kMaxWidth, *xs = heads + kPmHeadFloats;
  float *embw = xs + 32, *embb = embw + 4 * ppo_policy::kActions;
  int* act = reinterpret_cast<int*>(embb + 4);
  const int b = blockIdx.x, tid = (int)threadIdx.x, wv = wave_id(), lane = lane_id();
  const int sin_dim = 20 + app_dim, Ly = ppo_policy::layers(sh);
  const GnnShape gs = make_shape(1, 1, b, B, sin_dim, lim_enc, elu);
  lds_zero(lds, kGnnLdsFloats);
  WG_SYNC();
  gnn_setup(L, gs, P + 2 * W_END);
  WG_SYNC();
  float* Z = L.X;          // [20] the current state
  if (tid < 18) Z[tid] = z0[(size_t)b * 18 + tid];
  if (tid < 4 * ppo_policy::kActions) embw[tid] = emb_w[tid];
  if (tid < 4) embb[tid] = emb_b[tid];
  const FwdW fw = gnn_fwdw_load(P);
  __syncthreads();
  bool going = true;
  for (int t = 0; t <= S; ++t) {
    if (tid < 4) o[tid] = ppo_policy::observe_model(Z[2 + tid], tid, hw);
    __syncthreads();
    const float* in = o;
    for (int ly = 0; ly < Ly; ++ly) {
      const int K = ppo_policy::width_in(sh, ly), J = ppo_policy::width_out(sh, ly);
      const float* wT = params + ppo_policy::offset(sh, ly);
      float* out = ly == Ly - 1 ? heads : (ly & 1) ? bb : a;
      if (tid < J) out[tid] = ppo_policy::neuron(wT, wT + (size_t)K * J, in, K, J, tid, ly != Ly - 1);
      if (ly == 1 && wv == 3 && t > 0) {          // the reward of the step before: plan_finish_k's arithmetic on L.PRED's row
        const int l = lane & 31;
        const bool lo = lane < 32;
        if (lo) xs[l] = L.PRED[l];
        float h = rh[RhCl<32>::B0A + l] + rh_dot_rows<32, 32>(rh + RhCl<32>::W0A, xs, l);
        h = fmaxf(h, 0.0f);
        if (lo) xs[l] = h;
        float h32 = 0.0f;
        h32 += rh[RhCl<32>::B0B + l] + rh_dot_rows<32, 32>(rh + RhCl<32>::W0B, xs, l);
        if (lo) xs[l] = h32;
        const float a1 = fmaxf(rh[RhCl<32>::B1A + (l & 15)] + rh_dot_rows<32, 16>(rh + RhCl<32>::W1A, xs, l), 0.0f);
        if (lane < 16) xs[l] = a1;
        const float a2 = fmaxf(rh[RhCl<32>::B1B + (l & 7)] + rh_dot_rows<16, 8>(rh + RhCl<32>::W1B, xs, l), 0.0f);
        if (lane < 8) xs[l] = a2;
        float z = rh[RhCl<32>::B1C];
#pragma unroll
        for (int k = 0; k < 8; ++k) z = fmaf(rh[RhCl<32>::W1C + k], xs[k], z);
        const float rw = 1.0f / (1.0f + expf(-z));
        if (lane == 0) rewards[(size_t)b * S + t - 1] = rw - 1.0f;
      }
      __syncthreads();
      in = out;
    }
    if (!ppo_policy::heads_finite(heads)) {
      going = false;
      break;
    }
    if (tid < 4) obs[((size_t)b * (S + 1) + t) * 4 + tid] = o[tid];
    if (t == S) break;
    if (tid == 0) {
      const size_t at = (size_t)b * S + t;
      float lp;
      double margin;
      values[at] = heads[0];
      const int action = ppo_policy::draw(heads + 1, u[at], &lp, &margin);
      actions[at] = action;
      logp[at] = lp;
      act[0] = action;
    }
    __syncthreads();
    if (tid < sin_dim) {
      float v;
      if (tid < 16) {
        v = Z[2 + tid];
      } else if (tid < 20) {
        const int action = act[0], e = tid - 16;
        v = embb[e];
        for (int k = 0; k < ppo_policy::kActions; ++k) v = fmaf(k == action ? 1.0f : 0.0f, embw[e * ppo_policy::kActions + k], v);
      } else {
        v = app[(size_t)b * app_dim + (tid - 20)];
      }
      L.SIN[tid] = v;
    }
    WG_SYNC();
    gnn_forward(L, gs, P, fw);
    const size_t at = (size_t)b * S + t;
    if (tid < 18) {
      float v;
      if (tid < 2) {
        v = Z[tid];                                       // scale stays constant
      } else {
        const int d = tid - 2;
        v = 2.0f * sigmoidf_(L.RES[d]) - 1.0f + (d < 2 ? L.SIN[d] : 0.0f);
      }
      z_pred[at * 18 + tid] = v;
      Z[tid] = v;
    }
    if (pred != nullptr && tid < 32) pred[at * 32 + tid] = L.PRED[tid];
    __syncthreads();
  }
  if (going && wv == 3 && lane == 0) {
    next_value[b] = heads[0];
    ppo_policy::discounted(rewards + (size_t)b * S, heads[0], discount, S, returns + (size_t)b * S);
  }
  if (tid == 0) status[b] = going ? ppo_policy::kOk : ppo_policy::kNonFinite;
}

}  // namespace stove
