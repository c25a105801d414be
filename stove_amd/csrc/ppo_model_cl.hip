// The model-based PPO arm's collection on models of state-code length cl = 16 and 64 (stove_ppo_collect_model_cl, capi.hip): what
// ppo_collect_model_k (ppo_model.hip) does at cl = 32, on the width-generic step of gnn_cl.hip.  One workgroup of 256 threads owns one
// trajectory for all S steps, laid out as gnn_cl_rollout_k<CL> lays out a sequence with G = 1 -- cl_carve, cl_setup and cl_forward as
// they are, the state row in L.X (N <= 6 rows of cl/2 + 2 floats); one object goes the same way, no second kernel.  Between two steps:
//   observation   ppo_policy::observe_model on columns 2 .. 5 of the state rows, into the trajectory's LDS row (the row obs[b][t] gets)
//   policy        ppo_policy::neuron, neuron j of a layer on thread j, one workgroup barrier per layer; the image staged in LDS when it
//                 fits behind everything else (`staged`), else read from global memory through the cache
//   draw          ppo_policy::draw on thread 0; the action reaches the rows through LDS
//   extra inputs  columns cl/2 .. cl/2 + 3 of row r of L.SIN: column `action` of the embedding Linear plus its bias in plan_prep_k's order
//                 of operations (the bits of stove_small_linear on a one-hot row); behind them the trajectory's appearance row
//   state         after cl_forward exactly what gnn_cl_rollout_k writes: 2 sigmoid(res) - 1, plus the previous position in the first
//                 two columns; the scale columns copied
//   reward        plan_finish_k<CL>'s arithmetic on the step's L.PRED rows, minus 1.0f, by wave 3 behind the step (the serial form: reading
//                 the head's rows a float4 at a time instead changed the launch's time by nothing, DESIGN 4i -- it is not what a step waits for).
// LDS: GC<64>::kLdsFloats is 147 776 of a CU's 163 840 bytes, so at cl = 64 the reward head's transposed tables (42 KiB) do not fit and
// its weights are read from global memory in the parameter block's own layout (rh_dot_rows: rh_dot_t's terms in rh_dot_t's order on its
// two chains); at cl = 16 (76 KB) the tables are staged as plan_finish_k keeps them.
// One trajectory per workgroup: whether it goes on is the same for every thread, so every thread meets every barrier.  Plain vector
// stores only, no atomics; rewards are written and read back (the returns) by the same thread.
// The reward head's layout and dots (RhCl, rh_dot_t, rh_dot_rows: reward_head.h), the constants and the kernel's parameter list
// (ppo_model_step.h) are shared; the step between two dynamics steps and the reward head's forward (pc_reward) are this file's own
// text, held bit for bit to reward_head.h's rh_forward by the tests: written on shared helpers a launch measured 4 to 5 % slower at
// both widths and the cause was not found (the policy block accounted for all of it at cl = 64 and for part of it at cl = 16).
// Included from capi.hip after gnn_cl.hip, whose GC / ClLds / cl_forward it steps.
#include "common.h"
#include "ppo_model_step.h"

namespace stove {

template <int CL>
struct PcShape {
  using R = RhCl<CL>;
  static constexpr bool kRhStaged = CL <= 16;                        // the reward head's tables in LDS
  static constexpr int kApp = env_step::kMaxObjects * (CL / 2 - 4);  // the trajectory's appearance rows at their widest
  static constexpr int kRhV = 2 * CL + R::H1 + 2 * R::H2 + 4;        // the reward head's vectors (plan_finish_k's V)
  static constexpr int kRhFloats = kRhStaged ? 2 * CL * CL + CL * R::H1 + R::H1 * R::H2 + kRhV : 0;
  // the launch's LDS beyond the dynamics' (GC<CL>::kLdsFloats): policy rows, the reward head's scratch, the embedding, the appearance
  static constexpr int kFloats = kPmObsFloats + 2 * ppo_policy::kMaxWidth + kPmHeadFloats + CL + kPmEmbRows * ppo_policy::kActions +
                                 kPmEmbRows + kApp + 4 + kRhFloats;
  static constexpr size_t kFixedBytes = (size_t)(GC<CL>::kLdsFloats + kFloats) * sizeof(float);
  static_assert(kFloats % 4 == 0 && GC<CL>::kLdsFloats % 4 == 0, "the scratch and the image behind it stay 16-byte aligned");
  // cl_forward places nothing beside the dynamic part today; a KiB is left for what a compiler may
  static_assert(kFixedBytes + 1024 <= kPmLdsLimit, "the step's LDS and the policy's rows fit one CU");
};

static_assert(PcShape<16>::kFixedBytes == 78720 && PcShape<32>::kFixedBytes == 137328 && PcShape<64>::kFixedBytes == 150896,
              "the launch's LDS is part of what `staged` decides");

template <int CL>
struct PcLds {
  float *o, *a, *b, *heads, *xs, *embw, *embb, *app, *Wt0a, *Wt0b, *Wt1a, *Wt1b, *V, *img;
  int* act;
};
template <int CL>
__device__ __forceinline__ PcLds<CL> pc_carve(float* base) {
  using S = PcShape<CL>;
  using R = RhCl<CL>;
  PcLds<CL> M;
  M.o = base;
  M.a = M.o + kPmObsFloats;
  M.b = M.a + ppo_policy::kMaxWidth;
  M.heads = M.b + ppo_policy::kMaxWidth;
  M.xs = M.heads + kPmHeadFloats;                          // [CL] the reward head's vector, wave 3's
  M.embw = M.xs + CL;                                      // [4N][9]
  M.embb = M.embw + kPmEmbRows * ppo_policy::kActions;     // [4N]
  M.app = M.embb + kPmEmbRows;                             // [N][app_dim]
  M.act = reinterpret_cast<int*>(M.app + S::kApp);
  M.Wt0a = M.app + S::kApp + 4;
  M.Wt0b = M.Wt0a + (S::kRhStaged ? CL * CL : 0);
  M.Wt1a = M.Wt0b + (S::kRhStaged ? CL * CL : 0);
  M.Wt1b = M.Wt1a + (S::kRhStaged ? CL * R::H1 : 0);
  M.V = M.Wt1b + (S::kRhStaged ? R::H1 * R::H2 : 0);
  M.img = M.Wt0a + S::kRhFloats;
  return M;
}

// the image is staged when it fits behind everything else
template <int CL>
inline bool pc_staged(size_t n_params) { return PcShape<CL>::kFixedBytes + 1024 + n_params * sizeof(float) <= kPmLdsLimit; }
template <int CL>
inline size_t pc_lds_bytes(size_t n_params) { return PcShape<CL>::kFixedBytes + (pc_staged<CL>(n_params) ? n_params * sizeof(float) : 0); }

// the reward head on the N rows of `pred` (LDS, row stride ld), by one wave: plan_finish_k<CL>'s arithmetic, nothing saved.  Lane
// l < CL holds element l; the lanes from CL up repeat lane l - CL's arithmetic and write nothing.
template <int CL>
__device__ __forceinline__ float pc_reward(const PcLds<CL>& M, const float* pred, int ld, const float* __restrict__ rh, int N, int lane) {
  using R = RhCl<CL>;
  constexpr int H1 = R::H1, H2 = R::H2;
  constexpr bool ST = PcShape<CL>::kRhStaged;
  const int l = lane & (CL - 1);
  const bool act = lane < CL;
  float* x = M.xs;
  const float *b0a = ST ? M.V : rh + R::B0A, *b0b = ST ? M.V + CL : rh + R::B0B, *b1a = ST ? M.V + 2 * CL : rh + R::B1A;
  const float *b1b = ST ? M.V + 2 * CL + H1 : rh + R::B1B, *w1c = ST ? M.V + 2 * CL + H1 + H2 : rh + R::W1C;
  const float* b1c = ST ? M.V + 2 * CL + H1 + 2 * H2 : rh + R::B1C;
  float hsum = 0.0f;
  for (int o = 0; o < N; ++o) {
    if (act) x[l] = pred[o * ld + l];
    float h = b0a[l] + (ST ? rh_dot_t<CL, CL>(M.Wt0a, x, l) : rh_dot_rows<CL, CL>(rh + R::W0A, x, l));
    h = fmaxf(h, 0.0f);
    if (act) x[l] = h;
    hsum += b0b[l] + (ST ? rh_dot_t<CL, CL>(M.Wt0b, x, l) : rh_dot_rows<CL, CL>(rh + R::W0B, x, l));
  }
  if (act) x[l] = hsum;
  const float a1 = fmaxf(b1a[l & (H1 - 1)] + (ST ? rh_dot_t<CL, H1>(M.Wt1a, x, l) : rh_dot_rows<CL, H1>(rh + R::W1A, x, l)), 0.0f);
  if (lane < H1) x[l] = a1;
  const float a2 = fmaxf(b1b[l & (H2 - 1)] + (ST ? rh_dot_t<H1, H2>(M.Wt1b, x, l) : rh_dot_rows<H1, H2>(rh + R::W1B, x, l)), 0.0f);
  if (lane < H2) x[l] = a2;
  float z = b1c[0];
#pragma unroll
  for (int k = 0; k < H2; ++k) z = fmaf(w1c[k], x[k], z);
  return 1.0f / (1.0f + expf(-z));
}

// grid B, block 256, dynamic LDS pc_lds_bytes<CL>.  z0 (B, N, cl/2 + 2); app (B, N, app_dim) or null; params the policy's image;
// emb_w (4N, 9), emb_b (4N); P the dynamics' image at CL; rh the reward head's block at CL; u (B, S); z_pred (B, S, N, cl/2 + 2);
// pred (B, S, N, CL) or null; obs (B, S + 1, 4N); actions, rewards, values, logp, returns (B, S); next_value, status (B,).
template <int CL>
__global__ __launch_bounds__(256) void ppo_collect_model_cl_k(PM_KERNEL_PARAMS) {
  using K = GC<CL>;
  using R = RhCl<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const PcLds<CL> M = pc_carve<CL>(lds + K::kLdsFloats);
  const int b = blockIdx.x, tid = (int)threadIdx.x, wv = wave_id(), lane = lane_id();
  const int sin_dim = D + 4 + app_dim, W = 4 * N, Ly = ppo_policy::layers(sh);
  const GnnShape gs = make_shape(N, 1, b, B, sin_dim, lim_enc, elu);
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, gs, P + 2 * K::W_END);
  float* Z = L.X;          // [N][LDZ] the current state
  for (int i = tid; i < N * ZW; i += blockDim.x) Z[(i / ZW) * LDZ + i % ZW] = z0[(size_t)b * N * ZW + i];
  for (int i = tid; i < W * ppo_policy::kActions; i += blockDim.x) M.embw[i] = emb_w[i];
  if (tid < W) M.embb[tid] = emb_b[tid];
  for (int i = tid; i < N * app_dim; i += blockDim.x) M.app[i] = app[(size_t)b * N * app_dim + i];
  if constexpr (PcShape<CL>::kRhStaged) {          // the reward head's tables, transposed as plan_finish_k keeps them
    constexpr int H1 = R::H1, H2 = R::H2;
    for (int i = tid; i < CL * CL; i += blockDim.x) {
      const int o = i / CL, k = i % CL;                    // W (out o, in k) -> Wt[k][o]
      M.Wt0a[k * CL + o] = rh[R::W0A + i];
      M.Wt0b[k * CL + o] = rh[R::W0B + i];
    }
    for (int i = tid; i < H1 * CL; i += blockDim.x) M.Wt1a[(i % CL) * H1 + i / CL] = rh[R::W1A + i];
    for (int i = tid; i < H2 * H1; i += blockDim.x) M.Wt1b[(i % H1) * H2 + i / H1] = rh[R::W1B + i];
    float *b0a = M.V, *b0b = M.V + CL, *b1a = M.V + 2 * CL, *b1b = b1a + H1, *w1c = b1b + H2, *b1c = w1c + H2;
    for (int i = tid; i < CL; i += blockDim.x) { b0a[i] = rh[R::B0A + i]; b0b[i] = rh[R::B0B + i]; }
    for (int i = tid; i < H1; i += blockDim.x) b1a[i] = rh[R::B1A + i];
    for (int i = tid; i < H2; i += blockDim.x) { b1b[i] = rh[R::B1B + i]; w1c[i] = rh[R::W1C + i]; }
    if (tid == 0) b1c[0] = rh[R::B1C];
  }
  const float* wts = params;
  if (staged) {
    for (int i = tid; i < n_params; i += blockDim.x) M.img[i] = params[i];
    wts = M.img;
  }
  __syncthreads();
  bool going = true;
  for (int t = 0; t <= S; ++t) {
    if (tid < W) M.o[tid] = ppo_policy::observe_model(Z[(tid >> 2) * LDZ + 2 + (tid & 3)], tid & 3, hw);
    __syncthreads();
    const float* in = M.o;
    for (int ly = 0; ly < Ly; ++ly) {
      const int Kin = ppo_policy::width_in(sh, ly), J = ppo_policy::width_out(sh, ly);
      const float* wT = wts + ppo_policy::offset(sh, ly);
      float* out = ly == Ly - 1 ? M.heads : (ly & 1) ? M.b : M.a;
      if (tid < J) out[tid] = ppo_policy::neuron(wT, wT + (size_t)Kin * J, in, Kin, J, tid, ly != Ly - 1);
      __syncthreads();
      in = out;
    }
    if (!ppo_policy::heads_finite(M.heads)) {      // (every thread reads the same ten words)
      going = false;
      break;
    }
    if (tid < W) obs[((size_t)b * (S + 1) + t) * W + tid] = M.o[tid];
    if (t == S) break;
    const size_t at = (size_t)b * S + t;
    if (tid == 0) {
      float lp;
      double margin;
      values[at] = M.heads[0];
      const int action = ppo_policy::draw(M.heads + 1, u[at], &lp, &margin);
      actions[at] = action;
      logp[at] = lp;
      M.act[0] = action;
    }
    __syncthreads();
    for (int i = tid; i < N * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      float v;
      if (c < D) {
        v = Z[r * LDZ + 2 + c];
      } else if (c < D + 4) {       // the embedding Linear on a one-hot row, in small_linear_k's order of operations (the same bits)
        const int action = M.act[0], o = r * 4 + (c - D);
        v = M.embb[o];
        for (int k = 0; k < ppo_policy::kActions; ++k) v = fmaf(k == action ? 1.0f : 0.0f, M.embw[o * ppo_policy::kActions + k], v);
      } else {
        v = M.app[r * app_dim + (c - D - 4)];
      }
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, gs, P);
    for (int idx = tid; idx < N * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      float v;
      if (q < 2) {
        v = Z[r * LDZ + q];                                  // scale stays constant
      } else {
        const int d = q - 2;
        v = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f + (d < 2 ? L.SIN[r * LDN + d] : 0.0f);
      }
      z_pred[(at * N + r) * ZW + q] = v;
      Z[r * LDZ + q] = v;
    }
    if (pred != nullptr) {
      for (int i = tid; i < N * CL; i += blockDim.x) {
        const int r = i / CL, c = i % CL;
        pred[(at * N + r) * CL + c] = L.PRED[r * LDN + c];
      }
    }
    if (wv == 3) {
      const float rw = pc_reward<CL>(M, L.PRED, LDN, rh, N, lane);
      if (lane == 0) rewards[at] = rw - 1.0f;
    }
    __syncthreads();
  }
  if (going && wv == 3 && lane == 0) {          // (the thread that wrote the rewards)
    next_value[b] = M.heads[0];
    ppo_policy::discounted(rewards + (size_t)b * S, M.heads[0], discount, S, returns + (size_t)b * S);
  }
  if (tid == 0) status[b] = going ? ppo_policy::kOk : ppo_policy::kNonFinite;
}

}  // namespace stove
