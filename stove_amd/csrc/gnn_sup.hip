// The state-supervised baseline (reference model/supairvised/dynamics.py:39-107 with debug_rollout = True, train.py:77-108): the time
// loop around cl_forward / cl_backward of gnn_cl.hip with a cl-wide carry, and the discounted rollout loss.
//
//   code_0 = [x[:, 0] | latent0]
//   warm-up, i = 1 .. V-1:  res = core(code_{i-1});  code_i = [x[:, i] | res[..., 4:]]                       (labels are teacher-forced)
//   rollout, k = 0 .. R-1:  res = core(cur);  cur = [res[..., :2] + cur[..., :2] | res[..., 2:]];  pred[:, k] = cur[..., :4]
//
// core = Dynamics.forward(code, 0, lim_enc = 4) on a cl-wide code: sin_dim = cl, no sigmoid squashing, positions only are added.
// Both kernels are gnn_cl_rollout_k / gnn_cl_rollout_bwd_k with another epilogue; the core functions are used as they are.  The carry
// is cl wide and L.X only cl/2 + 4, so one more [NRP][LDN] buffer sits behind cl_carve's (SupC<CL>::kLdsFloats).
//
// Included from capi.hip after gnn_cl.hip.
#include "common.h"

namespace stove {

template <int CL>
struct SupC {
  using K = GC<CL>;
  static constexpr int kCarry = K::NRP * K::LDN;               // the code (forward) or its gradient (backward) between two steps
  static constexpr int kLdsFloats = K::kLdsFloats + kCarry;
  static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS budget of a CU");
};

// x (B,V,N,4), latent0 (B,N,CL-4) -> pred (B,R,N,4); codes (B,V-1+R,N,CL) (optional): the input code of every step
template <int CL>
__global__ __launch_bounds__(256) void gnn_sup_rollout_k(const float* __restrict__ x, const float* __restrict__ latent0,
                                                         const float* __restrict__ P, float* __restrict__ pred,
                                                         float* __restrict__ codes, int B, int V, int R, int N, int G, int elu) {
  using K = GC<CL>;
  constexpr int LDN = K::LDN;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  float* CUR = lds + K::kLdsFloats;        // [NRP][LDN] the current code
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, CL, 4, elu);
  const int S = V - 1 + R;
  lds_zero(lds, SupC<CL>::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
    const int r = i / CL, c = i % CL;
    const int b = b0 + r / N, n = r % N;
    CUR[r * LDN + c] = c < 4 ? x[(((size_t)b * V) * N + n) * 4 + c] : latent0[((size_t)b * N + n) * (CL - 4) + (c - 4)];
  }
  WG_SYNC();
  for (int s = 0; s < S; ++s) {
    for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
      const int r = i / CL, c = i % CL;
      const float v = CUR[r * LDN + c];
      L.SIN[r * LDN + c] = v;
      if (codes != nullptr) codes[(((size_t)(b0 + r / N) * S + s) * N + r % N) * CL + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
      const int r = i / CL, c = i % CL;
      const int b = b0 + r / N, n = r % N;
      float v = L.RES[r * LDN + c];
      if (s < V - 1) {
        if (c < 4) v = x[(((size_t)b * V + s + 1) * N + n) * 4 + c];          // the observed state replaces the predicted one
      } else {
        if (c < 2) v += L.SIN[r * LDN + c];
        if (c < 4) pred[(((size_t)b * R + (s - (V - 1))) * N + n) * 4 + c] = v;
      }
      CUR[r * LDN + c] = v;
    }
    WG_SYNC();
  }
}

// The time loop backwards; step s is recomputed from codes[:, s].  d_pred (B,R,N,4) -> d_latent0 (B,N,CL-4) (optional),
// gpart[block][kGrads].  x gets no gradient: columns 0..3 of a warm-up step's next code are labels.
template <int CL>
__global__ __launch_bounds__(256) void gnn_sup_rollout_bwd_k(const float* __restrict__ P, const float* __restrict__ codes,
                                                             const float* __restrict__ d_pred, float* __restrict__ d_latent0,
                                                             float* __restrict__ gpart, int B, int V, int R, int N, int G, int elu) {
  using K = GC<CL>;
  constexpr int LDN = K::LDN;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  float* CAR = lds + K::kLdsFloats;        // [NRP][LDN] gradient carried into the input code of step s+1
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, CL, 4, elu);
  const int S = V - 1 + R;
  lds_zero(lds, SupC<CL>::kLdsFloats);
  f32x4 acc[K::NSLOT];
  float vg[K::VQ];
#pragma unroll
  for (int k = 0; k < K::NSLOT; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < K::VQ; ++k) vg[k] = 0.0f;
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  WG_SYNC();
  for (int s = S - 1; s >= 0; --s) {
    for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
      const int r = i / CL, c = i % CL;
      L.SIN[r * LDN + c] = codes[(((size_t)(b0 + r / N) * S + s) * N + r % N) * CL + c];
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    // epilogue backward: dRES in L.DA, position carry in L.PC
    for (int i = threadIdx.x; i < K::NRP * CL; i += blockDim.x) {
      const int r = i / CL, c = i % CL;
      float g = 0.0f;
      if (r < sh.NR) {
        g = CAR[r * LDN + c];
        if (s >= V - 1) {
          if (c < 4) g += d_pred[(((size_t)(b0 + r / N) * R + (s - (V - 1))) * N + r % N) * 4 + c];
        } else if (c < 4) {
          g = 0.0f;                                                            // the next code's state columns are labels
        }
        if (c < 2) L.PC[r * 2 + c] = g;                                        // position = previous position + res (rollout steps)
      }
      L.DA[r * LDN + c] = g;
    }
    WG_SYNC();
    cl_backward<CL>(L, sh, P + K::W_END, acc, vg, nullptr, 0);
    for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
      const int r = i / CL, c = i % CL;
      CAR[r * LDN + c] = L.DA[r * LDN + c] + (c < 2 ? L.PC[r * 2 + c] : 0.0f);
    }
    WG_SYNC();
  }
  if (d_latent0 != nullptr) {
    for (int i = threadIdx.x; i < sh.NR * (CL - 4); i += blockDim.x) {
      const int r = i / (CL - 4), c = i % (CL - 4);
      d_latent0[((size_t)b0 * N + r) * (CL - 4) + c] = CAR[r * LDN + 4 + c];
    }
  }
  cl_store_grads<CL>(acc, vg, gpart + (size_t)blockIdx.x * K::kGrads);
}

// =================================================================================================
// The loss of SupTrainer.compute_loss and its gradient, one workgroup.  pred, future, d_pred (B,R,N,4); with e_t = pred_t - future_t
// and M = B N end entries per frame:
//   pred_loss  = sum_t df^(t+1) sum e_t^2 / M,   delta_loss = sum_{t < R-1} 6 df^(t+1) sum (e_{t+1} - e_t)^2 / M     (columns < end)
// losses = [pred_loss + delta_loss, pred_loss, delta_loss]; d_pred = d losses[0] / d pred, exact zeros in columns >= end.
// Thread t sums the entries t, t + 1024, ... in float64, then a tree over the threads: the order is fixed.
// =================================================================================================
constexpr int kSupLossThreads = 1024;

__global__ __launch_bounds__(kSupLossThreads) void sup_loss_k(const float* __restrict__ pred, const float* __restrict__ future,
                                                              float* __restrict__ losses, float* __restrict__ d_pred, int B, int R,
                                                              int N, int end, int with_delta, double discount) {
  __shared__ double sp[kSupLossThreads], sd[kSupLossThreads];
  const int n4 = N * 4, total = B * R * n4;
  const double inv = 1.0 / ((double)B * N * end);
  double ap = 0.0, ad = 0.0;
  for (int i = threadIdx.x; i < total; i += kSupLossThreads) {
    const int c = i & 3, t = (i / n4) % R;
    double g = 0.0;
    if (c < end) {
      const double w = pow(discount, (double)(t + 1));
      const double e = (double)pred[i] - (double)future[i];
      ap += w * e * e;
      g = 2.0 * w * e;
      if (with_delta && R > 1) {
        if (t < R - 1) {
          const double de = (double)pred[i + n4] - (double)future[i + n4] - e;
          ad += 6.0 * w * de * de;
          g -= 12.0 * w * de;
        }
        if (t > 0) {
          const double de = e - ((double)pred[i - n4] - (double)future[i - n4]);
          g += 12.0 * pow(discount, (double)t) * de;
        }
      }
    }
    d_pred[i] = (float)(g * inv);
  }
  sp[threadIdx.x] = ap;
  sd[threadIdx.x] = ad;
  __syncthreads();
  for (int h = kSupLossThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sp[threadIdx.x] += sp[threadIdx.x + h];
      sd[threadIdx.x] += sd[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double p = sp[0] * inv, d = sd[0] * inv;
    losses[0] = (float)(p + d);
    losses[1] = (float)p;
    losses[2] = (float)d;
  }
}

}  // namespace stove
