// The relational GNN core, the inference recursion and the rollout with the state-code length as a compile-time
// parameter (instantiated for cl = 16 and 64; cl = 32 keeps the tuned kernels of gnn.hip / gnn_small*.hip).
//
// Same formulation as the MFMA kernels of gnn.hip: a persistent workgroup (256 threads, 4 waves) owns G whole sequences
// for the whole time loop; every dense layer is a set of 16x16 tiles of v_mfma_f32_16x16x4_f32 (exact f32); the first
// edge layer is factorised W0 [s_i | s_j | d] = W0a s_i + W0b s_j + w_d d; the backward recomputes the step's forward in
// LDS and accumulates the weight gradients in MFMA accumulators across ALL time steps, written once per workgroup and
// reduced in a fixed order (no atomics: bitwise reproducible).  Bias / vector gradients are per-thread column sums kept
// in registers across the time loop.  Every offset (image sections, LDS strides, tile numbers) derives from CL.
//
// LDS budget (GC<CL>::kLdsFloats): the layout of gnn.hip (16 node rows, 80 edge rows) needs ~270 KB at cl = 64, above
// the 160 KB of a CU.  At cl = 64 a workgroup therefore owns ONE sequence (N <= 6: 8 node rows, 48 edge rows; MFMA
// operand rows past the 8th read as zero) and the backward-only edge buffer E32 aliases P, whose forward values are
// dead by then: 148 KB.  At cl = 16 the full 16 node rows / 80 edge rows cost 76 KB and up to floor(16/N) sequences
// share a workgroup.
//
// Included from capi.hip after gnn.hip, whose tile_each / act_phi / fast_tanh / GnnShape / LoopConst it reuses.
#include <type_traits>

#include "common.h"

namespace stove {

template <int CL>
struct GC {
  static constexpr int C = CL, D = CL / 2, ZW = CL / 2 + 2, CC = CL * CL;
  // parameter image P = [ W | W^T | VEC ] (floats); W: row-major [out][K]; W^T: the transposes
  static constexpr int W_ENC = 0, W_S0 = CC, W_S1 = 2 * CC, W_EF = 3 * CC, W_R1 = 11 * CC, W_A1 = 13 * CC, W_R2 = 15 * CC,
                       W_F0 = 16 * CC, W_F1 = 17 * CC, W_F2 = 18 * CC, W_O0 = 19 * CC, W_O1 = 21 * CC, W_END = 22 * CC;
  static constexpr int V_ENC = 0, V_S0 = C, V_S1 = 2 * C, V_BR0 = 3 * C, V_WDR = 5 * C, V_BA0 = 7 * C, V_WDA = 9 * C, V_BR1 = 11 * C,
                       V_BA1 = 12 * C, V_BR2 = 13 * C, V_WA2 = 14 * C, V_BA2 = 15 * C, V_F0 = 16 * C, V_F1 = 17 * C, V_F2 = 18 * C,
                       V_O0 = 19 * C, V_O1 = 20 * C, V_END = 21 * C;
  static constexpr int kParams = 2 * W_END + V_END;
  static constexpr int kGrads = W_END + V_END;           // gradient image (W layout + VEC)
  static constexpr int NRP = CL <= 32 ? 16 : 8;          // node rows kept in LDS
  static constexpr int NEM = CL <= 32 ? 80 : 48;         // edge rows kept in LDS (a multiple of 16)
  static constexpr int LDN = C + 4, LDC = 2 * C + 4, LDP = 8 * C + 4, LDZ = ZW + 2;
  // weight-gradient tiles (16 x 16) are numbered through the W image: tile T lives in wave T & 3, accumulator T >> 2
  static constexpr int NSLOT = (W_END / 256 + 3) / 4;
  static constexpr int VQ = (V_END + 255) / 256;         // vector-gradient elements per thread
  static constexpr int kLdsFloats = 11 * NRP * LDN + 2 * NRP * LDC + NRP * LDP + 2 * NEM * LDC + 3 * NEM * LDN + 3 * NEM + 32 + 32 +
                                    V_END + 2 * NEM + 32 + 16 * LDZ;
  static_assert(NEM * LDN <= NRP * LDP, "E32 aliases P");
  static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS budget of a CU");
};

template <int CL>
struct ClLds {
  float *SIN, *H1, *SD, *PRED, *F1, *F2, *O1, *RES, *DA, *DB, *DC;   // [NRP][LDN]
  float *CAT, *DCAT;                                                  // [NRP][LDC]  CAT = [F3 | S]
  float* P;                                                           // [NRP][LDP]
  float* E32;                                                         // [NEM][LDN]  backward only, aliases P
  float *R1, *A1;                                                     // [NEM][LDC]
  float *R2, *A2, *R3;                                                // [NEM][LDN]
  float *ATT, *DIST, *DATT;                                           // [NEM]
  float* DDIST;                                                       // [16][2]
  float* PC;                                                          // [16][2] position carry of the time loop
  float* V;                                                           // [V_END] copy of the VEC image
  int *EI, *EJ;                                                       // [NEM] node rows of edge e = (g, i, j); -1 for padding
  int *NG, *NI;                                                       // [16]
  float* X;                                                           // [16][LDZ] state / gradient carry of the time loops
};

template <int CL>
__device__ __forceinline__ ClLds<CL> cl_carve(float* base) {
  using K = GC<CL>;
  ClLds<CL> L;
  float* p = base;
  auto take = [&](int n) { float* q = p; p += n; return q; };
  L.SIN = take(K::NRP * K::LDN); L.H1 = take(K::NRP * K::LDN); L.SD = take(K::NRP * K::LDN); L.PRED = take(K::NRP * K::LDN);
  L.F1 = take(K::NRP * K::LDN); L.F2 = take(K::NRP * K::LDN); L.O1 = take(K::NRP * K::LDN); L.RES = take(K::NRP * K::LDN);
  L.DA = take(K::NRP * K::LDN); L.DB = take(K::NRP * K::LDN); L.DC = take(K::NRP * K::LDN);
  L.CAT = take(K::NRP * K::LDC); L.DCAT = take(K::NRP * K::LDC);
  L.P = take(K::NRP * K::LDP);
  L.E32 = L.P;
  L.R1 = take(K::NEM * K::LDC); L.A1 = take(K::NEM * K::LDC);
  L.R2 = take(K::NEM * K::LDN); L.A2 = take(K::NEM * K::LDN); L.R3 = take(K::NEM * K::LDN);
  L.ATT = take(K::NEM); L.DIST = take(K::NEM); L.DATT = take(K::NEM);
  L.DDIST = take(32);
  L.PC = take(32);
  L.V = take(K::V_END);
  L.EI = reinterpret_cast<int*>(take(K::NEM));
  L.EJ = reinterpret_cast<int*>(take(K::NEM));
  L.NG = reinterpret_cast<int*>(take(16));
  L.NI = reinterpret_cast<int*>(take(16));
  L.X = take(16 * K::LDZ);
  return L;
}

// C(16x16) = A[16 x K] B^T: A rows in LDS (rows >= arows read as zero), B rows = output columns in global memory.
template <int K>
__device__ __forceinline__ f32x4 cl_tile(const float* A, int lda, int arows, const float* __restrict__ B, int ldb) {
  const int l = lane_id(), i = l & 15, kq = l >> 4;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  const bool ok = i < arows;
#pragma unroll 4
  for (int kb = 0; kb < K / 16; ++kb) {
    float4 a = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) a = *reinterpret_cast<const float4*>(A + i * lda + kb * 16 + 4 * kq);
    const float4 b = *reinterpret_cast<const float4*>(B + i * ldb + kb * 16 + 4 * kq);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

// weight gradient of one layer: acc tile (o, i) += sum_rows dO[row][o] In[row][i]; rows past `rows` read as zero
template <int OUT, int IN, int T0>
__device__ __forceinline__ void cl_dw(f32x4* acc, const float* dO, int ldo, const float* In, int ldi, int rows, int wv) {
  constexpr int NT = (OUT / 16) * (IN / 16);
  const int l = lane_id(), i = l & 15, kq = l >> 4;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    if (((T0 + k) & 3) != wv) continue;
    const int ot = k / (IN / 16), it = k % (IN / 16);
    f32x4 a = acc[(T0 + k) >> 2];
    for (int r0 = 0; r0 < rows; r0 += 16) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int r = r0 + 4 * kq + m;
        float x = 0.0f, y = 0.0f;
        if (r < rows) {
          x = dO[r * ldo + ot * 16 + i];
          y = In[r * ldi + it * 16 + i];
        }
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, a, 0, 0, 0);
      }
    }
    acc[(T0 + k) >> 2] = a;
  }
}
template <int OUT, int IN, int T0>
__device__ __forceinline__ void cl_dw_store(const f32x4* acc, float* __restrict__ img, int wv) {
  constexpr int NT = (OUT / 16) * (IN / 16);
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    if (((T0 + k) & 3) != wv) continue;
    const int ot = k / (IN / 16), it = k % (IN / 16);
    tile_each(acc[(T0 + k) >> 2], ot * 16, it * 16, [&](int r, int c, float v) { img[r * IN + c] = v; });
  }
}
// vector gradients: thread t owns elements t + 256 q of the VEC image; elements [v0, v0 + len) += sum_rows dO[row][.] * scale[row]
template <int CL>
__device__ __forceinline__ void cl_vec(float* vg, int v0, int len, const float* dO, int ldo, int rows, const float* scale) {
#pragma unroll
  for (int q = 0; q < GC<CL>::VQ; ++q) {
    const int v = (int)threadIdx.x + 256 * q;
    if (v >= v0 && v < v0 + len) {
      const int c = v - v0;
      float s = 0.0f;
      if (scale != nullptr) {
        for (int r = 0; r < rows; ++r) s = fmaf(dO[r * ldo + c], scale[r], s);
      } else {
        for (int r = 0; r < rows; ++r) s += dO[r * ldo + c];
      }
      vg[q] += s;
    }
  }
}

template <int CL>
__device__ __forceinline__ void cl_setup(const ClLds<CL>& L, const GnnShape& sh, const float* __restrict__ Vg) {
  using K = GC<CL>;
  const int tid = threadIdx.x;
  for (int i = tid; i < K::V_END; i += blockDim.x) L.V[i] = Vg[i];
  const int NN = sh.N * sh.N;
  if (tid < K::NEM) {
    int ei = -1, ej = -1;
    if (tid < sh.NE) {
      const int g = tid / NN, ij = tid % NN;
      ei = g * sh.N + ij / sh.N;
      ej = g * sh.N + ij % sh.N;
    }
    L.EI[tid] = ei;
    L.EJ[tid] = ej;
  }
  if (tid < 16) {
    L.NG[tid] = (tid / sh.N) * sh.N;
    L.NI[tid] = tid % sh.N;
  }
}

// =================================================================================================
// forward of one GNN step; input L.SIN (rows < NR, cols < sin_dim, rest zero), output L.RES, L.PRED
// =================================================================================================
template <int CL>
__device__ __forceinline__ void cl_forward(const ClLds<CL>& L, const GnnShape& sh, const float* __restrict__ Wf) {
  using K = GC<CL>;
  constexpr int C = K::C, LDN = K::LDN, LDC = K::LDC, LDP = K::LDP, NRP = K::NRP, CT = C / 16;
  const int wv = wave_id();
  const int tid = threadIdx.x;
  const float* V = L.V;
  float* S = L.CAT + C;   // S lives in CAT[:, C:2C]
  // 1. state encoder; raw positions (first lim_enc dims) are kept for the distances
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.SIN, LDN, NRP, Wf + K::W_ENC + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) S[r * LDC + c] = (c < sh.lim_enc) ? L.SIN[r * LDN + c] : v + V[K::V_ENC + c];
    });
  }
  WG_SYNC();
  // 2. self-dynamics layer 0, the factorised first edge layer (rel_i | rel_j | att_i | att_j), squared distances
  for (int t = wv; t < 9 * CT; t += 4) {
    if (t < 8 * CT) {
      const f32x4 acc = cl_tile<C>(S, LDC, NRP, Wf + K::W_EF + t * 16 * C, C);
      tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
        if (r < NRP) L.P[r * LDP + c] = v;
      });
    } else {
      const int n = t - 8 * CT;
      const f32x4 acc = cl_tile<C>(S, LDC, NRP, Wf + K::W_S0 + n * 16 * C, C);
      tile_each(acc, 0, n * 16, [&](int r, int c, float v) {
        if (r < NRP) L.H1[r * LDN + c] = act_phi(v + V[K::V_S0 + c], sh.elu);
      });
    }
  }
  if (tid < sh.ME * 16) {
    const int e = tid;
    float d = 0.0f;
    if (L.EI[e] >= 0) {
      const int ni = L.EI[e], nj = L.EJ[e];
      const float dx = S[ni * LDC] - S[nj * LDC], dy = S[ni * LDC + 1] - S[nj * LDC + 1];
      d = dx * dx + dy * dy;
    }
    L.DIST[e] = d;
  }
  WG_SYNC();
  // 3. edge pre-activations (gather) + self-dynamics layer 1
  for (int idx = tid; idx < sh.ME * 16 * 2 * C; idx += blockDim.x) {
    const int e = idx / (2 * C), c = idx % (2 * C);
    float r1 = 0.0f, a1 = 0.0f;
    const int ni = L.EI[e];
    if (ni >= 0) {
      const int nj = L.EJ[e];
      const float d = L.DIST[e];
      r1 = act_phi(L.P[ni * LDP + c] + L.P[nj * LDP + 2 * C + c] + V[K::V_WDR + c] * d + V[K::V_BR0 + c], sh.elu);
      a1 = act_phi(L.P[ni * LDP + 4 * C + c] + L.P[nj * LDP + 6 * C + c] + V[K::V_WDA + c] * d + V[K::V_BA0 + c], sh.elu);
    }
    L.R1[e * LDC + c] = r1;
    L.A1[e * LDC + c] = a1;
  }
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.H1, LDN, NRP, Wf + K::W_S1 + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.SD[r * LDN + c] = v + V[K::V_S1 + c] + L.H1[r * LDN + c];
    });
  }
  WG_SYNC();
  // 4. second edge layers (2C -> C), relation and attention
  for (int t = wv; t < sh.ME * CT * 2; t += 4) {
    const int which = t & 1, n = (t >> 1) % CT, m = (t >> 1) / CT;
    if (which == 0) {
      const f32x4 acc = cl_tile<2 * C>(L.R1 + m * 16 * LDC, LDC, 16, Wf + K::W_R1 + n * 16 * 2 * C, 2 * C);
      tile_each(acc, m * 16, n * 16, [&](int r, int c, float v) { L.R2[r * LDN + c] = act_phi(v + V[K::V_BR1 + c], sh.elu); });
    } else {
      const f32x4 acc = cl_tile<2 * C>(L.A1 + m * 16 * LDC, LDC, 16, Wf + K::W_A1 + n * 16 * 2 * C, 2 * C);
      tile_each(acc, m * 16, n * 16, [&](int r, int c, float v) { L.A2[r * LDN + c] = act_phi(v + V[K::V_BA1 + c], sh.elu); });
    }
  }
  WG_SYNC();
  // 5. third edge layers: relation C -> C (+skip), attention C -> 1 -> exp
  if (tid < sh.ME * 16) {
    float q = V[K::V_BA2];
    for (int c = 0; c < C; ++c) q = fmaf(L.A2[tid * LDN + c], V[K::V_WA2 + c], q);
    L.ATT[tid] = (tid < sh.NE) ? __expf(q) : 0.0f;
  }
  for (int t = wv; t < sh.ME * CT; t += 4) {
    const int m = t / CT, n = t % CT;
    const f32x4 acc = cl_tile<C>(L.R2 + m * 16 * LDN, LDN, 16, Wf + K::W_R2 + n * 16 * C, C);
    tile_each(acc, m * 16, n * 16, [&](int r, int c, float v) { L.R3[r * LDN + c] = v + V[K::V_BR2 + c] + L.R2[r * LDN + c]; });
  }
  WG_SYNC();
  // 6. masked, attention-weighted aggregation over the other objects
  for (int idx = tid; idx < NRP * C; idx += blockDim.x) {
    const int r = idx / C, c = idx % C;
    float v = 0.0f;
    if (r < sh.NR) {
      const int i = L.NI[r], e0 = r * sh.N;                  // edges (r -> j) are rows e0 .. e0+N-1
      v = L.SD[r * LDN + c];
      for (int j = 0; j < sh.N; ++j)
        if (j != i) v = fmaf(L.R3[(e0 + j) * LDN + c], L.ATT[e0 + j], v);
    }
    L.PRED[r * LDN + c] = v;
  }
  WG_SYNC();
  // 7-11. affector and output MLPs
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.PRED, LDN, NRP, Wf + K::W_F0 + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.F1[r * LDN + c] = fast_tanh(v + V[K::V_F0 + c]);
    });
  }
  WG_SYNC();
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.F1, LDN, NRP, Wf + K::W_F1 + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.F2[r * LDN + c] = fast_tanh(v + V[K::V_F1 + c]) + L.F1[r * LDN + c];
    });
  }
  WG_SYNC();
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.F2, LDN, NRP, Wf + K::W_F2 + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.CAT[r * LDC + c] = v + V[K::V_F2 + c];
    });
  }
  WG_SYNC();
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<2 * C>(L.CAT, LDC, NRP, Wf + K::W_O0 + t * 16 * 2 * C, 2 * C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.O1[r * LDN + c] = fast_tanh(v + V[K::V_O0 + c]);
    });
  }
  WG_SYNC();
  for (int t = wv; t < CT; t += 4) {
    const f32x4 acc = cl_tile<C>(L.O1, LDN, NRP, Wf + K::W_O1 + t * 16 * C, C);
    tile_each(acc, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.RES[r * LDN + c] = v + V[K::V_O1 + c] + L.O1[r * LDN + c];
    });
  }
  WG_SYNC();
}

// =================================================================================================
// backward of one GNN step.  Requires the buffers left by cl_forward of the same step.
// in : L.DA = dL/dRES (rows >= NR zero);  dpred_up (global, may be null) = dL/dPRED from outside
// out: L.DA = dL/dSIN;  weight gradients accumulate into acc[NSLOT] (MFMA tiles) and vg[VQ].
// =================================================================================================
template <int CL>
__device__ __forceinline__ void cl_backward(const ClLds<CL>& L, const GnnShape& sh, const float* __restrict__ WT, f32x4* acc, float* vg,
                                            const float* dpred_up /* global or null */, size_t dpred_seq_stride) {
  using K = GC<CL>;
  constexpr int C = K::C, LDN = K::LDN, LDC = K::LDC, LDP = K::LDP, NRP = K::NRP, CT = C / 16;
  const int wv = wave_id();
  const int tid = threadIdx.x;
  const float* V = L.V;
  float* S = L.CAT + C;
  const int ER = sh.ME * 16;      // edge rows in use
  // b1. out.1:  RES = O1 W^T + b + O1
  cl_dw<C, C, K::W_O1 / 256>(acc, L.DA, LDN, L.O1, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_O1, C, L.DA, LDN, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DA, LDN, NRP, WT + K::W_O1 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) {
        const float o = L.O1[r * LDN + c];
        L.DB[r * LDN + c] = (v + L.DA[r * LDN + c]) * (1.0f - o * o);       // d pre-tanh of out.0
      }
    });
  }
  WG_SYNC();
  // b2. out.0 on CAT = [F3 | S]
  cl_dw<C, 2 * C, K::W_O0 / 256>(acc, L.DB, LDN, L.CAT, LDC, NRP, wv);
  cl_vec<CL>(vg, K::V_O0, C, L.DB, LDN, NRP, nullptr);
  for (int t = wv; t < 2 * CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DB, LDN, NRP, WT + K::W_O0 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.DCAT[r * LDC + c] = v;
    });
  }
  WG_SYNC();
  // b3. affector.2:  F3 = F2 W^T + b      (dF3 = DCAT[:, :C])
  cl_dw<C, C, K::W_F2 / 256>(acc, L.DCAT, LDC, L.F2, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_F2, C, L.DCAT, LDC, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DCAT, LDC, NRP, WT + K::W_F2 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) {
        const float th = L.F2[r * LDN + c] - L.F1[r * LDN + c];              // tanh(u) of affector.1
        L.DA[r * LDN + c] = v;                                               // dF2 (skip path)
        L.DC[r * LDN + c] = v * (1.0f - th * th);                            // du
      }
    });
  }
  WG_SYNC();
  // b4. affector.1:  F2 = tanh(F1 W^T + b) + F1
  cl_dw<C, C, K::W_F1 / 256>(acc, L.DC, LDN, L.F1, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_F1, C, L.DC, LDN, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DC, LDN, NRP, WT + K::W_F1 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) {
        const float f1 = L.F1[r * LDN + c];
        L.DB[r * LDN + c] = (v + L.DA[r * LDN + c]) * (1.0f - f1 * f1);      // d pre-tanh of affector.0
      }
    });
  }
  WG_SYNC();
  // b5. affector.0:  F1 = tanh(PRED W^T + b)
  cl_dw<C, C, K::W_F0 / 256>(acc, L.DB, LDN, L.PRED, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_F0, C, L.DB, LDN, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DB, LDN, NRP, WT + K::W_F0 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) {
        float up = 0.0f;
        if (dpred_up != nullptr && r < sh.NR) up = dpred_up[(size_t)(r / sh.N) * dpred_seq_stride + (r % sh.N) * C + c];
        L.DC[r * LDN + c] = v + up;                                          // dPRED = dSD
      }
    });
  }
  WG_SYNC();
  // b6a. d attention: 16 lanes per edge
  for (int e0 = 0; e0 < ER; e0 += 16) {
    const int e = e0 + (tid >> 4);
    const int ni = L.EI[e];
    float v = 0.0f;
    if (ni >= 0 && ni != L.EJ[e])
      for (int c = tid & 15; c < C; c += 16) v = fmaf(L.DC[ni * LDN + c], L.R3[e * LDN + c], v);
    v = row_sum_lane15(v);
    if ((tid & 15) == 15) L.DATT[e] = v * L.ATT[e];                          // att = exp(q)
  }
  WG_SYNC();
  // b6b. dR3 in place; attention output layer grads (A2 still holds the forward values)
  cl_vec<CL>(vg, K::V_WA2, C, L.A2, LDN, ER, L.DATT);
  cl_vec<CL>(vg, K::V_BA2, 1, L.DATT, 1, ER, nullptr);
  for (int idx = tid; idx < ER * C; idx += blockDim.x) {
    const int e = idx / C, c = idx % C;
    const int ni = L.EI[e];
    float v = 0.0f;
    if (ni >= 0 && ni != L.EJ[e]) v = L.DC[ni * LDN + c] * L.ATT[e];
    L.R3[e * LDN + c] = v;
  }
  WG_SYNC();
  // b7. rel.2:  R3 = R2 W^T + b + R2 ;  attention pre-activation grads in place in A2
  cl_dw<C, C, K::W_R2 / 256>(acc, L.R3, LDN, L.R2, LDN, ER, wv);
  cl_vec<CL>(vg, K::V_BR2, C, L.R3, LDN, ER, nullptr);
  for (int t = wv; t < sh.ME * CT; t += 4) {
    const int m = t / CT, n = t % CT;
    const f32x4 a = cl_tile<C>(L.R3 + m * 16 * LDN, LDN, 16, WT + K::W_R2 + n * 16 * C, C);
    tile_each(a, m * 16, n * 16, [&](int r, int c, float v) {
      L.E32[r * LDN + c] = (v + L.R3[r * LDN + c]) * dphi_from_out(L.R2[r * LDN + c], sh.elu);
    });
  }
  for (int idx = tid; idx < ER * C; idx += blockDim.x) {
    const int e = idx / C, c = idx % C;
    const float y = L.A2[e * LDN + c];
    L.A2[e * LDN + c] = L.DATT[e] * V[K::V_WA2 + c] * dphi_from_out(y, sh.elu);
  }
  WG_SYNC();
  // b8. rel.1 / att.1 weight grads (inputs R1 / A1 still intact)
  cl_dw<C, 2 * C, K::W_R1 / 256>(acc, L.E32, LDN, L.R1, LDC, ER, wv);
  cl_dw<C, 2 * C, K::W_A1 / 256>(acc, L.A2, LDN, L.A1, LDC, ER, wv);
  cl_vec<CL>(vg, K::V_BR1, C, L.E32, LDN, ER, nullptr);
  cl_vec<CL>(vg, K::V_BA1, C, L.A2, LDN, ER, nullptr);
  WG_SYNC();
  // b9. rel.1 / att.1 data grads, multiplied by phi'(first-layer output), in place in R1 / A1
  for (int t = wv; t < sh.ME * 2 * CT * 2; t += 4) {
    const int which = t & 1, n = (t >> 1) % (2 * CT), m = (t >> 1) / (2 * CT);
    if (which == 0) {
      const f32x4 a = cl_tile<C>(L.E32 + m * 16 * LDN, LDN, 16, WT + K::W_R1 + n * 16 * C, C);
      tile_each(a, m * 16, n * 16, [&](int r, int c, float v) { L.R1[r * LDC + c] = v * dphi_from_out(L.R1[r * LDC + c], sh.elu); });
    } else {
      const f32x4 a = cl_tile<C>(L.A2 + m * 16 * LDN, LDN, 16, WT + K::W_A1 + n * 16 * C, C);
      tile_each(a, m * 16, n * 16, [&](int r, int c, float v) { L.A1[r * LDC + c] = v * dphi_from_out(L.A1[r * LDC + c], sh.elu); });
    }
  }
  WG_SYNC();
  // b10. first edge layer: scatter (as a gather) into dP, bias / distance-weight grads, d distance
  cl_vec<CL>(vg, K::V_BR0, 2 * C, L.R1, LDC, ER, nullptr);
  cl_vec<CL>(vg, K::V_WDR, 2 * C, L.R1, LDC, ER, L.DIST);
  cl_vec<CL>(vg, K::V_BA0, 2 * C, L.A1, LDC, ER, nullptr);
  cl_vec<CL>(vg, K::V_WDA, 2 * C, L.A1, LDC, ER, L.DIST);
  for (int idx = tid; idx < NRP * 8 * C; idx += blockDim.x) {
    const int r = idx / (8 * C), c = idx % (8 * C);
    const int blk = c / (2 * C), cc = c % (2 * C);
    float v = 0.0f;
    if (r < sh.NR) {
      const float* src = (blk < 2) ? L.R1 : L.A1;
      const int g0 = L.NG[r], i = L.NI[r];
      if (blk & 1) {
        for (int j = 0; j < sh.N; ++j) v += src[((g0 + j) * sh.N + i) * LDC + cc];      // r as the second argument s_j
      } else {
        for (int j = 0; j < sh.N; ++j) v += src[(r * sh.N + j) * LDC + cc];             // r as the first argument s_i
      }
    }
    L.P[r * LDP + c] = v;
  }
  // dL/d dist_e: 16 lanes per edge, row reduction
  for (int e0 = 0; e0 < ER; e0 += 16) {
    const int e = e0 + (tid >> 4);
    float v = 0.0f;
    for (int c = tid & 15; c < 2 * C; c += 16)
      v += L.R1[e * LDC + c] * V[K::V_WDR + c] + L.A1[e * LDC + c] * V[K::V_WDA + c];
    v = row_sum_lane15(v);
    if ((tid & 15) == 15) L.DATT[e] = v;
  }
  WG_SYNC();
  // b11. edge-first + self.1
  cl_dw<8 * C, C, K::W_EF / 256>(acc, L.P, LDP, S, LDC, NRP, wv);
  cl_dw<C, C, K::W_S1 / 256>(acc, L.DC, LDN, L.H1, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_S1, C, L.DC, LDN, NRP, nullptr);
  for (int t = wv; t < 2 * CT; t += 4) {
    if (t < CT) {
      // dS from the edge layers: dP (rows x 8C) Wef (8C x C)
      const f32x4 a = cl_tile<8 * C>(L.P, LDP, NRP, WT + K::W_EF + t * 16 * 8 * C, 8 * C);
      tile_each(a, 0, t * 16, [&](int r, int c, float v) {
        if (r < NRP) L.DA[r * LDN + c] = v;
      });
    } else {
      const int n = t - CT;
      const f32x4 a = cl_tile<C>(L.DC, LDN, NRP, WT + K::W_S1 + n * 16 * C, C);
      tile_each(a, 0, n * 16, [&](int r, int c, float v) {
        if (r < NRP) L.DB[r * LDN + c] = (v + L.DC[r * LDN + c]) * dphi_from_out(L.H1[r * LDN + c], sh.elu);   // d pre-act of self.0
      });
    }
  }
  if (tid < 32) {
    const int r = tid >> 1, ax = tid & 1;
    float s = 0.0f;
    if (r < sh.NR) {
      const int g0 = L.NG[r], i = L.NI[r];
      for (int j = 0; j < sh.N; ++j) {
        const float diff = S[r * LDC + ax] - S[(g0 + j) * LDC + ax];
        s += 2.0f * diff * (L.DATT[r * sh.N + j] + L.DATT[(g0 + j) * sh.N + i]);
      }
    }
    L.DDIST[tid] = s;
  }
  WG_SYNC();
  // b12. self.0 ; total dS ; split into the encoder output part and the pass-through part
  cl_dw<C, C, K::W_S0 / 256>(acc, L.DB, LDN, S, LDC, NRP, wv);
  cl_vec<CL>(vg, K::V_S0, C, L.DB, LDN, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DB, LDN, NRP, WT + K::W_S0 + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) {
        float tot = v + L.DA[r * LDN + c] + L.DCAT[r * LDC + C + c];
        if (c < 2) tot += L.DDIST[r * 2 + c];
        const bool raw = c < sh.lim_enc;
        L.DC[r * LDN + c] = raw ? 0.0f : tot;      // d encoder output
        L.F1[r * LDN + c] = raw ? tot : 0.0f;      // straight to SIN (F1 is dead by now)
      }
    });
  }
  WG_SYNC();
  // b13. encoder
  cl_dw<C, C, K::W_ENC / 256>(acc, L.DC, LDN, L.SIN, LDN, NRP, wv);
  cl_vec<CL>(vg, K::V_ENC, C, L.DC, LDN, NRP, nullptr);
  for (int t = wv; t < CT; t += 4) {
    const f32x4 a = cl_tile<C>(L.DC, LDN, NRP, WT + K::W_ENC + t * 16 * C, C);
    tile_each(a, 0, t * 16, [&](int r, int c, float v) {
      if (r < NRP) L.DA[r * LDN + c] = v + L.F1[r * LDN + c];
    });
  }
  WG_SYNC();
}

template <int CL>
__device__ __forceinline__ void cl_store_grads(const f32x4* acc, const float* vg, float* __restrict__ gout) {
  using K = GC<CL>;
  constexpr int C = K::C;
  const int wv = wave_id();
  cl_dw_store<C, C, K::W_ENC / 256>(acc, gout + K::W_ENC, wv);
  cl_dw_store<C, C, K::W_S0 / 256>(acc, gout + K::W_S0, wv);
  cl_dw_store<C, C, K::W_S1 / 256>(acc, gout + K::W_S1, wv);
  cl_dw_store<8 * C, C, K::W_EF / 256>(acc, gout + K::W_EF, wv);
  cl_dw_store<C, 2 * C, K::W_R1 / 256>(acc, gout + K::W_R1, wv);
  cl_dw_store<C, 2 * C, K::W_A1 / 256>(acc, gout + K::W_A1, wv);
  cl_dw_store<C, C, K::W_R2 / 256>(acc, gout + K::W_R2, wv);
  cl_dw_store<C, C, K::W_F0 / 256>(acc, gout + K::W_F0, wv);
  cl_dw_store<C, C, K::W_F1 / 256>(acc, gout + K::W_F1, wv);
  cl_dw_store<C, C, K::W_F2 / 256>(acc, gout + K::W_F2, wv);
  cl_dw_store<C, 2 * C, K::W_O0 / 256>(acc, gout + K::W_O0, wv);
  cl_dw_store<C, C, K::W_O1 / 256>(acc, gout + K::W_O1, wv);
#pragma unroll
  for (int q = 0; q < K::VQ; ++q) {
    const int v = (int)threadIdx.x + 256 * q;
    if (v < K::V_END) gout[K::W_END + v] = vg[q];
  }
}

// sequences per workgroup
template <int CL>
__host__ __device__ inline int cl_group_for(int B, int N) {
  if (GC<CL>::NRP < 16) return 1;
  const int a = 16 / N, b = GC<CL>::NEM / (N * N);
  int gmax = a < b ? a : b;
  if (gmax < 1) gmax = 1;
  int g = (B + 255) / 256;
  if (g < 1) g = 1;
  return g > gmax ? gmax : g;
}

template <int CL>
__device__ __forceinline__ void cl_load_sin(const ClLds<CL>& L, const GnnShape& sh, const float* __restrict__ sin, int b0) {
  for (int i = threadIdx.x; i < sh.NR * sh.sin_dim; i += blockDim.x) {
    const int r = i / sh.sin_dim, c = i % sh.sin_dim;
    L.SIN[r * GC<CL>::LDN + c] = sin[((size_t)b0 * sh.N + r) * sh.sin_dim + c];
  }
}

// =================================================================================================
// single step: Dynamics.forward(s) -> result (B,N,CL), dynamic_pred (B,N,CL)
// =================================================================================================
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_step_fwd_k(const float* __restrict__ sin, const float* __restrict__ P,
                                                         float* __restrict__ res, float* __restrict__ pred,
                                                         int B, int N, int G, int sin_dim, int lim_enc, int elu) {
  using K = GC<CL>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  cl_load_sin<CL>(L, sh, sin, b0);
  WG_SYNC();
  cl_forward<CL>(L, sh, P);
  for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
    const int r = i / CL, c = i % CL;
    res[((size_t)b0 * N + r) * CL + c] = L.RES[r * K::LDN + c];
    if (pred != nullptr) pred[((size_t)b0 * N + r) * CL + c] = L.PRED[r * K::LDN + c];
  }
}

template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_step_bwd_k(const float* __restrict__ sin, const float* __restrict__ P,
                                                         const float* __restrict__ dres, const float* __restrict__ dpred,
                                                         float* __restrict__ dsin, float* __restrict__ gpart,
                                                         int B, int N, int G, int sin_dim, int lim_enc, int elu) {
  using K = GC<CL>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  cl_load_sin<CL>(L, sh, sin, b0);
  f32x4 acc[K::NSLOT];
  float vg[K::VQ];
#pragma unroll
  for (int k = 0; k < K::NSLOT; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < K::VQ; ++k) vg[k] = 0.0f;
  WG_SYNC();
  cl_forward<CL>(L, sh, P);
  for (int i = threadIdx.x; i < K::NRP * CL; i += blockDim.x) {
    const int r = i / CL, c = i % CL;
    L.DA[r * K::LDN + c] = (r < sh.NR) ? dres[((size_t)b0 * N + r) * CL + c] : 0.0f;
  }
  WG_SYNC();
  cl_backward<CL>(L, sh, P + K::W_END, acc, vg, dpred != nullptr ? dpred + (size_t)b0 * N * CL : nullptr, (size_t)N * CL);
  for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
    const int r = i / sin_dim, c = i % sin_dim;
    dsin[((size_t)b0 * N + r) * sin_dim + c] = L.DA[r * K::LDN + c];
  }
  cl_store_grads<CL>(acc, vg, gpart + (size_t)blockIdx.x * K::kGrads);
}

// =================================================================================================
// inference recursion, as dyn_loop_fwd_k / dyn_loop_bwd_k of gnn.hip with D = CL/2 dynamic dims:
//   z1 (B,N,D+2) [sx, sy/sx, x, y, vx, vy, latent D-4];  zsup, zsstd (B,Ts,N,6);  eps (B,Ts,N,D+2);
//   extra (B,Ts,N,E), E = sin_dim - D;  outputs (B,Ts,N,.): z D+2, zdyn D, zdstd D, mean D+2, std D+2, pred CL (optional)
// =================================================================================================
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_loop_fwd_k(
    const float* __restrict__ z1, const float* __restrict__ zsup, const float* __restrict__ zsstd,
    const float* __restrict__ eps, const float* __restrict__ extra, const float* __restrict__ P,
    float* __restrict__ z, float* __restrict__ zdyn, float* __restrict__ zdstd, float* __restrict__ mean,
    float* __restrict__ stdv, float* __restrict__ pred,
    int B, int Ts, int N, int G, int sin_dim, int lim_enc, int elu, LoopConst kc) {
  using K = GC<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  const int E = sin_dim - D;
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  float* Z = L.X;     // [16][LDZ] current state z[t-1]
  for (int i = threadIdx.x; i < sh.NR * ZW; i += blockDim.x) Z[(i / ZW) * LDZ + i % ZW] = z1[(size_t)b0 * N * ZW + i];
  WG_SYNC();
  for (int ts = 0; ts < Ts; ++ts) {
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      float v;
      if (c < D) v = Z[r * LDZ + 2 + c];
      else v = extra[(((size_t)(b0 + r / N) * Ts + ts) * N + r % N) * E + (c - D)];
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    for (int idx = threadIdx.x; idx < sh.NR * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      const int b = b0 + r / N, n = r % N;
      const size_t o = ((size_t)b * Ts + ts) * N + n;
      float mu, sg;
      if (q < 2) {
        mu = zsup[o * 6 + q];
        sg = zsstd[o * 6 + q];
      } else {
        const int d = q - 2;
        const float m = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f;
        const float sd = std_scale(d, kc) * sigmoidf_(L.RES[r * LDN + D + d]);
        const float zd = m + (d < 2 ? L.SIN[r * LDN + d] : 0.0f);
        zdyn[o * D + d] = zd;
        zdstd[o * D + d] = sd;
        if (d < 4) {
          const float ms = zsup[o * 6 + 2 + d], ss = zsstd[o * 6 + 2 + d];
          const float sd2 = sd * sd, ss2 = ss * ss, DD = sd2 + ss2;
          mu = (ss2 * zd + sd2 * ms) / DD;
          sg = sd * ss / sqrtf(DD);
        } else {
          mu = zd;
          sg = sd;
        }
      }
      const float zv = fmaf(sg, eps[o * ZW + q], mu);
      z[o * ZW + q] = zv;
      mean[o * ZW + q] = mu;
      stdv[o * ZW + q] = sg;
      Z[r * LDZ + q] = zv;
    }
    if (pred != nullptr) {
      for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
        const int r = i / CL, c = i % CL;
        pred[(((size_t)(b0 + r / N) * Ts + ts) * N + r % N) * CL + c] = L.PRED[r * LDN + c];
      }
    }
    WG_SYNC();
  }
}

// backward of the recursion (the forward of every step is recomputed from the stored z).  Upstream gradients (any may be
// null): dz, dzdyn, dmean, dstd, dpred.  Outputs: dz1, dzsup, dzsstd, dextra, gpart[block][kGrads].
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_loop_bwd_k(
    const float* __restrict__ z1, const float* __restrict__ zsup, const float* __restrict__ zsstd,
    const float* __restrict__ eps, const float* __restrict__ extra, const float* __restrict__ P,
    const float* __restrict__ z,
    const float* __restrict__ dz, const float* __restrict__ dzdyn, const float* __restrict__ dmean,
    const float* __restrict__ dstd, const float* __restrict__ dpred,
    float* __restrict__ dz1, float* __restrict__ dzsup, float* __restrict__ dzsstd, float* __restrict__ dextra,
    float* __restrict__ gpart,
    int B, int Ts, int N, int G, int sin_dim, int lim_enc, int elu, LoopConst kc) {
  using K = GC<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  const int E = sin_dim - D;
  lds_zero(lds, K::kLdsFloats);
  f32x4 acc[K::NSLOT];
  float vg[K::VQ];
#pragma unroll
  for (int k = 0; k < K::NSLOT; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < K::VQ; ++k) vg[k] = 0.0f;
  float* CAR = L.X;   // [16][LDZ] gradient carried into z[t] from step t+1
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  WG_SYNC();
  for (int ts = Ts - 1; ts >= 0; --ts) {
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      const int b = b0 + r / N, n = r % N;
      float v;
      if (c < D) v = (ts == 0) ? z1[((size_t)b * N + n) * ZW + 2 + c] : z[(((size_t)b * Ts + ts - 1) * N + n) * ZW + 2 + c];
      else v = extra[(((size_t)b * Ts + ts) * N + n) * E + (c - D)];
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    // epilogue backward: per (row, q) -> dRES in L.DA, SuPAIR grads, position carry in L.PC
    for (int idx = threadIdx.x; idx < K::NRP * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      if (r >= sh.NR) {
        if (q >= 2) {
          L.DA[r * LDN + q - 2] = 0.0f;
          L.DA[r * LDN + D + q - 2] = 0.0f;
        }
        continue;
      }
      const int b = b0 + r / N, n = r % N;
      const size_t o = ((size_t)b * Ts + ts) * N + n;
      const float ep = eps[o * ZW + q];
      const float gz = (dz != nullptr ? dz[o * ZW + q] : 0.0f) + CAR[r * LDZ + q];
      const float gmu = gz + (dmean != nullptr ? dmean[o * ZW + q] : 0.0f);
      const float gsg = gz * ep + (dstd != nullptr ? dstd[o * ZW + q] : 0.0f);
      if (q < 2) {
        dzsup[o * 6 + q] = gmu;
        dzsstd[o * 6 + q] = gsg;
        continue;
      }
      const int d = q - 2;
      const float kd = std_scale(d, kc);
      const float m = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f;
      const float sd = kd * sigmoidf_(L.RES[r * LDN + D + d]);
      const float zd = m + (d < 2 ? L.SIN[r * LDN + d] : 0.0f);
      float gzd = (dzdyn != nullptr) ? dzdyn[o * D + d] : 0.0f;
      float gsd;
      if (d < 4) {
        const float ms = zsup[o * 6 + 2 + d], ss = zsstd[o * 6 + 2 + d];
        const float sd2 = sd * sd, ss2 = ss * ss, DD = sd2 + ss2, iD = 1.0f / DD;
        const float mu = (ss2 * zd + sd2 * ms) * iD;
        const float rD = rsqrtf(DD);
        gzd += gmu * ss2 * iD;
        gsd = gmu * (ms - mu) * iD * 2.0f * sd + gsg * ss * ss2 * iD * rD;
        dzsup[o * 6 + 2 + d] = gmu * sd2 * iD;
        dzsstd[o * 6 + 2 + d] = gmu * (zd - mu) * iD * 2.0f * ss + gsg * sd * sd2 * iD * rD;
      } else {
        gzd += gmu;
        gsd = gsg;
      }
      if (d < 2) L.PC[r * 2 + d] = gzd;                                    // z_dyn position = previous position + delta
      L.DA[r * LDN + d] = gzd * 0.5f * (1.0f - m * m);                      // m = 2 sigmoid - 1
      L.DA[r * LDN + D + d] = gsd * sd * (1.0f - sd / kd);                  // sd = k sigmoid
    }
    WG_SYNC();
    cl_backward<CL>(L, sh, P + K::W_END, acc, vg, dpred != nullptr ? dpred + ((size_t)b0 * Ts + ts) * N * CL : nullptr, (size_t)Ts * N * CL);
    // new carry into z[t-1]
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      const int b = b0 + r / N, n = r % N;
      const float g = L.DA[r * LDN + c];
      if (c < D) CAR[r * LDZ + 2 + c] = g + (c < 2 ? L.PC[r * 2 + c] : 0.0f);
      else dextra[(((size_t)b * Ts + ts) * N + n) * E + (c - D)] = g;
    }
    if (threadIdx.x < sh.NR * 2) CAR[(threadIdx.x >> 1) * LDZ + (threadIdx.x & 1)] = 0.0f;
    WG_SYNC();
  }
  for (int i = threadIdx.x; i < sh.NR * ZW; i += blockDim.x) dz1[(size_t)b0 * N * ZW + i] = CAR[(i / ZW) * LDZ + i % ZW];
  cl_store_grads<CL>(acc, vg, gpart + (size_t)blockIdx.x * K::kGrads);
}

// =================================================================================================
// generative rollout, mean prediction, forward only:
//   z_last (B,N,D+2); extra (B,A,N,E) indexed t % A or null;  z_pred (B,num,N,D+2); zstd (B,num,N,D), pred (B,num,N,CL) optional
// =================================================================================================
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_rollout_k(const float* __restrict__ z_last, const float* __restrict__ extra,
                                                        const float* __restrict__ P, float* __restrict__ z_pred,
                                                        float* __restrict__ zstd, float* __restrict__ pred,
                                                        int B, int num, int A, int N, int G, int sin_dim, int lim_enc, int elu, LoopConst kc) {
  using K = GC<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  const int E = sin_dim - D;
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  float* Z = L.X;
  for (int i = threadIdx.x; i < sh.NR * ZW; i += blockDim.x) Z[(i / ZW) * LDZ + i % ZW] = z_last[(size_t)b0 * N * ZW + i];
  WG_SYNC();
  for (int t = 0; t < num; ++t) {
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      float v;
      if (c < D) v = Z[r * LDZ + 2 + c];
      else v = extra[(((size_t)(b0 + r / N) * A + (t % A)) * N + r % N) * E + (c - D)];
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    for (int idx = threadIdx.x; idx < sh.NR * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      const size_t o = ((size_t)(b0 + r / N) * num + t) * N + r % N;
      float v;
      if (q < 2) {
        v = Z[r * LDZ + q];                                  // scale stays constant
      } else {
        const int d = q - 2;
        v = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f + (d < 2 ? L.SIN[r * LDN + d] : 0.0f);
        if (zstd != nullptr) zstd[o * D + d] = std_scale(d, kc) * sigmoidf_(L.RES[r * LDN + D + d]);
      }
      z_pred[o * ZW + q] = v;
      Z[r * LDZ + q] = v;
    }
    if (pred != nullptr) {
      for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
        const int r = i / CL, c = i % CL;
        pred[(((size_t)(b0 + r / N) * num + t) * N + r % N) * CL + c] = L.PRED[r * LDN + c];
      }
    }
    WG_SYNC();
  }
}

// =================================================================================================
// sampling rollout, forward only: gnn_cl_rollout_k with a draw per step, as rollout_sample_fwd_k (gnn.hip) is to rollout_fwd_k --
//   eps, log_q (B,num,N,D); z = mean + sd eps goes to z_pred and back into Z; no barrier the mean rollout does not have
// =================================================================================================
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_rollout_sample_k(const float* __restrict__ z_last, const float* __restrict__ extra,
                                                               const float* __restrict__ P, const float* __restrict__ eps,
                                                               float* __restrict__ z_pred, float* __restrict__ log_q,
                                                               float* __restrict__ zstd, float* __restrict__ pred,
                                                               int B, int num, int A, int N, int G, int sin_dim, int lim_enc, int elu, LoopConst kc) {
  using K = GC<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  const int E = sin_dim - D;
  lds_zero(lds, K::kLdsFloats);
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  float* Z = L.X;
  for (int i = threadIdx.x; i < sh.NR * ZW; i += blockDim.x) Z[(i / ZW) * LDZ + i % ZW] = z_last[(size_t)b0 * N * ZW + i];
  WG_SYNC();
  for (int t = 0; t < num; ++t) {
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      float v;
      if (c < D) v = Z[r * LDZ + 2 + c];
      else v = extra[(((size_t)(b0 + r / N) * A + (t % A)) * N + r % N) * E + (c - D)];
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    for (int idx = threadIdx.x; idx < sh.NR * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      const size_t o = ((size_t)(b0 + r / N) * num + t) * N + r % N;
      float v;
      if (q < 2) {
        v = Z[r * LDZ + q];                                  // scale stays constant
      } else {
        const int d = q - 2;
        const float mean = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f + (d < 2 ? L.SIN[r * LDN + d] : 0.0f);
        const float sd = std_scale(d, kc) * sigmoidf_(L.RES[r * LDN + D + d]);
        const float ep = eps[o * D + d];
        v = fmaf(sd, ep, mean);
        log_q[o * D + d] = sample_log_q(ep, sd);
        if (zstd != nullptr) zstd[o * D + d] = sd;
      }
      z_pred[o * ZW + q] = v;
      Z[r * LDZ + q] = v;                                  // the drawn state is the next step's input
    }
    if (pred != nullptr) {
      for (int i = threadIdx.x; i < sh.NR * CL; i += blockDim.x) {
        const int r = i / CL, c = i % CL;
        pred[(((size_t)(b0 + r / N) * num + t) * N + r % N) * CL + c] = L.PRED[r * LDN + c];
      }
    }
    WG_SYNC();
  }
}

// =================================================================================================
// backward of both rollouts, as rollout_bwd_k (gnn.hip) with D = CL/2: the time loop backwards, each step's forward recomputed from
// z_pred[:, t-1] (z_last at t = 0), weight gradients in the MFMA accumulators over all steps.  eps null: the mean rollout.
//   upstream (any may be null; d_log_q only with eps): d_z_pred (B,num,N,D+2), d_log_q (B,num,N,D), d_pred (B,num,N,CL)
//   outputs: d_z_last (B,N,D+2), d_extra (B,A,N,E) (every row written), gpart[block][kGrads]
// The carry lives in L.X (columns 0..1: the scale gradient summed over the steps); no buffer beyond cl_carve's.
// =================================================================================================
template <int CL>
__global__ __launch_bounds__(256) void gnn_cl_rollout_bwd_k(const float* __restrict__ z_last, const float* __restrict__ extra,
                                                            const float* __restrict__ P, const float* __restrict__ eps,
                                                            const float* __restrict__ z_pred, const float* __restrict__ d_z_pred,
                                                            const float* __restrict__ d_log_q, const float* __restrict__ d_pred,
                                                            float* __restrict__ d_z_last, float* d_extra, float* __restrict__ gpart,
                                                            int B, int num, int A, int N, int G, int sin_dim, int lim_enc, int elu, LoopConst kc) {
  using K = GC<CL>;
  constexpr int D = K::D, ZW = K::ZW, LDN = K::LDN, LDZ = K::LDZ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ClLds<CL> L = cl_carve<CL>(lds);
  const int b0 = blockIdx.x * G;
  const GnnShape sh = make_shape(N, G, b0, B, sin_dim, lim_enc, elu);
  const int E = sin_dim - D;
  lds_zero(lds, K::kLdsFloats);
  f32x4 acc[K::NSLOT];
  float vg[K::VQ];
#pragma unroll
  for (int k = 0; k < K::NSLOT; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < K::VQ; ++k) vg[k] = 0.0f;
  float* CAR = L.X;   // [16][LDZ] gradient carried into z_pred[t] from step t+1; columns 0..1: the scale gradient summed so far
  WG_SYNC();
  cl_setup<CL>(L, sh, P + 2 * K::W_END);
  if (d_extra != nullptr) {      // extra rows past the last step (A > num): nothing reads them
    for (int a = num; a < A; ++a)
      for (int i = threadIdx.x; i < sh.NR * E; i += blockDim.x)
        d_extra[(((size_t)(b0 + (i / E) / N) * A + a) * N + (i / E) % N) * E + i % E] = 0.0f;
  }
  WG_SYNC();
  for (int t = num - 1; t >= 0; --t) {
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      const int b = b0 + r / N, n = r % N;
      float v;
      if (c < D) v = (t == 0) ? z_last[((size_t)b * N + n) * ZW + 2 + c] : z_pred[(((size_t)b * num + t - 1) * N + n) * ZW + 2 + c];
      else v = extra[(((size_t)b * A + (t % A)) * N + n) * E + (c - D)];
      L.SIN[r * LDN + c] = v;
    }
    WG_SYNC();
    cl_forward<CL>(L, sh, P);
    // epilogue backward: per (row, q) -> dRES in L.DA, position carry in L.PC
    for (int idx = threadIdx.x; idx < K::NRP * ZW; idx += blockDim.x) {
      const int r = idx / ZW, q = idx % ZW;
      if (r >= sh.NR) {
        if (q >= 2) {
          L.DA[r * LDN + q - 2] = 0.0f;
          L.DA[r * LDN + D + q - 2] = 0.0f;
        }
        continue;
      }
      const size_t o = ((size_t)(b0 + r / N) * num + t) * N + r % N;
      const float gz = (d_z_pred != nullptr ? d_z_pred[o * ZW + q] : 0.0f) + CAR[r * LDZ + q];
      if (q < 2) {
        CAR[r * LDZ + q] = gz;                                               // z_pred[:, t, :, :2] = z_last[..., :2]
        continue;
      }
      const int d = q - 2;
      const float kd = std_scale(d, kc);
      const float m = 2.0f * sigmoidf_(L.RES[r * LDN + d]) - 1.0f;
      float gs = 0.0f;                                                       // sd * dL/dsd
      float sd = 0.0f;
      if (eps != nullptr) {
        // z = mean + sd eps, log_q = -eps^2/2 - log sd - const:  dL/dsd = gz eps - d_log_q / sd
        sd = kd * sigmoidf_(L.RES[r * LDN + D + d]);
        gs = gz * eps[o * D + d] * sd - (d_log_q != nullptr ? d_log_q[o * D + d] : 0.0f);
      }
      if (d < 2) L.PC[r * 2 + d] = gz;                                       // mean position = previous position + m
      L.DA[r * LDN + d] = gz * 0.5f * (1.0f - m * m);                        // m = 2 sigmoid - 1
      L.DA[r * LDN + D + d] = gs * (1.0f - sd / kd);                         // sd = k sigmoid
    }
    WG_SYNC();
    cl_backward<CL>(L, sh, P + K::W_END, acc, vg, d_pred != nullptr ? d_pred + ((size_t)b0 * num + t) * N * CL : nullptr,
                    (size_t)num * N * CL);
    // new carry into z_pred[t-1]
    for (int i = threadIdx.x; i < sh.NR * sin_dim; i += blockDim.x) {
      const int r = i / sin_dim, c = i % sin_dim;
      const float g = L.DA[r * LDN + c];
      if (c < D) {
        CAR[r * LDZ + 2 + c] = g + (c < 2 ? L.PC[r * 2 + c] : 0.0f);
      } else {
        float* dst = d_extra + (((size_t)(b0 + r / N) * A + (t % A)) * N + r % N) * E + (c - D);
        *dst = (t + A < num) ? *dst + g : g;                                 // a later step of this row has been here: same thread
      }
    }
    WG_SYNC();
  }
  for (int i = threadIdx.x; i < sh.NR * ZW; i += blockDim.x) d_z_last[(size_t)b0 * N * ZW + i] = CAR[(i / ZW) * LDZ + i % ZW];
  cl_store_grads<CL>(acc, vg, gpart + (size_t)blockIdx.x * K::kGrads);
}

// ---- host side of the entry points in capi.hip
// f(std::integral_constant<int, CL>) for a supported width
template <class F>
static inline int with_cl(int cl, F f) {
  if (cl == 16) return f(std::integral_constant<int, 16>{});
  if (cl == 64) return f(std::integral_constant<int, 64>{});
  return (int)hipErrorInvalidValue;
}
template <int CL>
static inline int cl_blocks(int B, int N) {
  const int g = cl_group_for<CL>(B, N);
  return (B + g - 1) / g;
}

}  // namespace stove
