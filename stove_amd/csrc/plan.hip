// One expansion of a batch of search trees on the learned model (reference mcts_stove.py:95-137 and the value arithmetic of
// MCTS.backpropagate, :186-196): every tree m hands over the pool slot of the leaf it selected, and for each of its A actions the
// mean rollout runs 1 + L steps from that leaf -- action a first, then L given random actions -- with the reward head on every step.
// Three launches on one stream, nothing synchronised:
//   plan_prep_k    gathers the leaf states by index and writes the per-step [action embedding | appearance] rows the rollout reads
//                  (column `action` of the embedding Linear plus its bias -- no one-hot, no tiled copies, no embedding GEMM),
//   the rollout launcher of the model's state-code length cl (stove_rollout_fwd at cl = 32: the kernels of gnn_small.hip / gnn.hip;
//                  stove_rollout_fwd_cl at cl = 16 / 64: gnn_cl.hip -- as they are),
//   plan_finish_k  reward head per step without saved activations, q in a fixed summation order, child states scattered to the pool.
// Everything is cl wide where it was 32: states N (cl/2 + 2) floats, pred rows cl, the reward head cl-cl-cl / cl-cl/2-cl/4-1.
// Indices live on the device: a tree with an index out of range (leaf, child range, len_s, any of its A L actions) is flagged by
// plan_prep_k, rolls out a zero state instead of reading the pool, gets NaN in its q / reward rows and writes no pool slot.
// The reward head's parameter layout and dots are reward_head.h's (RhCl, rh_dot_t), the embedding of one action is ppo_model_step.h's
// pm_embed; plan_finish_k's forward is reward_head_fwd_k's arithmetic in its own text, as are the imagined collections'
// (ppo_model.hip, ppo_model_cl.hip), and the tests hold them all to one another bit for bit.
#include "common.h"
#include "ppo_model_step.h"
#include "reward_head.h"

namespace stove {

constexpr int kPlanPrepThreads = 256;

// ok[m] = 1 where every index of tree m is in range.  z_in (M A, N, zw), extra (M A, 1 + L, N, 4 + app_dim); zw = cl/2 + 2
__global__ __launch_bounds__(kPlanPrepThreads) void plan_prep_k(const float* __restrict__ z_pool, const int* __restrict__ leaf,
                                                                const int* __restrict__ child, const int* __restrict__ len_s,
                                                                const float* __restrict__ app, const int* __restrict__ acts,
                                                                const float* __restrict__ emb_w, const float* __restrict__ emb_b,
                                                                float* __restrict__ z_in, float* __restrict__ extra, int* __restrict__ ok,
                                                                int cap, int A, int L, int D, int N, int app_dim, int zw) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int lf = leaf[m], ch = child[m], ls = len_s[m];
  const int* am = acts + (size_t)m * A * L;
  int bad = lf < 0 || lf >= cap || ch < 0 || ch > cap - A || ls < 1 || ls > D;
  for (int i = tid; i < A * L; i += kPlanPrepThreads) bad |= am[i] < 0 || am[i] >= A;
  bad = __syncthreads_or(bad);
  if (tid == 0) ok[m] = !bad;
  const int zrow = N * zw;
  const float* zl = z_pool + ((size_t)m * cap + (bad ? 0 : lf)) * zrow;
  float* zo = z_in + (size_t)m * A * zrow;
  for (int i = tid; i < A * zrow; i += kPlanPrepThreads) zo[i] = bad ? 0.0f : zl[i % zrow];
  const int E = 4 + app_dim, steps = 1 + L;
  float* eo = extra + (size_t)m * A * steps * N * E;
  for (int i = tid; i < A * steps * N * E; i += kPlanPrepThreads) {
    const int e = i % E, r = (i / E) % N, t = (i / (E * N)) % steps, a = i / (E * N * steps);
    float v = 0.0f;
    if (!bad) {
      if (e < 4) {
        v = pm_embed(emb_w, emb_b, r * 4 + e, t == 0 ? a : am[a * L + t - 1], A);
      } else {
        v = app[((size_t)m * N + r) * app_dim + (e - 4)];
      }
    }
    eo[i] = v;
  }
}

// pred (M A, 1 + L, N, CL), z_pred (M A, 1 + L, N, CL/2 + 2) of the rollout -> q (M, A), r_first (M, A), r_roll (M, A, L) (the last two
// may be NULL) and the state after step 0 of row (m, a) into z_pool[m, child[m] + a].  reward_head_fwd_k's arithmetic, nothing saved:
//   head0 = Linear(CL, CL) - ReLU - Linear(CL, CL) summed over the objects, head1 = Linear(CL, CL/2) - ReLU - Linear(CL/2, CL/4) - ReLU
//   - Linear(CL/4, 1), sigmoid;
//   q = (r0 - 1) gamma^len_s + (sum_{k < min(2 D - len_s + 1, L)} (r_k - 1)) (sum_{j = len_s}^{D - 1} gamma^j)
// (the reference's broadcast product of the two sums; the second one is empty, 0, at len_s = D).  One wave per row, lane l < CL holds
// element l (the lanes from CL up repeat lane l - CL's arithmetic and write nothing); sums in step order.  The weights are staged
// transposed once per workgroup: 42 KiB of LDS at CL = 64.
template <int CL>
__global__ __launch_bounds__(64 * kRhWaves) void plan_finish_k(const float* __restrict__ pred, const float* __restrict__ z_pred,
                                                               const float* __restrict__ P, const int* __restrict__ ok,
                                                               const int* __restrict__ child, const int* __restrict__ len_s,
                                                               float* __restrict__ z_pool, float* __restrict__ q, float* __restrict__ r_first,
                                                               float* __restrict__ r_roll, int rows, int cap, int A, int L, int D, int N,
                                                               float gamma) {
  using R = RhCl<CL>;
  constexpr int H1 = R::H1, H2 = R::H2;
  static_assert(CL == 16 || CL == 32 || CL == 64, "one wave holds a CL-wide vector; rh_dot_t takes K in fours");
  __shared__ __attribute__((aligned(16))) float Wt0a[CL * CL], Wt0b[CL * CL], Wt1a[CL * H1], Wt1b[H1 * H2], V[CL + CL + H1 + H2 + H2 + 4],
      xs[kRhWaves][CL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & (CL - 1);
  for (int i = tid; i < CL * CL; i += blockDim.x) {
    const int o = i / CL, k = i % CL;                    // W (out o, in k) -> Wt[k][o]
    Wt0a[k * CL + o] = P[R::W0A + i];
    Wt0b[k * CL + o] = P[R::W0B + i];
  }
  for (int i = tid; i < H1 * CL; i += blockDim.x) Wt1a[(i % CL) * H1 + i / CL] = P[R::W1A + i];
  for (int i = tid; i < H2 * H1; i += blockDim.x) Wt1b[(i % H1) * H2 + i / H1] = P[R::W1B + i];
  float* b0a = V; float* b0b = V + CL; float* b1a = V + 2 * CL; float* b1b = b1a + H1; float* w1c = b1b + H2; float* b1c = w1c + H2;
  for (int i = tid; i < CL; i += blockDim.x) { b0a[i] = P[R::B0A + i]; b0b[i] = P[R::B0B + i]; }
  for (int i = tid; i < H1; i += blockDim.x) b1a[i] = P[R::B1A + i];
  for (int i = tid; i < H2; i += blockDim.x) { b1b[i] = P[R::B1B + i]; w1c[i] = P[R::W1C + i]; }
  if (tid == 0) b1c[0] = P[R::B1C];
  __syncthreads();
  float* x = xs[wv];
  const bool act = lane < CL;
  const int steps = 1 + L, zrow = N * (CL / 2 + 2);
  const float nan = __int_as_float(0x7fc00000);
  for (int row = blockIdx.x * kRhWaves + wv; row < rows; row += gridDim.x * kRhWaves) {
    const int m = row / A, a = row - m * A;
    if (!ok[m]) {          // (the same for the whole wave)
      if (lane == 0) {
        q[row] = nan;
        if (r_first != nullptr) r_first[row] = nan;
      }
      if (r_roll != nullptr)
        for (int k = lane; k < L; k += 64) r_roll[(size_t)row * L + k] = nan;
      continue;
    }
    const int ls = len_s[m];
    const int counted = min(2 * D - ls + 1, L);
    float r0 = 0.0f, s1 = 0.0f;
    for (int t = 0; t < steps; ++t) {
      const size_t it = (size_t)row * steps + t;
      float hsum = 0.0f;
      for (int o = 0; o < N; ++o) {
        const size_t prow = (it * N + o) * CL;
        if (act) x[l] = pred[prow + l];
        float h = b0a[l] + rh_dot_t<CL, CL>(Wt0a, x, l);
        h = fmaxf(h, 0.0f);
        if (act) x[l] = h;
        hsum += b0b[l] + rh_dot_t<CL, CL>(Wt0b, x, l);
      }
      if (act) x[l] = hsum;
      const float a1 = fmaxf(b1a[l & (H1 - 1)] + rh_dot_t<CL, H1>(Wt1a, x, l), 0.0f);
      if (lane < H1) x[l] = a1;
      const float a2 = fmaxf(b1b[l & (H2 - 1)] + rh_dot_t<H1, H2>(Wt1b, x, l), 0.0f);
      if (lane < H2) x[l] = a2;
      float z = b1c[0];
#pragma unroll
      for (int k = 0; k < H2; ++k) z = fmaf(w1c[k], x[k], z);
      const float r = 1.0f / (1.0f + expf(-z));
      if (t == 0) {
        r0 = r;
        if (lane == 0 && r_first != nullptr) r_first[row] = r;
      } else {
        if (t - 1 < counted) s1 += r - 1.0f;
        if (lane == 0 && r_roll != nullptr) r_roll[(size_t)row * L + t - 1] = r;
      }
    }
    if (lane == 0) {
      float g = 1.0f;
      for (int j = 0; j < ls; ++j) g *= gamma;
      const float first = (r0 - 1.0f) * g;
      float s2 = 0.0f;
      for (int j = ls; j < D; ++j) {
        s2 += g;
        g *= gamma;
      }
      q[row] = fmaf(s1, s2, first);
    }
    const float* zs = z_pred + (size_t)row * steps * zrow;         // step 0
    float* zd = z_pool + ((size_t)m * cap + child[m] + a) * zrow;
    for (int i = lane; i < zrow; i += 64) zd[i] = zs[i];
  }
}

}  // namespace stove
