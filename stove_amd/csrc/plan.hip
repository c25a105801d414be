// One expansion of a batch of search trees on the learned model (reference mcts_stove.py:95-137 and the value arithmetic of
// MCTS.backpropagate, :186-196): every tree m hands over the pool slot of the leaf it selected, and for each of its A actions the
// mean rollout runs 1 + L steps from that leaf -- action a first, then L given random actions -- with the reward head on every step.
// Three launches on one stream, nothing synchronised:
//   plan_prep_k    gathers the leaf states by index and writes the per-step [action embedding | appearance] rows the rollout reads
//                  (column `action` of the embedding Linear plus its bias -- no one-hot, no tiled copies, no embedding GEMM),
//   the cl = 32 rollout launcher (stove_rollout_fwd: the kernels of gnn_small.hip / gnn.hip as they are),
//   plan_finish_k  reward head per step without saved activations, q in a fixed summation order, child states scattered to the pool.
// Indices live on the device: a tree with an index out of range (leaf, child range, len_s, any of its A L actions) is flagged by
// plan_prep_k, rolls out a zero state instead of reading the pool, gets NaN in its q / reward rows and writes no pool slot.
#include "common.h"

namespace stove {

constexpr int kPlanPrepThreads = 256;

// ok[m] = 1 where every index of tree m is in range.  z_in (M A, N, 18), extra (M A, 1 + L, N, 4 + app_dim)
__global__ __launch_bounds__(kPlanPrepThreads) void plan_prep_k(const float* __restrict__ z_pool, const int* __restrict__ leaf,
                                                                const int* __restrict__ child, const int* __restrict__ len_s,
                                                                const float* __restrict__ app, const int* __restrict__ acts,
                                                                const float* __restrict__ emb_w, const float* __restrict__ emb_b,
                                                                float* __restrict__ z_in, float* __restrict__ extra, int* __restrict__ ok,
                                                                int cap, int A, int L, int D, int N, int app_dim) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int lf = leaf[m], ch = child[m], ls = len_s[m];
  const int* am = acts + (size_t)m * A * L;
  int bad = lf < 0 || lf >= cap || ch < 0 || ch > cap - A || ls < 1 || ls > D;
  for (int i = tid; i < A * L; i += kPlanPrepThreads) bad |= am[i] < 0 || am[i] >= A;
  bad = __syncthreads_or(bad);
  if (tid == 0) ok[m] = !bad;
  const int zrow = N * 18;
  const float* zl = z_pool + ((size_t)m * cap + (bad ? 0 : lf)) * zrow;
  float* zo = z_in + (size_t)m * A * zrow;
  for (int i = tid; i < A * zrow; i += kPlanPrepThreads) zo[i] = bad ? 0.0f : zl[i % zrow];
  const int E = 4 + app_dim, steps = 1 + L;
  float* eo = extra + (size_t)m * A * steps * N * E;
  for (int i = tid; i < A * steps * N * E; i += kPlanPrepThreads) {
    const int e = i % E, r = (i / E) % N, t = (i / (E * N)) % steps, a = i / (E * N * steps);
    float v = 0.0f;
    if (!bad) {
      if (e < 4) {        // the embedding Linear on a one-hot row, in small_linear_k's order of operations (the same bits)
        const int act = t == 0 ? a : am[a * L + t - 1], o = r * 4 + e;
        v = emb_b[o];
        for (int k = 0; k < A; ++k) v = fmaf(k == act ? 1.0f : 0.0f, emb_w[(size_t)o * A + k], v);
      } else {
        v = app[((size_t)m * N + r) * app_dim + (e - 4)];
      }
    }
    eo[i] = v;
  }
}

// pred (M A, 1 + L, N, 32), z_pred (M A, 1 + L, N, 18) of the rollout -> q (M, A), r_first (M, A), r_roll (M, A, L) (the last two may
// be NULL) and the state after step 0 of row (m, a) into z_pool[m, child[m] + a].  reward_head_fwd_k's arithmetic, nothing saved.
//   q = (r0 - 1) gamma^len_s + (sum_{k < min(2 D - len_s + 1, L)} (r_k - 1)) (sum_{j = len_s}^{D - 1} gamma^j)
// (the reference's broadcast product of the two sums; the second one is empty, 0, at len_s = D).  One wave per row, sums in step order.
__global__ __launch_bounds__(64 * kRhWaves) void plan_finish_k(const float* __restrict__ pred, const float* __restrict__ z_pred,
                                                               const float* __restrict__ P, const int* __restrict__ ok,
                                                               const int* __restrict__ child, const int* __restrict__ len_s,
                                                               float* __restrict__ z_pool, float* __restrict__ q, float* __restrict__ r_first,
                                                               float* __restrict__ r_roll, int rows, int cap, int A, int L, int D, int N,
                                                               float gamma) {
  __shared__ __attribute__((aligned(16))) float Wt0a[1024], Wt0b[1024], Wt1a[512], Wt1b[128], V[32 + 32 + 16 + 8 + 8 + 4], xs[kRhWaves][32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & 31;
  for (int i = tid; i < 1024; i += blockDim.x) {
    const int o = i >> 5, k = i & 31;                    // W (out o, in k) -> Wt[k][o]
    Wt0a[k * 32 + o] = P[RH_W0A + i];
    Wt0b[k * 32 + o] = P[RH_W0B + i];
  }
  for (int i = tid; i < 512; i += blockDim.x) Wt1a[(i & 31) * 16 + (i >> 5)] = P[RH_W1A + i];
  for (int i = tid; i < 128; i += blockDim.x) Wt1b[(i & 15) * 8 + (i >> 4)] = P[RH_W1B + i];
  float* b0a = V; float* b0b = V + 32; float* b1a = V + 64; float* b1b = V + 80; float* w1c = V + 88; float* b1c = V + 96;
  for (int i = tid; i < 32; i += blockDim.x) { b0a[i] = P[RH_B0A + i]; b0b[i] = P[RH_B0B + i]; }
  for (int i = tid; i < 16; i += blockDim.x) b1a[i] = P[RH_B1A + i];
  for (int i = tid; i < 8; i += blockDim.x) { b1b[i] = P[RH_B1B + i]; w1c[i] = P[RH_W1C + i]; }
  if (tid == 0) b1c[0] = P[RH_B1C];
  __syncthreads();
  float* x = xs[wv];
  const bool act = lane < 32;
  const int steps = 1 + L, zrow = N * 18;
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
      float h32 = 0.0f;
      for (int o = 0; o < N; ++o) {
        const size_t prow = (it * N + o) * 32;
        if (act) x[l] = pred[prow + l];
        float h = b0a[l] + rh_dot_t<32, 32>(Wt0a, x, l);
        h = fmaxf(h, 0.0f);
        if (act) x[l] = h;
        h32 += b0b[l] + rh_dot_t<32, 32>(Wt0b, x, l);
      }
      if (act) x[l] = h32;
      const float a1 = fmaxf(b1a[l & 15] + rh_dot_t<32, 16>(Wt1a, x, l), 0.0f);
      if (lane < 16) x[l] = a1;
      const float a2 = fmaxf(b1b[l & 7] + rh_dot_t<16, 8>(Wt1b, x, l), 0.0f);
      if (lane < 8) x[l] = a2;
      float z = b1c[0];
#pragma unroll
      for (int k = 0; k < 8; ++k) z = fmaf(w1c[k], x[k], z);
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
