// The PPO update on the device (stove_ppo_update, capi.hip): every epoch and mini-batch, E x M dependent optimiser steps, in ONE
// launch of ONE workgroup of 1024 lanes.  The arithmetic is csrc/ppo_update.h's, the text the CPU driver runs.  The steps are a serial
// chain and each needs a reduction over all rows and all parameters; __syncthreads() is the only synchronisation used -- no traffic
// between workgroups, no grid barrier, no spin, no atomics, plain vector stores only.
//
// Per step, in tiles of kUpdTile rows (a wave per row): gather the tile's rows through perm; forward with a neuron per lane, the
// activations kept in the tile's LDS rows (ppo_update.h describes a row); the heads of the tile's rows on a lane each, the loss terms summed
// in row order by thread 0; backward through the layers with an input entry per lane, its sum over j ascending; then the weight and
// bias gradients: one lane owns one parameter entry (entry `local` of layer l on lane local % 1024) and carries its float32 sum over
// the rows, ascending, in a register across the tiles.  After the last tile: the squared norm in float64 (the lane's entries in
// order, a wave reduction in a fixed pattern, the sixteen waves in order), the clip coefficient, Adam on the lane's entries.
// kStaged: the image lives in LDS beside the tile, each transposed weight with an odd row stride so that the backward's lanes (one
// weight row each) fall on different banks, and is written back once at the end; otherwise it stays in global memory, is read
// through the cache and is updated in place.  m and v stay in global memory: only their owning lane ever touches an entry.
// Every lane walks the same steps and tiles and meets every barrier; the decision to stop is read from LDS by all of them.
#include "common.h"
#include "ppo_update.h"

namespace stove {

constexpr int kUpdWaves = 16, kUpdThreads = kUpdWaves * kWave, kUpdTile = kUpdWaves;
constexpr int kUpdHeadDoubles = 2 * ppo_policy::kActions;            // head_row's working room, per row of the tile
// the tile's row terms, the waves' partial norms, the step's scalars, the heads' working room
// and the layer table: per layer in, out, the image's row stride, entries, the row's input and derivative offsets, the image's offset
// as the forward reads it and in global memory (read from LDS where needed, so that none of it is held in registers across the step)
constexpr int kUpdTabInts = 8, kUpdTabDoubles = ppo_policy::kMaxLayers * kUpdTabInts / 2;
constexpr int kUpdScalDoubles = 3 * kUpdTile + kUpdWaves + 8 + kUpdTile * kUpdHeadDoubles + kUpdTabDoubles;
enum { kTabK, kTabJ, kTabJp, kTabCount, kTabAct, kTabDelta, kTabImg, kTabOff };
constexpr size_t kUpdLdsLimit = 160 * 1024;
// gradient entries per lane and layer at the widest shape: (4 * 6 + 1) * 128, 129 * 32, 33 * 128, 129 * 128 (twice), 129 * 10 over 1024 lanes
constexpr int kUpdSlots0 = 4, kUpdSlots1 = 5, kUpdSlots2 = 5, kUpdSlotsMid = 17, kUpdSlotsHeads = 2;
static_assert((4 * env_step::kMaxObjects + 1) * ppo_policy::kBase0 <= kUpdSlots0 * kUpdThreads, "layer 0 fits its slots");
static_assert((ppo_policy::kBase0 + 1) * ppo_policy::kBase1 <= kUpdSlots1 * kUpdThreads, "layer 1 fits its slots");
static_assert((ppo_policy::kBase1 + 1) * ppo_policy::kMaxHidden <= kUpdSlots2 * kUpdThreads, "layer 2 fits its slots");
static_assert((ppo_policy::kMaxHidden + 1) * ppo_policy::kMaxHidden <= kUpdSlotsMid * kUpdThreads, "the deep layers fit their slots");
static_assert((ppo_policy::kMaxHidden + 1) * ppo_policy::kHeads <= kUpdSlotsHeads * kUpdThreads, "the heads fit their slots");

// the row stride of a transposed weight in the staged image: odd
__host__ __device__ inline int upd_stride(int J, bool staged) { return staged ? (J | 1) : J; }
__host__ __device__ inline size_t upd_image_offset(const ppo_policy::Shape& s, int l, bool staged) {
  if (!staged) return ppo_policy::offset(s, l);
  size_t o = 0;
  for (int k = 0; k < l; ++k) o += (size_t)(ppo_policy::width_in(s, k) + 1) * (size_t)upd_stride(ppo_policy::width_out(s, k), true);
  return o;
}
inline size_t upd_tile_bytes(const ppo_policy::Shape& s) {
  return kUpdScalDoubles * sizeof(double) + (size_t)kUpdTile * ppo_update::row_floats(s) * sizeof(float);
}
// the image is staged when it fits beside the tile (ppo_staged's test)
inline bool upd_staged(const ppo_policy::Shape& s) {
  return upd_tile_bytes(s) + upd_image_offset(s, ppo_policy::layers(s), true) * sizeof(float) <= kUpdLdsLimit;
}
inline size_t upd_lds_bytes(const ppo_policy::Shape& s) {
  return upd_tile_bytes(s) + (upd_staged(s) ? upd_image_offset(s, ppo_policy::layers(s), true) * sizeof(float) : 0);
}

// where the lane's entries of a layer (out = J) start and how they advance: entry local = tid + 1024 i is (k, j) = (local / J, local % J)
struct UpdWalk {
  int k0, j0, qk, qj;
};
__device__ __forceinline__ UpdWalk upd_walk(int J) {
  const int tid = (int)threadIdx.x;
  return UpdWalk{tid / J, tid % J, kUpdThreads / J, kUpdThreads % J};
}

// the tile's rows added to the lane's gradient entries of one layer: entry after entry, each over the rows in ascending order
template <int kS>
__device__ __forceinline__ void upd_grad_tile(float (&g)[kS], const float* rows, int stride, int n_rows, const int* tab) {
  const int J = tab[kTabJ], count = tab[kTabCount], a_off = tab[kTabAct], d_off = tab[kTabDelta];
  const UpdWalk w = upd_walk(J);
  const int tid = (int)threadIdx.x;
  int k = w.k0, j = w.j0;
#pragma unroll
  for (int i = 0; i < kS; ++i) {
    if (kUpdThreads * i >= count) break;          // (the same for every lane)
    if (tid + kUpdThreads * i < count) {
      const float *a = rows + a_off + k, *d = rows + d_off + j;
      g[i] = ppo_update::grad_rows(g[i], a, d, (size_t)stride, n_rows);
    }
    k += w.qk;
    j += w.qj;
    if (j >= J) {
      j -= J;
      ++k;
    }
  }
}

template <int kS>
__device__ __forceinline__ double upd_square(const float (&g)[kS], const int* tab, double sq) {
  const int count = tab[kTabCount];
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int i = 0; i < kS; ++i)
    if (tid + kUpdThreads * i < count) sq = sq + (double)g[i] * (double)g[i];
  return sq;
}

// Adam on the lane's entries of one layer: img / stride the image the forward reads (LDS or global), m, v at the layer's global offset
template <int kS>
__device__ __forceinline__ void upd_adam(const float (&g)[kS], float* image, float* m_all, float* v_all, const int* tab, float coef,
                                         const ppo_update::AdamStep& a, float eps) {
  const int J = tab[kTabJ], count = tab[kTabCount], stride = tab[kTabJp];
  float *img = image + tab[kTabImg], *m = m_all + tab[kTabOff], *v = v_all + tab[kTabOff];
  const UpdWalk w = upd_walk(J);
  const int tid = (int)threadIdx.x;
  int k = w.k0, j = w.j0;
#pragma unroll
  for (int i = 0; i < kS; ++i) {
    const int local = tid + kUpdThreads * i;
    if (local < count) {
      float mm = m[local], vv = v[local];
      float* p = img + (size_t)k * stride + j;
      *p = ppo_update::adam_entry(*p, g[i], coef, &mm, &vv, a, eps);
      m[local] = mm;
      v[local] = vv;
    }
    k += w.qk;
    j += w.qj;
    if (j >= J) {
      j -= J;
      ++k;
    }
  }
}

template <int kS>
__device__ __forceinline__ void upd_zero(float (&g)[kS]) {
#pragma unroll
  for (int i = 0; i < kS; ++i) g[i] = 0.0f;
}

// the sum of a double over the wave's lanes in a fixed pattern (xor butterflies), the same in every lane
__device__ __forceinline__ double upd_wave_sum(double x) {
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, kWave);
  return x;
}

// grid 1, block kUpdThreads, dynamic LDS upd_lds_bytes.  params, m, v: the image and Adam's moments (n_params floats) in/out; step (1,)
// in/out; obs (n, 4N); actions, returns, values, logp, adv (n,); perm (E, n); losses (E * M, 3); gnorm (E * M,); status (2,).
template <bool kStaged, bool kDeep>
__global__ __launch_bounds__(kUpdThreads) void ppo_update_k(float* params, float* m, float* v, int* step, const float* __restrict__ obs,
                                                            const int* __restrict__ actions, const float* __restrict__ returns,
                                                            const float* __restrict__ values, const float* __restrict__ logp,
                                                            const float* __restrict__ adv, const int* __restrict__ perm, float* losses,
                                                            float* gnorm, int* status, ppo_policy::Shape sh, ppo_update::Hyper hy, int n,
                                                            int M, int max_steps) {
  extern __shared__ __attribute__((aligned(16))) double upd_lds[];
  const int tid = (int)threadIdx.x, w = wave_id(), lane = lane_id();
  double* terms = upd_lds;                          // (kUpdTile, 3)
  double* wsum = terms + 3 * kUpdTile;              // (kUpdWaves,)
  double* scal = wsum + kUpdWaves;                  // value, action, entropy, norm; [4] the bad-index flag; [5], [6] Adam's step scalars
  float* rows = reinterpret_cast<float*>(upd_lds + kUpdScalDoubles);
  int* tab = reinterpret_cast<int*>(scal + 8 + kUpdTile * kUpdHeadDoubles);
  const int L = ppo_policy::layers(sh), W = 4 * sh.N, stride = ppo_update::row_floats(sh), mb = n / M;
  float* img = kStaged ? rows + (size_t)kUpdTile * stride : params;
  if (tid < L) {
    int* t = tab + tid * kUpdTabInts;
    t[kTabK] = ppo_policy::width_in(sh, tid);
    t[kTabJ] = ppo_policy::width_out(sh, tid);
    t[kTabJp] = upd_stride(ppo_policy::width_out(sh, tid), kStaged);
    t[kTabCount] = ppo_update::entries(sh, tid);
    t[kTabAct] = ppo_update::act_offset(sh, tid);
    t[kTabDelta] = ppo_update::delta_offset(sh, tid);
    t[kTabImg] = (int)upd_image_offset(sh, tid, kStaged);
    t[kTabOff] = (int)ppo_policy::offset(sh, tid);
  }
  __syncthreads();
  if (kStaged) {
    for (int l = 0; l < L; ++l) {
      const int* t = tab + l * kUpdTabInts;
      const int J = t[kTabJ], Jp = t[kTabJp], count = t[kTabCount];
      const float* src = params + t[kTabOff];
      float* dst = img + t[kTabImg];
      for (int e = tid; e < count; e += kUpdThreads) dst[(size_t)(e / J) * Jp + e % J] = src[e];
    }
  }
  const int step0 = step[0];
  float* row = rows + (size_t)w * stride;
  float g0[kUpdSlots0], g1[kUpdSlots1], g2[kUpdSlots2], g3[kDeep ? kUpdSlotsMid : 1], g4[kDeep ? kUpdSlotsMid : 1], g5[kUpdSlotsHeads];
  int done = 0, code = ppo_update::kOk;
  __syncthreads();
  for (int at = 0; at < max_steps; ++at) {
    const int* sel = perm + (size_t)(at / M) * n + (size_t)(at % M) * mb;
    // ---- the step's indices
    if (tid == 0) scal[4] = 0.0;
    __syncthreads();
    for (int r = tid; r < mb; r += kUpdThreads) {
      const int i = sel[r];
      bool bad = i < 0 || i >= n;
      if (!bad) bad = actions[i] < 0 || actions[i] >= ppo_policy::kActions;
      if (bad) scal[4] = 1.0;
    }
    __syncthreads();
    if (scal[4] != 0.0) {
      code = ppo_update::kBadIndex;
      break;
    }
    upd_zero(g0);
    upd_zero(g1);
    upd_zero(g2);
    upd_zero(g3);
    upd_zero(g4);
    upd_zero(g5);
    double value = 0.0, action = 0.0, entropy = 0.0;          // (thread 0's)
    for (int base = 0; base < mb; base += kUpdTile) {
      const int n_rows = mb - base < kUpdTile ? mb - base : kUpdTile;
      const bool live = w < n_rows;
      const int i = live ? sel[base + w] : 0;
      // ---- gather and forward
      if (live) {
        if (lane < W) row[lane] = obs[(size_t)i * W + lane];
        if (lane == 0) row[W] = 1.0f;
      }
      __syncthreads();
      for (int l = 0; l < L; ++l) {
        const int* t = tab + l * kUpdTabInts;
        const int K = t[kTabK], J = t[kTabJ], Jp = t[kTabJp];
        const float* wT = img + t[kTabImg];
        const float* in = row + t[kTabAct];
        float* out = row + (l == L - 1 ? t[kTabDelta] : t[kUpdTabInts + kTabAct]);
        if (live) {
          for (int j = lane; j < J; j += kWave) out[j] = ppo_update::neuron(wT, wT + (size_t)K * Jp, in, K, (size_t)Jp, j, l != L - 1);
          if (l != L - 1 && lane == 0) out[J] = 1.0f;
        }
        __syncthreads();
      }
      // ---- the head of each row: a lane per row (one pass of that long text serves the whole tile)
      if (tid < n_rows) {
        const int ir = sel[base + tid];
        const ppo_update::RowTerms t = ppo_update::head_row(rows + (size_t)tid * stride + tab[(L - 1) * kUpdTabInts + kTabDelta], actions[ir], returns[ir],
                                                            values[ir], logp[ir], adv[ir], hy, mb, scal + 8 + tid * kUpdHeadDoubles);
        terms[3 * tid] = t.value;
        terms[3 * tid + 1] = t.action;
        terms[3 * tid + 2] = t.entropy;
      }
      __syncthreads();
      if (tid == 0)
        for (int r = 0; r < n_rows; ++r) {
          value = value + terms[3 * r];
          action = action + terms[3 * r + 1];
          entropy = entropy + terms[3 * r + 2];
        }
      // ---- backward
      for (int l = L - 1; l >= 1; --l) {
        const int* t = tab + l * kUpdTabInts;
        const int K = t[kTabK], J = t[kTabJ], Jp = t[kTabJp];
        const float* wT = img + t[kTabImg];
        const float* act = row + t[kTabAct];
        const float* delta = row + t[kTabDelta];
        float* below = row + t[kTabDelta - kUpdTabInts];
        if (live)
          for (int k = lane; k < K; k += kWave) below[k] = ppo_update::back_entry(wT, (size_t)Jp, delta, J, k, act[k]);
        __syncthreads();
      }
      // ---- the gradients: the tile's rows onto the lane's entries
      upd_grad_tile(g0, rows, stride, n_rows, tab);
      upd_grad_tile(g1, rows, stride, n_rows, tab + kUpdTabInts);
      upd_grad_tile(g2, rows, stride, n_rows, tab + 2 * kUpdTabInts);
      if (kDeep) {
        upd_grad_tile(g3, rows, stride, n_rows, tab + 3 * kUpdTabInts);
        upd_grad_tile(g4, rows, stride, n_rows, tab + 4 * kUpdTabInts);
      }
      upd_grad_tile(g5, rows, stride, n_rows, tab + (L - 1) * kUpdTabInts);
      __syncthreads();
    }
    // ---- the norm and the step's scalars
    double sq = upd_square(g0, tab, 0.0);
    sq = upd_square(g1, tab + kUpdTabInts, sq);
    sq = upd_square(g2, tab + 2 * kUpdTabInts, sq);
    if (kDeep) {
      sq = upd_square(g3, tab + 3 * kUpdTabInts, sq);
      sq = upd_square(g4, tab + 4 * kUpdTabInts, sq);
    }
    sq = upd_square(g5, tab + (L - 1) * kUpdTabInts, sq);
    sq = upd_wave_sum(sq);
    if (lane == 0) wsum[w] = sq;
    __syncthreads();
    if (tid == 0) {
      double total = 0.0;
      for (int k = 0; k < kUpdWaves; ++k) total = total + wsum[k];
      scal[0] = value / (double)mb;
      scal[1] = action / (double)mb;
      scal[2] = entropy / (double)mb;
      scal[3] = sqrt(total);
      const ppo_update::AdamStep a = ppo_update::adam_step(step0 + at + 1, hy.lr);
      scal[5] = a.step_size;
      scal[6] = a.root_bias2;
    }
    __syncthreads();
    const double norm = scal[3];
    if (!ppo_update::finite(scal[0]) || !ppo_update::finite(scal[1]) || !ppo_update::finite(scal[2]) || !ppo_update::finite(norm)) {
      code = ppo_update::kNonFinite;
      break;
    }
    // ---- Adam
    const float coef = (float)ppo_update::clip_coef(norm, hy.max_grad_norm);
    const ppo_update::AdamStep a{scal[5], scal[6]};
    upd_adam(g0, img, m, v, tab, coef, a, hy.eps);
    upd_adam(g1, img, m, v, tab + kUpdTabInts, coef, a, hy.eps);
    upd_adam(g2, img, m, v, tab + 2 * kUpdTabInts, coef, a, hy.eps);
    if (kDeep) {
      upd_adam(g3, img, m, v, tab + 3 * kUpdTabInts, coef, a, hy.eps);
      upd_adam(g4, img, m, v, tab + 4 * kUpdTabInts, coef, a, hy.eps);
    }
    upd_adam(g5, img, m, v, tab + (L - 1) * kUpdTabInts, coef, a, hy.eps);
    if (tid == 0) {
      losses[(size_t)at * 3] = (float)scal[0];
      losses[(size_t)at * 3 + 1] = (float)scal[1];
      losses[(size_t)at * 3 + 2] = (float)scal[2];
      gnorm[at] = (float)norm;
    }
    done = at + 1;
    __syncthreads();
  }
  __syncthreads();
  if (kStaged && done > 0) {
    for (int l = 0; l < L; ++l) {
      const int* t = tab + l * kUpdTabInts;
      const int J = t[kTabJ], Jp = t[kTabJp], count = t[kTabCount];
      float* dst = params + t[kTabOff];
      const float* src = img + t[kTabImg];
      for (int e = tid; e < count; e += kUpdThreads) dst[e] = src[(size_t)(e / J) * Jp + e % J];
    }
  }
  if (tid == 0) {
    step[0] = step0 + done;
    status[0] = code;
    status[1] = done;
  }
}

}  // namespace stove
