// The PPO update of the IMAGE policy on the device (stove_ppo_update_images, capi.hip): every epoch and mini-batch of
// PPOAgent.update for Policy((32, 32, 3F), 9) -- ppo_image.h describes the network and its parameter image -- as a fixed chain of
// launches per optimiser step on one stream.  The heads, the losses, the clip coefficient and Adam are ppo_update.h's text.
//
// One step on the mb rows the step's slice of perm names (row r of the step is sample i = perm[...][r]; its observation is the
// 3072 F contiguous floats at obs + (i / S) env_stride + (i % S) 3072, divided by 255 as they are read):
//   piu_check_k         the slice's indices and actions; one out of range sets status 2
//   forward             conv1, conv2, head.main [, the two deep layers]: each ONE product on the matrix cores (piu_gemm_k below), the
//                       bias and the ReLU in its epilogue, the activations kept in the workspace
//   piu_heads_k         value and logits (float32 FMAs, sixteen interleaved partial sums per output), head_row per row (its float64 terms to the workspace, the
//                       derivative by the ten outputs in place), and the derivative by the last hidden layer
//   backward            through the deep layers, head.main and conv2 down to conv1's outputs, a product each, masked by the ReLU that
//                       produced the layer's input; conv1 needs no input gradient
//   weight gradients    a product with K = the rows (the linear layers) or K = the rows x output positions (the convolutions); the
//                       bias is the weight row after the last input, whose activation is 1.  The convolutions' K is split over
//                       workgroups into partial images in the workspace, which piu_reduce_k adds in a fixed order
//   piu_norm_k          per 4096 entries of the gradient image a float64 sum of squares
//   piu_finish_k        the partial norms and the rows' loss terms summed in float64, each in a fixed pattern; a loss or norm that is not
//                       finite sets status 3; else losses, gnorm, the clip coefficient and Adam's step scalars
//   piu_adam_k          adam_entry on every entry; its first thread counts the step
// Every kernel reads status[0] first and returns when it is set, so the failing step and all after it change nothing.
//
// The product (piu_gemm_k): C (M x N) = A (M x K) B (K x N) with A, B and the epilogue given by a small struct of index functions,
// so that no operand is ever materialised (the windows, the im2col patches and the transposes are address arithmetic).  A workgroup
// of W = 4 waves (16 for head.main's forward, whose K = 1568 is long and whose tiles are few) owns one 32 x 32 tile of C as 2 x 2 tiles
// of __builtin_amdgcn_mfma_f32_16x16x4f32; wave w takes the K steps s = w, w + W, ... (four k each) of the workgroup's K range, the W
// partial tiles meet in LDS and are added in ascending order of w.  Rows, columns and k outside the problem read as zero.  Every sum has a fixed order: no atomics, no
// arrival counters, nothing waits on another workgroup; the only synchronisation is __syncthreads() and the launch boundary.  Plain
// vector stores only.
#include "common.h"
#include "ppo_image.h"
#include "ppo_update.h"

namespace stove {

typedef float piu_f4 __attribute__((ext_vector_type(4)));
constexpr int kPiuThreads = 256, kPiuTile = 32, kPiuAhead = 4;
constexpr int kPiuC1 = ppo_image::kConv1Floats, kPiuC2 = ppo_image::kFlat, kPiuPos1 = 225, kPiuPos2 = 49;
constexpr int kPiuFrame = ppo_image::kFrameFloats;
constexpr int kPiuNormChunk = 4096;          // entries of the gradient image per partial norm
constexpr int kPiuSplitMin = 256, kPiuSplitMax = 256;          // a convolution's weight gradient: positions per partial, partials at most
constexpr int kPiuReduceWaves = 16;
constexpr int kPiuHeadRows = 16;            // rows per workgroup of piu_heads_k
enum { kPiuCoef, kPiuStepSize, kPiuRootBias2, kPiuT, kPiuScalars = 8 };

// how the K = rows x positions of a convolution's weight gradient are split: `count` partials of `chunk` positions (a multiple of 16)
struct PiuSplit {
  int count, chunk;
};
__host__ __device__ inline PiuSplit piu_split(long long K) {
  long long chunk = (K + kPiuSplitMax - 1) / kPiuSplitMax;
  if (chunk < kPiuSplitMin) chunk = kPiuSplitMin;
  chunk = (chunk + 15) / 16 * 16;
  return PiuSplit{(int)((K + chunk - 1) / chunk), (int)chunk};
}

// the workspace: doubles first, then floats; offsets in bytes
struct PiuWs {
  size_t scal, normpart, terms, c1, c2, h, dheads, dh, dc2, dc1, grad, part2, part1, bytes;
  int norm_blocks;
};
inline PiuWs piu_ws(int mb, const ppo_image::Shape& sh) {
  PiuWs w;
  const size_t P = ppo_image::param_floats(sh), r = (size_t)mb;
  w.norm_blocks = (int)((P + kPiuNormChunk - 1) / kPiuNormChunk);
  size_t at = 0;
  auto take = [&](size_t count, size_t size) {
    const size_t o = at;
    at += (count * size + 15) / 16 * 16;
    return o;
  };
  w.scal = take(kPiuScalars, 8);
  w.normpart = take((size_t)w.norm_blocks, 8);
  w.terms = take(3 * r, 8);
  w.c1 = take(r * kPiuC1, 4);
  w.c2 = take(r * kPiuC2, 4);
  w.h = take(3 * r * sh.H, 4);
  w.dheads = take(r * ppo_image::kHeads, 4);
  w.dh = take(3 * r * sh.H, 4);
  w.dc2 = take(r * kPiuC2, 4);
  w.dc1 = take(r * kPiuC1, 4);
  w.grad = take(P, 4);
  w.part2 = take((size_t)piu_split((long long)mb * kPiuPos2).count * 289 * 32, 4);
  w.part1 = take((size_t)piu_split((long long)mb * kPiuPos1).count * (48 * sh.F + 1) * 32, 4);
  w.bytes = at;
  return w;
}

// the step's rows and where their observations live
struct PiuRows {
  const float* obs;
  const int* sel;
  int S, env_stride;
  __device__ __forceinline__ const float* window(int r) const {
    const int i = sel[r];
    return obs + (size_t)(i / S) * (size_t)env_stride + (size_t)(i % S) * kPiuFrame;
  }
};

// ---------------------------------------------------------------------------------------------- the problems of piu_gemm_k
// a(m, k), b(k, n): the operands, called inside the problem only; put(m, n, v): the epilogue.  kMFast: m is the fast index of the
// stores (the convolutions' maps are position-major).
struct PiuConv1Fwd {          // c1[r][n][pos] = relu(bias[n] + sum_k window(r)[patch(pos, k)] / 255 * w[k][n])
  static constexpr bool kMFast = true;
  int M, N, K;
  PiuRows rows;
  const float* w;
  float* c1;
  __device__ __forceinline__ float a(int m, int k) const {
    const int r = m / kPiuPos1, pos = m - r * kPiuPos1, y = pos / 15, x = pos - y * 15;
    const int c = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
    return ppo_image::scaled(rows.window(r)[c * 1024 + (2 * y + ky) * 32 + 2 * x + kx]);
  }
  __device__ __forceinline__ float b(int k, int n) const { return w[k * 32 + n]; }
  __device__ __forceinline__ void put(int m, int n, float v) const {
    const int r = m / kPiuPos1, pos = m - r * kPiuPos1;
    c1[(size_t)r * kPiuC1 + n * kPiuPos1 + pos] = ppo_image::relu(v + w[K * 32 + n]);
  }
};
__device__ __forceinline__ int piu_patch2(int pos, int k) {          // conv2's input (c, 2y + ky, 2x + kx) of output position pos, in a row of c1
  const int y = pos / 7, x = pos - y * 7, c = k / 9, t = k - c * 9, ky = t / 3, kx = t - ky * 3;
  return c * kPiuPos1 + (2 * y + ky) * 15 + 2 * x + kx;
}
struct PiuConv2Fwd {
  static constexpr bool kMFast = true;
  int M, N, K;
  const float *c1, *w;
  float* c2;
  __device__ __forceinline__ float a(int m, int k) const {
    const int r = m / kPiuPos2, pos = m - r * kPiuPos2;
    return c1[(size_t)r * kPiuC1 + piu_patch2(pos, k)];
  }
  __device__ __forceinline__ float b(int k, int n) const { return w[k * 32 + n]; }
  __device__ __forceinline__ void put(int m, int n, float v) const {
    const int r = m / kPiuPos2, pos = m - r * kPiuPos2;
    c2[(size_t)r * kPiuC2 + n * kPiuPos2 + pos] = ppo_image::relu(v + w[K * 32 + n]);
  }
};
struct PiuFcFwd {          // out[m][n] = relu(bias[n] + sum_k in[m][k] w[k][n])
  static constexpr bool kMFast = false;
  int M, N, K;
  const float *in, *w;
  float* out;
  __device__ __forceinline__ float a(int m, int k) const { return in[(size_t)m * K + k]; }
  __device__ __forceinline__ float b(int k, int n) const { return w[(size_t)k * N + n]; }
  __device__ __forceinline__ void put(int m, int n, float v) const { out[(size_t)m * N + n] = ppo_image::relu(v + w[(size_t)K * N + n]); }
};
struct PiuFcBwd {          // din[m][n] = act[m][n] > 0 ? sum_j dout[m][j] w[n][j] : 0   (w the layer's transposed weight (N, K))
  static constexpr bool kMFast = false;
  int M, N, K;
  const float *dout, *w, *act;
  float* din;
  __device__ __forceinline__ float a(int m, int k) const { return dout[(size_t)m * K + k]; }
  __device__ __forceinline__ float b(int k, int n) const { return w[(size_t)n * K + k]; }
  __device__ __forceinline__ void put(int m, int n, float v) const {
    const size_t e = (size_t)m * N + n;
    din[e] = act[e] > 0.0f ? v : 0.0f;
  }
};
struct PiuConv2Bwd {          // dc1[r][c][y][x] = c1 > 0 ? sum over (ky, kx, o) of dc2[r][o][(y - ky) / 2][(x - kx) / 2] w2[(c, ky, kx)][o] : 0
  static constexpr bool kMFast = true;
  int M, N, K;          // K = 288 counted as (ky * 3 + kx) * 32 + o
  const float *dc2, *w, *c1;
  float* dc1;
  __device__ __forceinline__ float a(int m, int k) const {
    const int r = m / kPiuPos1, pos = m - r * kPiuPos1, y = pos / 15, x = pos - y * 15;
    const int o = k & 31, t = k >> 5, ky = t / 3, kx = t - ky * 3, yy = y - ky, xx = x - kx;
    if (yy < 0 || xx < 0 || ((yy | xx) & 1) != 0 || yy > 12 || xx > 12) return 0.0f;
    return dc2[(size_t)r * kPiuC2 + o * kPiuPos2 + (yy >> 1) * 7 + (xx >> 1)];
  }
  __device__ __forceinline__ float b(int k, int n) const { return w[(n * 9 + (k >> 5)) * 32 + (k & 31)]; }
  __device__ __forceinline__ void put(int m, int n, float v) const {
    const int r = m / kPiuPos1, pos = m - r * kPiuPos1;
    const size_t e = (size_t)r * kPiuC1 + n * kPiuPos1 + pos;
    dc1[e] = c1[e] > 0.0f ? v : 0.0f;
  }
};
struct PiuFcGrad {          // g[m][n] = sum_r act[r][m] delta[r][n], the bias at m == width: act = 1
  static constexpr bool kMFast = false;
  int M, N, K;          // M = width + 1, K = the rows
  const float *act, *delta;
  float* g;
  __device__ __forceinline__ float a(int m, int k) const { return m < M - 1 ? act[(size_t)k * (M - 1) + m] : 1.0f; }
  __device__ __forceinline__ float b(int k, int n) const { return delta[(size_t)k * N + n]; }
  __device__ __forceinline__ void put(int m, int n, float v) const { g[(size_t)m * N + n] = v; }
};
struct PiuConv2Grad {          // partial z: g[(c, ky, kx)][n] over positions k = r * 49 + pos of the partial's range
  static constexpr bool kMFast = false;
  int M, N, K;          // M = 289
  const float *c1, *dc2;
  float* part;
  __device__ __forceinline__ float a(int m, int k) const {
    if (m == M - 1) return 1.0f;
    const int r = k / kPiuPos2, pos = k - r * kPiuPos2;
    return c1[(size_t)r * kPiuC1 + piu_patch2(pos, m)];
  }
  __device__ __forceinline__ float b(int k, int n) const {
    const int r = k / kPiuPos2, pos = k - r * kPiuPos2;
    return dc2[(size_t)r * kPiuC2 + n * kPiuPos2 + pos];
  }
  __device__ __forceinline__ void put(int m, int n, float v) const { part[((size_t)blockIdx.z * M + m) * 32 + n] = v; }
};
struct PiuConv1Grad {
  static constexpr bool kMFast = false;
  int M, N, K;          // M = 48 F + 1
  PiuRows rows;
  const float* dc1;
  float* part;
  __device__ __forceinline__ float a(int m, int k) const {
    if (m == M - 1) return 1.0f;
    const int r = k / kPiuPos1, pos = k - r * kPiuPos1, y = pos / 15, x = pos - y * 15;
    const int c = m >> 4, ky = (m >> 2) & 3, kx = m & 3;
    return ppo_image::scaled(rows.window(r)[c * 1024 + (2 * y + ky) * 32 + 2 * x + kx]);
  }
  __device__ __forceinline__ float b(int k, int n) const {
    const int r = k / kPiuPos1, pos = k - r * kPiuPos1;
    return dc1[(size_t)r * kPiuC1 + n * kPiuPos1 + pos];
  }
  __device__ __forceinline__ void put(int m, int n, float v) const { part[((size_t)blockIdx.z * M + m) * 32 + n] = v; }
};

// grid (ceil(M / 32), ceil(N / 32), partials), block 64 W.  k_chunk: the K range of partial z is [z k_chunk, min(K, (z + 1) k_chunk)).
// W = 4 waves, or 16 where K is long and the tiles are few (head.main's forward).
template <class P, int W>
__global__ __launch_bounds__(kWave * W) void piu_gemm_k(const int* __restrict__ status, P p, int k_chunk) {
  __shared__ float red[W][kPiuTile * kPiuTile];
  if (status[0] != 0) return;
  const int w = wave_id(), l = lane_id(), i = l & 15, kq = l >> 4;
  const int m0 = (int)blockIdx.x * kPiuTile, n0 = (int)blockIdx.y * kPiuTile;
  const int k_begin = (int)blockIdx.z * k_chunk, k_end = p.K - k_begin < k_chunk ? p.K : k_begin + k_chunk;
  const int ma = m0 + i, mc = m0 + 16 + i, na = n0 + i, nc = n0 + 16 + i;
  const bool ma_ok = ma < p.M, mc_ok = mc < p.M, na_ok = na < p.N, nc_ok = nc < p.N;
  piu_f4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = piu_f4{0.0f, 0.0f, 0.0f, 0.0f};
  const int steps = (k_end - k_begin + 3) / 4;          // (the same for every lane: an MFMA needs the whole wave)
  // kPiuAhead steps' operands are asked for before the first of them is used, so that the loads overlap; a step past the range reads zeros
  for (int s = w; s < steps; s += kPiuAhead * W) {
    float a0[kPiuAhead], a1[kPiuAhead], b0[kPiuAhead], b1[kPiuAhead];
#pragma unroll
    for (int u = 0; u < kPiuAhead; ++u) {
      const int k = k_begin + 4 * (s + u * W) + kq;
      const bool k_ok = k < k_end;
      a0[u] = k_ok && ma_ok ? p.a(ma, k) : 0.0f;
      a1[u] = k_ok && mc_ok ? p.a(mc, k) : 0.0f;
      b0[u] = k_ok && na_ok ? p.b(k, na) : 0.0f;
      b1[u] = k_ok && nc_ok ? p.b(k, nc) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kPiuAhead; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0[u], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b1[u], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b0[u], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b1[u], acc[1][1], 0, 0, 0);
    }
  }
  // element e of acc[u][v] is C[16 u + 4 kq + e][16 v + i]
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[w][(16 * u + 4 * kq + e) * kPiuTile + 16 * v + i] = acc[u][v][e];
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < kPiuTile * kPiuTile; idx += kWave * W) {
    const int mi = P::kMFast ? idx & 31 : idx >> 5, ni = P::kMFast ? idx >> 5 : idx & 31;
    const int at = mi * kPiuTile + ni;
    float s = red[0][at];
#pragma unroll
    for (int q = 1; q < W; ++q) s = s + red[q][at];
    if (m0 + mi < p.M && n0 + ni < p.N) p.put(m0 + mi, n0 + ni, s);
  }
}

// ---------------------------------------------------------------------------------------------- the small kernels
// the sum of a double over the workgroup in a fixed pattern: the wave's lanes by xor butterflies, the waves in ascending order
__device__ __forceinline__ double piu_block_sum(double x, double* lds) {
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, kWave);
  __syncthreads();
  if (lane_id() == 0) lds[wave_id()] = x;
  __syncthreads();
  double total = 0.0;
  for (int k = 0; k < kPiuThreads / kWave; ++k) total = total + lds[k];
  return total;
}

__global__ void piu_begin_k(int* status) {
  if (threadIdx.x == 0) {
    status[0] = ppo_update::kOk;
    status[1] = 0;
  }
}

// grid 1.  sel: the step's mb indices
__global__ __launch_bounds__(kPiuThreads) void piu_check_k(int* status, const int* __restrict__ sel, const int* __restrict__ actions, int mb, int n) {
  __shared__ int bad;
  if (status[0] != 0) return;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int r = (int)threadIdx.x; r < mb; r += kPiuThreads) {
    const int i = sel[r];
    bool b = i < 0 || i >= n;
    if (!b) b = actions[i] < 0 || actions[i] >= ppo_update::kActions;
    if (b) bad = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0 && bad != 0) status[0] = ppo_update::kBadIndex;
}

// grid ceil(mb / 16).  h (mb, H): the last hidden layer; w: the heads' transposed weight (H, 10) and bias; dheads (mb, 10), terms
// (mb, 3), dh (mb, H): out
__global__ __launch_bounds__(kPiuThreads) void piu_heads_k(const int* __restrict__ status, const float* __restrict__ h, const float* __restrict__ w,
                                                          const int* __restrict__ sel, const int* __restrict__ actions,
                                                          const float* __restrict__ returns, const float* __restrict__ values,
                                                          const float* __restrict__ logp, const float* __restrict__ adv, float* dheads,
                                                          double* terms, float* dh, ppo_update::Hyper hy, int mb, int H) {
  __shared__ float heads[kPiuHeadRows][ppo_image::kHeads];
  __shared__ double work[kPiuHeadRows][2 * ppo_update::kActions];
  if (status[0] != 0) return;
  constexpr int J = ppo_image::kHeads;
  const int tid = (int)threadIdx.x, base = (int)blockIdx.x * kPiuHeadRows;
  {          // sixteen lanes per row: lane q sums k = q, q + 16, ... ascending, the sixteen partial sums meet in xor butterflies, the bias last
    static_assert(kPiuHeadRows * 16 == kPiuThreads, "sixteen lanes per row");
    const int r = tid >> 4, q = tid & 15, row = base + r;
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.0f;
    if (row < mb) {
      const float* x = h + (size_t)row * H;
      for (int k = q; k < H; k += 16) {
        const float xk = x[k];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = fmaf(xk, w[k * J + j], acc[j]);
      }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1)
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], off, 16);
    if (q == 0 && row < mb)
#pragma unroll
      for (int j = 0; j < J; ++j) heads[r][j] = acc[j] + w[(size_t)H * J + j];
  }
  __syncthreads();
  if (tid < kPiuHeadRows && base + tid < mb) {
    const int row = base + tid, i = sel[row];
    const ppo_update::RowTerms t = ppo_update::head_row(heads[tid], actions[i], returns[i], values[i], logp[i], adv[i], hy, mb, work[tid]);
    terms[3 * (size_t)row] = t.value;
    terms[3 * (size_t)row + 1] = t.action;
    terms[3 * (size_t)row + 2] = t.entropy;
  }
  __syncthreads();
  if (tid < kPiuHeadRows * J) {
    const int r = tid / J, j = tid - r * J, row = base + r;
    if (row < mb) dheads[(size_t)row * J + j] = heads[r][j];
  }
  for (int idx = tid; idx < kPiuHeadRows * H; idx += kPiuThreads) {
    const int r = idx / H, k = idx - r * H, row = base + r;
    if (row >= mb) break;
    float acc = 0.0f;
    for (int j = 0; j < J; ++j) acc = fmaf(w[k * J + j], heads[r][j], acc);
    dh[(size_t)row * H + k] = h[(size_t)row * H + k] > 0.0f ? acc : 0.0f;
  }
}

// the convolutions' partial gradient images added up: grid ceil((count1 + count2) / 64), block 64 x kPiuReduceWaves.  Lane l of every
// wave owns entry 64 blockIdx.x + l (of conv1's image, then of conv2's); wave w adds the partials z = w, w + 16, ... in ascending
// order, the sixteen sums meet in LDS and are added in ascending order of w.
__global__ __launch_bounds__(kWave * kPiuReduceWaves) void piu_reduce_k(const int* __restrict__ status, const float* __restrict__ part1, int parts1,
                                                                       int count1, const float* __restrict__ part2, int parts2, int count2,
                                                                       float* g1, float* g2) {
  __shared__ float red[kPiuReduceWaves][kWave];
  if (status[0] != 0) return;
  const int w = wave_id(), l = lane_id();
  int e = (int)blockIdx.x * kWave + l;
  const bool first = e < count1;
  if (!first) e -= count1;
  const float* part = first ? part1 : part2;
  const int parts = first ? parts1 : parts2, count = first ? count1 : count2;
  float s = 0.0f;
  if (e < count)
    for (int z = w; z < parts; z += kPiuReduceWaves) s = s + part[(size_t)z * count + e];
  red[w][l] = s;
  __syncthreads();
  if (w == 0 && e < count) {
    float total = red[0][l];
#pragma unroll
    for (int q = 1; q < kPiuReduceWaves; ++q) total = total + red[q][l];
    (first ? g1 : g2)[e] = total;
  }
}

// grid ceil(P / 4096): block b's float64 sum of the squares of its 4096 entries
__global__ __launch_bounds__(kPiuThreads) void piu_norm_k(const int* __restrict__ status, const float* __restrict__ grad, double* part, int P) {
  __shared__ double lds[kPiuThreads / kWave];
  if (status[0] != 0) return;
  const int lo = (int)blockIdx.x * kPiuNormChunk;
  double sq = 0.0;
  for (int e = lo + (int)threadIdx.x; e < lo + kPiuNormChunk && e < P; e += kPiuThreads) sq = sq + (double)grad[e] * (double)grad[e];
  sq = piu_block_sum(sq, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// grid 1: the step's scalars
__global__ __launch_bounds__(kPiuThreads) void piu_finish_k(int* status, const double* __restrict__ part, int parts, const double* __restrict__ terms,
                                                           int mb, const int* __restrict__ step, double* scal, float* losses, float* gnorm,
                                                           ppo_update::Hyper hy) {
  __shared__ double lds[kPiuThreads / kWave];
  if (status[0] != 0) return;
  const int tid = (int)threadIdx.x;
  double sq = 0.0, value = 0.0, action = 0.0, entropy = 0.0;
  for (int b = tid; b < parts; b += kPiuThreads) sq = sq + part[b];
  for (int r = tid; r < mb; r += kPiuThreads) {
    value = value + terms[3 * (size_t)r];
    action = action + terms[3 * (size_t)r + 1];
    entropy = entropy + terms[3 * (size_t)r + 2];
  }
  sq = piu_block_sum(sq, lds);
  value = piu_block_sum(value, lds) / (double)mb;
  action = piu_block_sum(action, lds) / (double)mb;
  entropy = piu_block_sum(entropy, lds) / (double)mb;
  if (tid != 0) return;
  const double norm = sqrt(sq);
  if (!ppo_update::finite(value) || !ppo_update::finite(action) || !ppo_update::finite(entropy) || !ppo_update::finite(norm)) {
    status[0] = ppo_update::kNonFinite;
    return;
  }
  const int t = step[0] + 1;
  const ppo_update::AdamStep a = ppo_update::adam_step(t, hy.lr);
  scal[kPiuCoef] = (double)(float)ppo_update::clip_coef(norm, hy.max_grad_norm);
  scal[kPiuStepSize] = a.step_size;
  scal[kPiuRootBias2] = a.root_bias2;
  scal[kPiuT] = (double)t;
  losses[0] = (float)value;
  losses[1] = (float)action;
  losses[2] = (float)entropy;
  gnorm[0] = (float)norm;
}

// grid ceil(P / 256).  grad_out: NULL, or where the step's unclipped gradient image is kept
__global__ __launch_bounds__(kPiuThreads) void piu_adam_k(int* status, float* params, float* m, float* v, int* step, const float* __restrict__ grad,
                                                         float* grad_out, const double* __restrict__ scal, float eps, int P, int done) {
  if (status[0] != 0) return;
  const int e = (int)(blockIdx.x * kPiuThreads + threadIdx.x);
  if (e < P) {
    const ppo_update::AdamStep a{scal[kPiuStepSize], scal[kPiuRootBias2]};
    const float g = grad[e];
    float mm = m[e], vv = v[e];
    params[e] = ppo_update::adam_entry(params[e], g, (float)scal[kPiuCoef], &mm, &vv, a, eps);
    m[e] = mm;
    v[e] = vv;
    if (grad_out != nullptr) grad_out[e] = g;
  }
  if (e == 0) {
    step[0] = (int)scal[kPiuT];
    status[1] = done;
  }
}

// ---------------------------------------------------------------------------------------------- the chain
template <int W = 4, class P>
static int piu_gemm(hipStream_t st, const int* status, const P& p, int parts = 1, int k_chunk = 0) {
  const dim3 grid((unsigned)((p.M + kPiuTile - 1) / kPiuTile), (unsigned)((p.N + kPiuTile - 1) / kPiuTile), (unsigned)parts);
  auto* kern = piu_gemm_k<P, W>;
  STOVE_LAUNCH(kern, grid, dim3(kWave * W), 0, st, status, p, parts == 1 ? p.K : k_chunk);
  return (int)hipGetLastError();
}
#define PIU_TRY(expr)             \
  do {                            \
    const int e__ = (expr);       \
    if (e__ != 0) return e__;     \
  } while (0)

// the arguments as stove_ppo_update_images takes them (checked before)
static int piu_run(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns, const float* values,
                   const float* logp, const float* adv, const int* perm, float* losses, float* gnorm, float* grad_out, int* status, void* ws,
                   int n, int S, int env_stride, int M, int max_steps, const ppo_image::Shape& sh, const ppo_update::Hyper& hy, hipStream_t st) {
  STOVE_LAUNCH(piu_begin_k, dim3(1), dim3(kWave), 0, st, status);
  STOVE_LAUNCH_CHECK();
  if (max_steps == 0) return 0;
  const int mb = n / M, H = sh.H, L = ppo_image::layers(sh), P = (int)ppo_image::param_floats(sh), K1 = 48 * sh.F;
  const PiuWs w = piu_ws(mb, sh);
  char* base = (char*)ws;
  double *scal = (double*)(base + w.scal), *normpart = (double*)(base + w.normpart), *terms = (double*)(base + w.terms);
  float *c1 = (float*)(base + w.c1), *c2 = (float*)(base + w.c2), *h = (float*)(base + w.h), *dheads = (float*)(base + w.dheads);
  float *dh = (float*)(base + w.dh), *dc2 = (float*)(base + w.dc2), *dc1 = (float*)(base + w.dc1), *grad = (float*)(base + w.grad);
  float *part2 = (float*)(base + w.part2), *part1 = (float*)(base + w.part1);
  const size_t hs = (size_t)mb * H;          // one hidden layer's rows
  const PiuSplit s1 = piu_split((long long)mb * kPiuPos1), s2 = piu_split((long long)mb * kPiuPos2);
  const int hidden = L - 3;                  // head.main and the deep layers
  for (int at = 0; at < max_steps; ++at) {
    const int* sel = perm + (size_t)(at / M) * n + (size_t)(at % M) * mb;
    const PiuRows rows{obs, sel, S, env_stride};
    STOVE_LAUNCH(piu_check_k, dim3(1), dim3(kPiuThreads), 0, st, status, sel, actions, mb, n);
    STOVE_LAUNCH_CHECK();
    // ---- forward
    PIU_TRY(piu_gemm(st, status, PiuConv1Fwd{mb * kPiuPos1, 32, K1, rows, params, c1}));
    PIU_TRY(piu_gemm(st, status, PiuConv2Fwd{mb * kPiuPos2, 32, 288, c1, params + ppo_image::offset(sh, 1), c2}));
    PIU_TRY(piu_gemm<16>(st, status, PiuFcFwd{mb, H, kPiuC2, c2, params + ppo_image::offset(sh, 2), h}));
    for (int q = 1; q < hidden; ++q)
      PIU_TRY(piu_gemm(st, status, PiuFcFwd{mb, H, H, h + (q - 1) * hs, params + ppo_image::offset(sh, 2 + q), h + q * hs}));
    const float* w_heads = params + ppo_image::offset(sh, L - 1);
    STOVE_LAUNCH(piu_heads_k, dim3((unsigned)((mb + kPiuHeadRows - 1) / kPiuHeadRows)), dim3(kPiuThreads), 0, st, status, h + (hidden - 1) * hs, w_heads,
                 sel, actions, returns, values, logp, adv, dheads, terms, dh + (hidden - 1) * hs, hy, mb, H);
    STOVE_LAUNCH_CHECK();
    // ---- backward
    for (int q = hidden - 1; q >= 1; --q)
      PIU_TRY(piu_gemm(st, status, PiuFcBwd{mb, H, H, dh + q * hs, params + ppo_image::offset(sh, 2 + q), h + (q - 1) * hs, dh + (q - 1) * hs}));
    PIU_TRY(piu_gemm(st, status, PiuFcBwd{mb, kPiuC2, H, dh, params + ppo_image::offset(sh, 2), c2, dc2}));
    PIU_TRY(piu_gemm(st, status, PiuConv2Bwd{mb * kPiuPos1, 32, 288, dc2, params + ppo_image::offset(sh, 1), c1, dc1}));
    // ---- the weight gradients
    PIU_TRY(piu_gemm(st, status, PiuFcGrad{H + 1, ppo_image::kHeads, mb, h + (hidden - 1) * hs, dheads, grad + ppo_image::offset(sh, L - 1)}));
    for (int q = hidden - 1; q >= 0; --q)
      PIU_TRY(piu_gemm(st, status, PiuFcGrad{(q == 0 ? kPiuC2 : H) + 1, H, mb, q == 0 ? c2 : h + (q - 1) * hs, dh + q * hs, grad + ppo_image::offset(sh, 2 + q)}));
    PIU_TRY(piu_gemm(st, status, PiuConv2Grad{289, 32, mb * kPiuPos2, c1, dc2, part2}, s2.count, s2.chunk));
    PIU_TRY(piu_gemm(st, status, PiuConv1Grad{K1 + 1, 32, mb * kPiuPos1, rows, dc1, part1}, s1.count, s1.chunk));
    const int count1 = (K1 + 1) * 32, count2 = 289 * 32;
    STOVE_LAUNCH(piu_reduce_k, dim3((unsigned)((count1 + count2 + kWave - 1) / kWave)), dim3(kWave * kPiuReduceWaves), 0, st, status, part1, s1.count,
                 count1, part2, s2.count, count2, grad, grad + ppo_image::offset(sh, 1));
    STOVE_LAUNCH_CHECK();
    // ---- the optimiser
    STOVE_LAUNCH(piu_norm_k, dim3((unsigned)w.norm_blocks), dim3(kPiuThreads), 0, st, status, grad, normpart, P);
    STOVE_LAUNCH_CHECK();
    STOVE_LAUNCH(piu_finish_k, dim3(1), dim3(kPiuThreads), 0, st, status, normpart, w.norm_blocks, terms, mb, step, scal, losses + (size_t)at * 3,
                 gnorm + at, hy);
    STOVE_LAUNCH_CHECK();
    STOVE_LAUNCH(piu_adam_k, dim3((unsigned)((P + kPiuThreads - 1) / kPiuThreads)), dim3(kPiuThreads), 0, st, status, params, m, v, step, grad, grad_out,
                 scal, hy.eps, P, at + 1);
    STOVE_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace stove
