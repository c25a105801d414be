// Frame rendering at run-time sizes with the squared pixel error fused in (stove_render_frames_any, capi.hip): the composed branch of
// Supair.reconstruct_from_z (supair.py:484-498) per channel,
//   frame = clamp(bg + sum_k grid_sample(patch_k; [[1/sx, 0, -x/sx], [0, 1/sy, -y/sy]]), 0, 1),
// bilinear, zero padding, either align_corners convention, and sqerr[f] = sum over the frame's pixels of (frame - truth)^2.
//
// Layout (the width / height order of that code): a frame plane has W rows of H columns, pixel (c, r, q) at c*W*H + r*H + q; a patch
// plane has pw rows of ph columns.  The transform's x (sx, z[2]) runs along the columns, its y (sy, z[3]) along the rows.
//
// One workgroup of 256 threads per (tile of positions, frame); a position (r, q) is one thread's work for ALL channels, so the taps are
// computed once.  The workgroup first computes the n_obj inverse transforms folded with the pixel <-> normalised maps and each object's
// reach (the rows / columns whose taps can touch the patch), keeps them in LDS, and stages the patch rows of its frame there when
// they fit (STAGE); a position then skips every object whose reach misses it.
//
// With sqerr the grid has ONE tile per frame, so that the sum needs no second pass and no atomics: a thread adds its positions in
// ascending order (channels innermost), the 64 lanes of a wave are summed by wave_sum's fixed DPP tree, and thread 0 adds the four
// wave totals in wave order.  The order depends on nothing but (C, W, H): two calls agree bit for bit, with or without `out`.
// The price: a frame is one workgroup whatever its size, so a few very large frames are slower than the tiled launch plus a sum by the
// caller (DESIGN 4d has the figures); the evaluation scores thousands of small frames.
#pragma once
#include "common.h"

namespace stove {

constexpr int kRenderThreads = 256;
constexpr int kRenderMaxObj = 8;
constexpr int kRenderMaxCh = 4;

// pixel index -> normalised coordinate (affine_grid), normalised -> source index (grid_sample): idx = un_a * g + un_b
struct RenderGeom {
  int C, W, H, pw, ph;
  float col_a, col_b, row_a, row_b;          // u = col_a * q + col_b over the H columns, v = row_a * r + row_b over the W rows
  float px_a, px_b, py_a, py_b;              // patch column = px_a * gx + px_b (ph columns), patch row = py_a * gy + py_b (pw rows)
};

struct RenderObj {
  float ax, bx, ay, by;                      // gx = ax * u + bx, gy = ay * v + by
  int q0, q1, r0, r1;                        // reach: columns q0..q1 and rows r0..r1 (inclusive; empty when q0 > q1 or r0 > r1)
};

// Pixel indices i in [0, n) whose source index s = a * i + b can have a tap inside [0, m): -1 < s < m, widened by one pixel for the
// rounding of the float evaluation.  Anything not finite keeps the whole range (the taps themselves are checked again).
__device__ inline void render_reach(float a, float b, int n, int m, int* lo, int* hi) {
  *lo = 0;
  *hi = n - 1;
  const float e0 = (-1.0f - b) / a, e1 = ((float)m - b) / a;
  if (!(fabsf(e0) < 1e30f) || !(fabsf(e1) < 1e30f)) {
    if (a == 0.0f && !(b > -1.0f && b < (float)m)) *hi = -1;           // a constant source index outside the patch: nothing
    return;
  }
  const float l = fminf(fmaxf(floorf(fminf(e0, e1)) - 1.0f, 0.0f), (float)n);
  const float h = fminf(fmaxf(ceilf(fmaxf(e0, e1)) + 1.0f, -1.0f), (float)(n - 1));
  *lo = (int)l;
  *hi = (int)h;
}

// grid (n_frames, tiles), block 256, dynamic LDS: STAGE ? rows * C*pw*ph floats : 0.  tile_len positions per tile.
template <bool STAGE>
__global__ __launch_bounds__(kRenderThreads) void render_frames_any_k(const float* __restrict__ bg, const float* __restrict__ patches,
                                                                       int frames_per_patch, const float* __restrict__ z,
                                                                       const float* __restrict__ truth, float* __restrict__ out,
                                                                       float* __restrict__ sqerr, int n_obj, RenderGeom gm, int tile_len) {
  extern __shared__ float render_lds[];
  __shared__ RenderObj obj[kRenderMaxObj];
  __shared__ float wave_tot[kRenderThreads / 64];
  const int f = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
  const int P = gm.W * gm.H, PD = gm.C * gm.pw * gm.ph, pp = gm.pw * gm.ph;
  const size_t row0 = frames_per_patch > 0 ? (size_t)(f / frames_per_patch) * n_obj : 0;
  const int rows = frames_per_patch > 0 ? n_obj : 1;
  if (tid < n_obj) {
    const float* zk = z + ((size_t)f * n_obj + tid) * 4;
    RenderObj o;
    o.ax = 1.0f / zk[0];
    o.bx = -zk[2] / zk[0];
    o.ay = 1.0f / zk[1];
    o.by = -zk[3] / zk[1];
    // source column as a function of the pixel column: px_a * (ax * (col_a * q + col_b) + bx) + px_b
    render_reach(gm.px_a * o.ax * gm.col_a, gm.px_a * (o.ax * gm.col_b + o.bx) + gm.px_b, gm.H, gm.ph, &o.q0, &o.q1);
    render_reach(gm.py_a * o.ay * gm.row_a, gm.py_a * (o.ay * gm.row_b + o.by) + gm.py_b, gm.W, gm.pw, &o.r0, &o.r1);
    obj[tid] = o;
  }
  if constexpr (STAGE) {
    const float* src = patches + row0 * PD;
    for (int i = tid; i < rows * PD; i += kRenderThreads) render_lds[i] = src[i];
  }
  __syncthreads();

  const int p_end = min(P, (tile + 1) * tile_len);
  const size_t fbase = (size_t)f * gm.C * P;
  float err = 0.0f;
  for (int p = tile * tile_len + tid; p < p_end; p += kRenderThreads) {
    const int r = p / gm.H, q = p - r * gm.H;
    const float u = gm.col_a * (float)q + gm.col_b, v = gm.row_a * (float)r + gm.row_b;
    float acc[kRenderMaxCh];
#pragma unroll
    for (int c = 0; c < kRenderMaxCh; ++c) acc[c] = c < gm.C ? bg[(size_t)c * P + p] : 0.0f;
    for (int k = 0; k < n_obj; ++k) {
      const RenderObj o = obj[k];
      if (q < o.q0 || q > o.q1 || r < o.r0 || r > o.r1) continue;
      const float gx = o.ax * u + o.bx, gy = o.ay * v + o.by;
      const Tap1 tx = make_tap(gm.px_a * gx + gm.px_b, gm.ph);
      const Tap1 ty = make_tap(gm.py_a * gy + gm.py_b, gm.pw);
      const int krow = frames_per_patch > 0 ? k : 0;
      const float* pt = STAGE ? render_lds + krow * PD : patches + (row0 + krow) * PD;
      float s[kRenderMaxCh] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float inb = (a ? ty.in1 : ty.in0) * (b ? tx.in1 : tx.in0);
          if (inb != 0.0f) {                                       // the tap lies inside the patch: the read is in bounds
            const float w = (a ? ty.t : 1.0f - ty.t) * (b ? tx.t : 1.0f - tx.t);
            const int at = (ty.i0 + a) * gm.ph + tx.i0 + b;
#pragma unroll
            for (int c = 0; c < kRenderMaxCh; ++c)
              if (c < gm.C) s[c] = fmaf(w, pt[c * pp + at], s[c]);
          }
        }
#pragma unroll
      for (int c = 0; c < kRenderMaxCh; ++c) acc[c] += s[c];
    }
#pragma unroll
    for (int c = 0; c < kRenderMaxCh; ++c) {
      if (c < gm.C) {
        const float val = fminf(fmaxf(acc[c], 0.0f), 1.0f);
        const size_t at = fbase + (size_t)c * P + p;
        if (out) out[at] = val;
        if (sqerr) {
          const float d = val - truth[at];
          err = fmaf(d, d, err);
        }
      }
    }
  }
  if (sqerr) {                                   // (one tile per frame here: the workgroup holds the whole frame's sum)
    const float w = wave_sum(err);
    if (lane_id() == 0) wave_tot[wave_id()] = w;
    __syncthreads();
    if (tid == 0) {
      float tot = wave_tot[0];
      for (int i = 1; i < kRenderThreads / 64; ++i) tot += wave_tot[i];
      sqerr[f] = tot;
    }
  }
}

}  // namespace stove
