// Scene side of the likelihood over C colour planes (reference supair.py:44-110 with config.channels = C, debug_bw = False):
// glimpses and occlusion masks of every channel, and their backward to z.
//
// With colour the object SPN models C x patch_width x patch_height dimensions (300 at the default 10 x 10 glimpses), which the tuned
// 100-dimension tile kernels do not cover: the object side is the general-size operator of spn_obj_generic.hip on dense
// patches[np][C * pw * ph] / marg[np][C * pw * ph] rows in the reference's flatten order (c, pw, ph), and the background side the
// general-size operator of spn_bg_generic.hip over C * W * H dimensions with the mask plane (W * H) repeated for every channel.
//
// One wave per glimpse, lane = glimpse pixel (a loop of ceil(pw ph / 64) passes).  The sampling geometry of a pixel -- its bilinear
// taps and weights and the mask of the earlier objects at them -- is formed once and shared by the C channels.  The mask is the
// closed form of scene.hip (a pasted unit box is separable; the sequential clamps collapse), so it is identical across channels, as
// masks_from_z gives it.  The per-glimpse sums (the overlap ratio; dz of the glimpse's own box and of its occluders' boxes) are wave
// reductions in a fixed order: no atomics, so a replayed step is bit-equal to an eager one.
#include "common.h"

namespace stove {

constexpr int kColMaxC = 4;

// Glimpse of run-time size: pixel p = i ph + j sits at row i of pw (grid_sample's y) and column j of ph (its x), at the normalised
// coordinates u = pax j + pbx, v = pay i + pby ((2j + 1) / ph - 1, or -1 + 2j / (ph - 1) with align_corners).
struct GlimpseGeom {
  int pw, ph;
  float pax, pbx, pay, pby;
};

__device__ __forceinline__ PatchPix patch_pix_c(const float4 zk, int p, const SceneGeom& gm, const GlimpseGeom& gg) {
  PatchPix q;
  const int i = p / gg.ph, j = p - i * gg.ph;
  q.u = fmaf(gg.pax, (float)j, gg.pbx);
  q.v = fmaf(gg.pay, (float)i, gg.pby);
  const float gx = fmaf(zk.x, q.u, zk.z);
  const float gy = fmaf(zk.y, q.v, zk.w);
  q.tx = make_tap(fmaf(gm.sxa, gx, gm.cx), gm.W);
  q.ty = make_tap(fmaf(gm.sya, gy, gm.cy), gm.H);
  return q;
}

// frames: rows of C * W * H floats (frame map fm); z [np][4] = [sx, sy, x, y] -> patches, marg [np][C * pw * ph], ovl [np]
template <int NMAX>
__global__ __launch_bounds__(256) void scene_colour_fwd_k(const float* __restrict__ frames, const float* __restrict__ z,
                                                          float* __restrict__ patches, float* __restrict__ marg, float* __restrict__ ovl,
                                                          int n_obj, int n_patches, int C, FrameMap fm, SceneGeom gm, GlimpseGeom gg) {
  const int patch = blockIdx.x * 4 + wave_id();
  if (patch >= n_patches) return;              // wave-uniform
  const int lane = lane_id();
  const int f = patch / n_obj, k = patch % n_obj;
  const int IW = gm.W, IH = gm.H, plane = IW * IH, P = gg.pw * gg.ph;
  const float* zf = z + (size_t)f * n_obj * 4;
  const float4 zk = *reinterpret_cast<const float4*>(zf + k * 4);
  constexpr int NOCC = NMAX > 1 ? NMAX - 1 : 1;      // the last object of a frame occludes nobody
  float isx[NOCC], isy[NOCC], ox[NOCC], oy[NOCC];
#pragma unroll
  for (int j = 0; j < NOCC; ++j) {
    const float4 zj = *reinterpret_cast<const float4*>(zf + (j < n_obj ? j : 0) * 4);
    isx[j] = 1.0f / zj.x;
    isy[j] = 1.0f / zj.y;
    ox[j] = -zj.z * isx[j];
    oy[j] = -zj.w * isy[j];
  }
  const float* img = frames + fm.row(f) * (size_t)C * plane;
  float* pr = patches + (size_t)patch * C * P;
  float* mr = marg + (size_t)patch * C * P;
  float msum = 0.0f;
  for (int p = lane; p < P; p += 64) {
    const PatchPix q = patch_pix_c(zk, p, gm, gg);
    int off[4];
    float wt[4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int iy = min(max(q.ty.i0 + a, 0), IH - 1), ix = min(max(q.tx.i0 + c, 0), IW - 1);
        off[a * 2 + c] = iy * IW + ix;
        wt[a * 2 + c] = (a ? q.ty.in1 : q.ty.in0) * (c ? q.tx.in1 : q.tx.in0) * (a ? q.ty.t : 1.0f - q.ty.t) * (c ? q.tx.t : 1.0f - q.tx.t);
      }
    // earlier objects' coverage at the two tap columns / rows; run[a][c] = min(1, sum of their boxes) at tap (a, c)
    float run[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < NOCC; ++j) {
      if (j < k) {
        float d;
        const float cx0 = cover(inv_pix_x(isx[j], ox[j], q.tx.i0, gm), IW, &d), cx1 = cover(inv_pix_x(isx[j], ox[j], q.tx.i0 + 1, gm), IW, &d);
        const float cy0 = cover(inv_pix_y(isy[j], oy[j], q.ty.i0, gm), IH, &d), cy1 = cover(inv_pix_y(isy[j], oy[j], q.ty.i0 + 1, gm), IH, &d);
        run[0] = fminf(run[0] + cx0 * cy0, 1.0f);
        run[1] = fminf(run[1] + cx1 * cy0, 1.0f);
        run[2] = fminf(run[2] + cx0 * cy1, 1.0f);
        run[3] = fminf(run[3] + cx1 * cy1, 1.0f);
      }
    }
    float seen = 0.0f;
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) seen = fmaf(wt[t4], 1.0f - run[t4], seen);
    const float mg = 1.0f - seen;                   // supair.py:331, the same in every channel
    msum += mg;
    for (int c = 0; c < C; ++c) {
      const float* ic = img + (size_t)c * plane;
      float xv = 0.0f;
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) xv = fmaf(wt[t4], ic[off[t4]], xv);
      pr[c * P + p] = xv;
      mr[c * P + p] = mg;
    }
  }
  // overlap ratio = mean of the mask over (c, pw, ph) = its mean over one plane
  const float s = wave_sum(msum);
  if (lane == 0) ovl[patch] = s / (float)P;
}

// d_patch, d_marg [np][C * pw * ph] (the object SPN's data gradients; d_marg already gated by its clamp), d_ovl [np] ->
// dzc[patch][NMAX][4]: entry j = k (the glimpse's own object) through the sample locations, entries j < k (its occluders) through
// the mask 1 - sample(1 - bg_<k).  The arithmetic is that of scene_pixtile_bwd_k<.., ANY> (scene_fused.hip) with the image term
// summed over the channels and the mask gradient summed over the planes, in channel order.
template <int NMAX>
__global__ __launch_bounds__(256) void scene_colour_bwd_k(const float* __restrict__ frames, const float* __restrict__ z,
                                                          const float* __restrict__ d_patch, const float* __restrict__ d_marg,
                                                          const float* __restrict__ d_ovl, float* __restrict__ dzc, int n_obj, int n_patches,
                                                          int C, FrameMap fm, SceneGeom gm, GlimpseGeom gg) {
  const int patch = blockIdx.x * 4 + wave_id();
  if (patch >= n_patches) return;              // wave-uniform
  const int lane = lane_id();
  const int f = patch / n_obj, k = patch % n_obj;
  const int IW = gm.W, IH = gm.H, plane = IW * IH, P = gg.pw * gg.ph;
  const float SXA = gm.sxa, SYA = gm.sya, CXc = gm.cx, CYc = gm.cy;
  const float* zf = z + (size_t)f * n_obj * 4;
  const float4 zk = *reinterpret_cast<const float4*>(zf + k * 4);
  const float* img = frames + fm.row(f) * (size_t)C * plane;
  const float* dpr = d_patch + (size_t)patch * C * P;
  const float* dmr = d_marg + (size_t)patch * C * P;
  const float govl = d_ovl[patch] * (-1.0f / (float)P);    // d overlap / d seen, summed over the C identical planes
  constexpr int NOCC = NMAX > 1 ? NMAX - 1 : 1;
  // occluders j < k: q(X) = isx (X - cx) + cxo;  j >= k: coverage 0 everywhere (through the constants)
  float isx[NOCC], isy[NOCC], cxo[NOCC], cyo[NOCC], xj[NOCC], yj[NOCC];
#pragma unroll
  for (int j = 0; j < NOCC; ++j) {
    const bool occ = j < k;
    const float sx = occ ? zf[j * 4] : 1.0f, sy = occ ? zf[j * 4 + 1] : 1.0f;
    xj[j] = occ ? zf[j * 4 + 2] : 0.0f;
    yj[j] = occ ? zf[j * 4 + 3] : 0.0f;
    isx[j] = occ ? 1.0f / sx : 0.0f;
    isy[j] = occ ? 1.0f / sy : 0.0f;
    cxo[j] = occ ? fmaf(-SXA * xj[j], isx[j], CXc) : -100.0f;
    cyo[j] = occ ? fmaf(-SYA * yj[j], isy[j], CYc) : -100.0f;
  }
  float own[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sx0[NOCC], sx2[NOCC], sy1[NOCC], sy3[NOCC];      // raw occluder sums: dqx (uu - x_j), dqx, dqy (vv - y_j), dqy
#pragma unroll
  for (int j = 0; j < NOCC; ++j) sx0[j] = sx2[j] = sy1[j] = sy3[j] = 0.0f;
  const float nW = (float)IW, nH = (float)IH;
  for (int p = lane; p < P; p += 64) {
    const PatchPix q = patch_pix_c(zk, p, gm, gg);
    const int c0 = min(max(q.tx.i0, 0), IW - 1), c1 = min(max(q.tx.i0 + 1, 0), IW - 1);
    const int r0 = min(max(q.ty.i0, 0), IH - 1), r1 = min(max(q.ty.i0 + 1, 0), IH - 1);
    const float inb00 = q.ty.in0 * q.tx.in0, inb01 = q.ty.in0 * q.tx.in1, inb10 = q.ty.in1 * q.tx.in0, inb11 = q.ty.in1 * q.tx.in1;
    const float wy0 = 1.0f - q.ty.t, wy1 = q.ty.t, wx0 = 1.0f - q.tx.t, wx1 = q.tx.t;
    // image term of the own object, summed over the channels; the mask gradient summed over the planes
    float gix = 0.0f, giy = 0.0f, dmg = 0.0f;
#pragma unroll
    for (int c = 0; c < kColMaxC; ++c) {
      if (c < C) {
        const float* ic = img + (size_t)c * plane;
        const float gX = dpr[c * P + p];
        const float im00 = ic[r0 * IW + c0] * inb00, im01 = ic[r0 * IW + c1] * inb01;
        const float im10 = ic[r1 * IW + c0] * inb10, im11 = ic[r1 * IW + c1] * inb11;
        gix = fmaf(gX, wy0 * (im01 - im00) + wy1 * (im11 - im10), gix);
        giy = fmaf(gX, wx0 * (im10 - im00) + wx1 * (im11 - im01), giy);
        dmg += dmr[c * P + p];
      }
    }
    float cx[NOCC][2], cy[NOCC][2], dcx[NOCC][2], dcy[NOCC][2];
    float s00 = 0.0f, s01 = 0.0f, s10 = 0.0f, s11 = 0.0f;     // mask sum at tap (row a, column c): s_ac
    const float fx = (float)q.tx.i0 - CXc, fy = (float)q.ty.i0 - CYc;
#pragma unroll
    for (int j = 0; j < NOCC; ++j) {
      const float qx = fmaf(isx[j], fx, cxo[j]), qy = fmaf(isy[j], fy, cyo[j]);
      cx[j][0] = cover_cf(qx, &dcx[j][0], nW);
      cx[j][1] = cover_cf(qx + isx[j], &dcx[j][1], nW);
      cy[j][0] = cover_cf(qy, &dcy[j][0], nH);
      cy[j][1] = cover_cf(qy + isy[j], &dcy[j][1], nH);
      s00 = fmaf(cx[j][0], cy[j][0], s00);
      s01 = fmaf(cx[j][1], cy[j][0], s01);
      s10 = fmaf(cx[j][0], cy[j][1], s10);
      s11 = fmaf(cx[j][1], cy[j][1], s11);
    }
    const float vis00 = (1.0f - fminf(s00, 1.0f)) * inb00, vis01 = (1.0f - fminf(s01, 1.0f)) * inb01;
    const float vis10 = (1.0f - fminf(s10, 1.0f)) * inb10, vis11 = (1.0f - fminf(s11, 1.0f)) * inb11;
    // mg = 1 - seen: dL/dseen = -dL/dmg (the SPN's share, gated by its clamp) plus the overlap prior's
    const float dseen = govl - dmg;
    const float dpx = gix + dseen * (wy0 * (vis01 - vis00) + wy1 * (vis11 - vis10));
    const float dpy = giy + dseen * (wx0 * (vis10 - vis00) + wx1 * (vis11 - vis01));
    const float dgx = dpx * SXA, dgy = dpy * SYA;
    own[0] = fmaf(dgx, q.u, own[0]);
    own[1] = fmaf(dgy, q.v, own[1]);
    own[2] += dgx;
    own[3] += dgy;
    // occluders: through the mask value at each tap; dbox_ac = -dseen * wt_ac where the tap is inside and unclamped
    const float nb00 = (inb00 != 0.0f && s00 <= 1.0f) ? -dseen * wy0 * wx0 : 0.0f;
    const float nb01 = (inb01 != 0.0f && s01 <= 1.0f) ? -dseen * wy0 * wx1 : 0.0f;
    const float nb10 = (inb10 != 0.0f && s10 <= 1.0f) ? -dseen * wy1 * wx0 : 0.0f;
    const float nb11 = (inb11 != 0.0f && s11 <= 1.0f) ? -dseen * wy1 * wx1 : 0.0f;
    const float uu0 = fmaf(gm.fax, (float)q.tx.i0, gm.fbx), uu1 = uu0 + gm.fax;
    const float vv0 = fmaf(gm.fay, (float)q.ty.i0, gm.fby), vv1 = vv0 + gm.fay;
#pragma unroll
    for (int j = 0; j < NOCC; ++j) {
      const float gx0 = fmaf(nb00, cy[j][0], nb10 * cy[j][1]) * dcx[j][0];     // column c = 0: sum over the two rows
      const float gx1 = fmaf(nb01, cy[j][0], nb11 * cy[j][1]) * dcx[j][1];
      const float gy0 = fmaf(nb00, cx[j][0], nb01 * cx[j][1]) * dcy[j][0];     // row a = 0: sum over the two columns
      const float gy1 = fmaf(nb10, cx[j][0], nb11 * cx[j][1]) * dcy[j][1];
      sx0[j] = fmaf(gx0, uu0 - xj[j], fmaf(gx1, uu1 - xj[j], sx0[j]));
      sx2[j] += gx0 + gx1;
      sy1[j] = fmaf(gy0, vv0 - yj[j], fmaf(gy1, vv1 - yj[j], sy1[j]));
      sy3[j] += gy0 + gy1;
    }
  }
  // q = (X - cx)/s + cx - sxa x/s  =>  dL/ds = -sxa (uu - x)/s^2 dL/dq,  dL/dx = -sxa/s dL/dq: the raw sums, scaled after the reduction
  float* out = dzc + (size_t)patch * NMAX * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float s = wave_sum(own[e]);
    if (lane == 0) out[k * 4 + e] = s;
  }
#pragma unroll
  for (int j = 0; j < NOCC; ++j) {
    if (j < k) {                               // wave-uniform
      const float a0 = wave_sum(sx0[j]), a1 = wave_sum(sy1[j]), a2 = wave_sum(sx2[j]), a3 = wave_sum(sy3[j]);
      if (lane == 0) {
        out[j * 4 + 0] = -SXA * isx[j] * isx[j] * a0;
        out[j * 4 + 1] = -SYA * isy[j] * isy[j] * a1;
        out[j * 4 + 2] = -SXA * isx[j] * a2;
        out[j * 4 + 3] = -SYA * isy[j] * a3;
      }
    }
  }
}

template <int NMAX>
static int scene_colour_fwd(const float* frames, const float* z, float* patches, float* marg, float* ovl, int n_obj, int np, int C, hipStream_t st,
                            FrameMap fm, SceneGeom gm, GlimpseGeom gg) {
  if (np == 0) return 0;
  STOVE_LAUNCH((scene_colour_fwd_k<NMAX>), dim3((np + 3) / 4), dim3(256), 0, st, frames, z, patches, marg, ovl, n_obj, np, C, fm, gm, gg);
  STOVE_LAUNCH_CHECK();
  return 0;
}

template <int NMAX>
static int scene_colour_bwd(const float* frames, const float* z, const float* d_patch, const float* d_marg, const float* d_ovl, float* dzc, int n_obj,
                            int np, int C, hipStream_t st, FrameMap fm, SceneGeom gm, GlimpseGeom gg) {
  if (np == 0) return 0;
  STOVE_LAUNCH((scene_colour_bwd_k<NMAX>), dim3((np + 3) / 4), dim3(256), 0, st, frames, z, d_patch, d_marg, d_ovl, dzc, n_obj, np, C, fm, gm, gg);
  STOVE_LAUNCH_CHECK();
  return 0;
}

}  // namespace stove
