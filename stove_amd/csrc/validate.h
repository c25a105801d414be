// Argument validation of the C ABI's entry points (include/stove_hip.h): plain host C++, no HIP types, so that the same code is
// compiled twice -- into libstove_hip.so (every entry point below calls its check first and returns the code) and, with
// -fsanitize=address,undefined, into the host-only driver tests/abi/validate_driver.cpp that the CPU test suite runs (SURVEY section 5,
// "Race detection / sanitizers").  A check reads its pointer ARGUMENTS (NULL, alignment) and the host-side table structs; it never
// dereferences device memory.  Return: 0 or kStoveInvalidValue (== hipErrorInvalidValue, asserted in capi.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/stove_hip.h"

namespace stove_validate {

constexpr int kStoveInvalidValue = 1;
constexpr int kMaxObjects = 8;        // N <= 8 everywhere (csrc/gnn.hip, scene kernels); the small-graph recursion kernels take 2..6

inline bool null_any() { return false; }
template <typename T, typename... Rest>
inline bool null_any(const T* p, const Rest*... rest) { return p == nullptr || null_any(rest...); }
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

inline int obj_tables(const StoveSpnTables* t) {
  if (t == nullptr || null_any(t->obj_scope, t->obj_coef, t->obj_wsum, t->obj_wroot)) return kStoveInvalidValue;
  return 0;
}
inline int bg_tables(const StoveSpnTables* t) {
  if (t == nullptr || null_any(t->bg_side, t->bg_coef, t->bg_wroot)) return kStoveInvalidValue;
  return 0;
}
inline int table_grads(const StoveSpnTableGrads* g, bool obj, bool bg) {
  if (g == nullptr) return kStoveInvalidValue;
  if (obj && null_any(g->obj_coef, g->obj_wsum, g->obj_wroot)) return kStoveInvalidValue;
  if (bg && null_any(g->bg_coef, g->bg_wroot)) return kStoveInvalidValue;
  return 0;
}

// ---- RatSpn operator (stove_objspn_*, stove_bgspn_*); n == 0 is a valid empty call (the forward returns at once)
inline int objspn_fwd(const StoveSpnTables* t, const float* inputs, const float* xw, const float* out, int n) {
  if (n < 0) return kStoveInvalidValue;
  if (n == 0) return 0;
  if (obj_tables(t) || null_any(inputs, xw, out)) return kStoveInvalidValue;
  return 0;
}
inline int objspn_bwd(const StoveSpnTables* t, const float* marg, const float* xw, const float* out, const float* dout,
                      const float* d_marg, const StoveSpnTableGrads* g, const void* ws, int n) {
  if (n < 0) return kStoveInvalidValue;
  // (n == 0 is a valid call that overwrites the table gradients with zeros: everything but the per-sample arrays is still needed)
  if (obj_tables(t) || t->obj_leaf_slot == nullptr || ws == nullptr || table_grads(g, true, false)) return kStoveInvalidValue;
  if (n == 0) return 0;
  if (null_any(xw, out, dout)) return kStoveInvalidValue;
  if (d_marg != nullptr && marg == nullptr) return kStoveInvalidValue;
  return 0;
}
inline int bgspn_fwd(const StoveSpnTables* t, const float* inputs, const float* ell, const float* out, int n, int n_pix) {
  if (n < 0 || n_pix < 1) return kStoveInvalidValue;
  if (n == 0) return 0;
  if (bg_tables(t) || null_any(inputs, ell, out)) return kStoveInvalidValue;
  return 0;
}
inline int bgspn_bwd(const StoveSpnTables* t, const float* inputs, const float* marg, const float* ell, const float* out, const float* dout,
                     const float* d_marg, const StoveSpnTableGrads* g, const void* ws, int n, int n_pix) {
  if (n < 0 || n_pix < 1) return kStoveInvalidValue;
  if (bg_tables(t) || ws == nullptr || table_grads(g, false, true)) return kStoveInvalidValue;
  if (n == 0) return 0;
  if (null_any(inputs, ell, out, dout)) return kStoveInvalidValue;
  if (d_marg != nullptr && marg == nullptr) return kStoveInvalidValue;
  return 0;
}

// ---- Supair.likelihood (stove_scene_*): frame map as stove_hip.h states it (0, 0 = dense)
inline int frame_map(int n_frames, int seq_frames, int seq_stride) {
  if (seq_frames == 0) return 0;
  if (seq_frames < 0 || seq_stride < seq_frames || n_frames % seq_frames != 0) return kStoveInvalidValue;
  return 0;
}
inline int scene_fwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride,
                     const float* ll, const float* saved) {
  if (n_frames < 0 || n_obj < 1 || n_obj > kMaxObjects || frame_map(n_frames, seq_frames, seq_stride)) return kStoveInvalidValue;
  if (n_frames == 0) return 0;
  if (obj_tables(t) || bg_tables(t) || null_any(frames, z, ll, saved)) return kStoveInvalidValue;
  return 0;
}
inline int scene_bwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride,
                     const float* saved, const float* dll, const float* dz, const StoveSpnTableGrads* g, const void* ws) {
  if (n_frames < 0 || n_obj < 1 || n_obj > kMaxObjects || frame_map(n_frames, seq_frames, seq_stride)) return kStoveInvalidValue;
  if (n_frames == 0) return 0;
  if (obj_tables(t) || t->obj_leaf_slot == nullptr || bg_tables(t) || null_any(frames, z, saved, dll, dz) || ws == nullptr ||
      table_grads(g, true, true))
    return kStoveInvalidValue;
  return 0;
}

// ---- the scene likelihood over colour channels (stove_scene_*_ch): object SPN of any shape over channels x pw x ph dimensions
// (the limits of stove_objspn_fwd_any), background tables [3][channels * W * H][6][3]
inline bool obj_any_bad(int R, int G, int S, int D, int Lmax) {
  return R < 1 || R > 8 || G < 1 || G > 16 || S < 1 || S > 16 || D < 4 || D > 1024 || Lmax < 1 || Lmax > D;
}
inline bool scene_ch_bad(int R, int G, int S, int D, int Lmax, size_t bg_coef_floats, int n_frames, int n_obj, int seq_frames, int seq_stride,
                        int channels, int W, int H, int pw, int ph) {
  if (n_frames < 0 || n_obj < 1 || n_obj > kMaxObjects || frame_map(n_frames, seq_frames, seq_stride)) return true;
  if (channels < 1 || channels > 4 || W < 2 || H < 2 || pw < 2 || ph < 2 || obj_any_bad(R, G, S, D, Lmax)) return true;
  return (long long)D != (long long)channels * pw * ph || bg_coef_floats != (size_t)3 * channels * W * H * 6 * 3;
}
inline int scene_ch_fwd(const int32_t* lscope, const float* coef, const float* wsum, const float* wroot, int R, int G, int S, int D, int Lmax,
                        const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats, const float* frames,
                        const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H, int pw, int ph,
                        const float* ll, const float* saved) {
  if (scene_ch_bad(R, G, S, D, Lmax, bg_coef_floats, n_frames, n_obj, seq_frames, seq_stride, channels, W, H, pw, ph)) return kStoveInvalidValue;
  if (n_frames == 0) return 0;
  if (lscope == nullptr || bg_side == nullptr || null_any(coef, wsum, wroot, bg_coef, bg_wroot, frames, z, ll, saved)) return kStoveInvalidValue;
  return 0;
}
inline int scene_ch_bwd(const int32_t* lscope, const int32_t* slot, const float* coef, const float* wsum, const float* wroot, int R, int G, int S,
                        int D, int Lmax, const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats,
                        const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H,
                        int pw, int ph, const float* saved, const float* dll, const float* dz, const float* g_coef, const float* g_wsum,
                        const float* g_wroot, const float* g_bg_coef, const float* g_bg_wroot, const void* ws) {
  if (scene_ch_bad(R, G, S, D, Lmax, bg_coef_floats, n_frames, n_obj, seq_frames, seq_stride, channels, W, H, pw, ph)) return kStoveInvalidValue;
  if (n_frames == 0) return 0;
  if (lscope == nullptr || slot == nullptr || bg_side == nullptr || ws == nullptr ||
      null_any(coef, wsum, wroot, bg_coef, bg_wroot, frames, z, saved, dll, dz, g_coef, g_wsum, g_wroot, g_bg_coef, g_bg_wroot))
    return kStoveInvalidValue;
  return 0;
}

// ---- Dynamics.forward (stove_gnn_*), the recursion (stove_dynloop_*), Stove.rollout: one check per operation, run with the limits
// of the kernels that serve the state-code length -- cl = 32 (csrc/gnn.hip, gnn_small*.hip) or 16 / 64 (stove_*_cl, csrc/gnn_cl.hip)
constexpr int kMaxObjectsCl = 6;
struct GnnLimits {
  int lo, hi, max_obj;        // state width cl / 2 <= sin_dim <= cl, N <= max_obj; hi == 0: no kernels for this width
  bool empty_bwd;             // an empty backward (B == 0 or Ts == 0) is checked here as the call that zeroes g_params; false: see gnn_bwd, dynloop_bwd
  bool bad(int B, int N, int sin_dim) const { return hi == 0 || B < 0 || N < 1 || N > max_obj || sin_dim < lo || sin_dim > hi; }
};
constexpr GnnLimits kGnn32{16, 32, kMaxObjects, false};
inline GnnLimits gnn_limits_cl(int cl) { return (cl == 16 || cl == 64) ? GnnLimits{cl / 2, cl, kMaxObjectsCl, true} : GnnLimits{0, 0, 0, true}; }

inline int gnn_fwd(const float* s_in, const float* params, const float* result, int B, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim)) return kStoveInvalidValue;
  if (B == 0) return 0;
  return null_any(s_in, params, result) ? kStoveInvalidValue : 0;
}
// (B == 0 zeroes g_params at every width; stove_gnn_bwd tests that pointer itself, ahead of this check)
inline int gnn_bwd(const float* s_in, const float* params, const float* d_result, const float* d_s_in, const float* g_params,
                   const void* ws, int B, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim) || (k.empty_bwd && g_params == nullptr)) return kStoveInvalidValue;
  if (B == 0) return 0;
  return (null_any(s_in, params, d_result, d_s_in, g_params) || ws == nullptr) ? kStoveInvalidValue : 0;
}
inline int dynloop_fwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                       const float* params, const float* z, const float* zdyn, const float* zdstd, const float* mean, const float* std_, int B,
                       int Ts, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim) || Ts < 0) return kStoveInvalidValue;
  if (B == 0 || Ts == 0) return 0;
  if (null_any(z1, zsup, zsstd, eps, params, z, zdyn, zdstd, mean, std_)) return kStoveInvalidValue;
  if (sin_dim > k.lo && extra == nullptr) return kStoveInvalidValue;
  return 0;
}
// An empty backward (B == 0 or Ts == 0): stove_dynloop_bwd has nothing to overwrite g_params with and refuses it; stove_dynloop_bwd_cl
// zeroes g_params, as stove_gnn_bwd_cl does.
inline int dynloop_bwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                       const float* params, const float* z, const float* dz1, const float* dzsup, const float* dzsstd, const float* dextra,
                       const float* g_params, const void* ws, int B, int Ts, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim) || Ts < 0 || g_params == nullptr) return kStoveInvalidValue;
  if (B == 0 || Ts == 0) return k.empty_bwd ? 0 : kStoveInvalidValue;
  if (null_any(z1, zsup, zsstd, eps, params, z, dz1, dzsup, dzsstd) || ws == nullptr) return kStoveInvalidValue;
  if (sin_dim > k.lo && (extra == nullptr || dextra == nullptr)) return kStoveInvalidValue;
  return 0;
}
inline int rollout_fwd(const float* z_last, const float* extra, const float* params, const float* z_pred, int B, int num,
                       int A, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim) || num < 0) return kStoveInvalidValue;
  if (B == 0 || num == 0) return 0;
  if (null_any(z_last, params, z_pred)) return kStoveInvalidValue;
  if (sin_dim > k.lo && (extra == nullptr || A < 1)) return kStoveInvalidValue;
  return 0;
}
// the sampling rollout: the mean rollout's contract plus the draws and their log-density, both required
inline int rollout_sample_fwd(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                              const float* log_q, int B, int num, int A, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (const int rc = rollout_fwd(z_last, extra, params, z_pred, B, num, A, N, sin_dim, k)) return rc;
  if (B == 0 || num == 0) return 0;
  return null_any(eps, log_q) ? kStoveInvalidValue : 0;
}
// the backward of either rollout (eps == NULL: the mean rollout).  g_params, and d_z_last / d_extra where they have elements, are
// overwritten even by an empty call (B == 0 or num == 0: zeros), so they are required throughout; of the upstream gradients d_z_pred
// and d_pred may be NULL, d_log_q too but only a sampling call (eps) can have one.  d_extra is NULL exactly when extra is.
inline int rollout_bwd(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                       const float* d_log_q, const float* d_z_last, const float* d_extra, const float* g_params, const void* ws, int B,
                       int num, int A, int N, int sin_dim, const GnnLimits& k = kGnn32) {
  if (k.bad(B, N, sin_dim) || num < 0 || g_params == nullptr) return kStoveInvalidValue;
  if (d_log_q != nullptr && eps == nullptr) return kStoveInvalidValue;
  if ((extra == nullptr) != (d_extra == nullptr)) return kStoveInvalidValue;
  if (sin_dim > k.lo && (extra == nullptr || A < 1)) return kStoveInvalidValue;
  if (B == 0) return 0;
  if (d_z_last == nullptr) return kStoveInvalidValue;
  if (num == 0) return 0;
  return (null_any(z_last, params, z_pred) || ws == nullptr) ? kStoveInvalidValue : 0;
}

// ---- the state-supervised baseline (stove_sup_*, csrc/gnn_sup.hip): V observed frames of N objects, R predicted ones, on the
// width-generic core (cl = 16 / 64, N <= 6).  B == 0 is a valid empty rollout (the backward then zeroes g_params); codes and d_latent0
// are optional; the loss has no empty call (a mean over nothing).
inline bool sup_dims_bad(int cl, int B, int V, int R, int N) {
  if (gnn_limits_cl(cl).bad(B, N, cl) || V < 1 || R < 1) return true;
  return (long long)V + R - 1 > 0x7fffffffLL;        // (the number of steps is an int)
}
inline int sup_rollout_fwd(const float* x, const float* latent0, const float* params, const float* pred, int cl, int B, int V, int R, int N) {
  if (sup_dims_bad(cl, B, V, R, N)) return kStoveInvalidValue;
  if (B == 0) return 0;
  return null_any(x, latent0, params, pred) ? kStoveInvalidValue : 0;
}
inline int sup_rollout_bwd(const float* x, const float* params, const float* codes, const float* d_pred, const float* g_params,
                           const void* ws, int cl, int B, int V, int R, int N) {
  if (sup_dims_bad(cl, B, V, R, N) || g_params == nullptr) return kStoveInvalidValue;
  if (B == 0) return 0;
  return (null_any(x, params, codes, d_pred) || ws == nullptr) ? kStoveInvalidValue : 0;
}
inline int sup_loss(const float* pred, const float* future, const float* losses, const float* d_pred, int B, int R, int N, int end) {
  if (B < 1 || R < 1 || N < 1 || N > kMaxObjectsCl || (end != 2 && end != 4)) return kStoveInvalidValue;
  if ((long long)B * R * N * 4 > 0x7fffffffLL) return kStoveInvalidValue;          // (the entries are counted in int)
  return null_any(pred, future, losses, d_pred) ? kStoveInvalidValue : 0;
}

// ---- stove_plan_expand: one expansion of M search trees (csrc/plan.hip).  Everything the host can see; the indices themselves
// (leaf, child, len_s, acts) are device memory and are checked by the kernels.  The rollout behind it is the one of the state-code
// length: `k` = kGnn32 (stove_plan_expand) or gnn_limits_cl(cl) (stove_plan_expand_cl: cl = 16 / 64, N <= 6); a node's input row
// [state cl/2 | action embedding 4 | appearance] has to fit cl, so app_dim <= cl/2 - 4.
constexpr int kPlanMaxActions = 64;
inline bool plan_dims_bad(int M, int A, int L, int N, int app_dim, const GnnLimits& k = kGnn32) {
  if (M < 1 || A < 1 || L < 1 || A > kPlanMaxActions || app_dim < 0 || k.bad(1, N, k.lo + 4 + app_dim)) return true;
  return (long long)M * A * (1 + (long long)L) > 0x7fffffffLL / (k.max_obj * k.hi);        // rows x steps x objects x cl stays an int
}
inline int plan_expand(const float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app, const int* acts,
                       const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, const float* q,
                       const void* ws, int M, int cap, int A, int L, int D, int N, int app_dim, const GnnLimits& k = kGnn32) {
  if (plan_dims_bad(M, A, L, N, app_dim, k) || D < 1 || cap < 1 + A) return kStoveInvalidValue;
  if (null_any(z_pool, emb_w, emb_b, gnn_params, rh_params, q) || null_any(leaf, child, len_s, acts) || ws == nullptr) return kStoveInvalidValue;
  if (app_dim > 0 && app == nullptr) return kStoveInvalidValue;
  return 0;
}

// ---- stove_plan_search: R iterations of select / expand / backpropagate on device-resident trees (csrc/plan_tree.hip).  What
// plan_expand rejects, plus the tree arrays; sel_trace is optional, R == 0 a valid call (only `action` is written; acts may be NULL).  The arrays'
// contents are device memory and are checked by the kernels (status).
inline int plan_search(const float* z_pool, const int* first, const int* parent, const int* depth, const int* Ns, const int* Nsa,
                       const double* Qsa, const int* used, const double* min_gap, const int* status, const int* action, const float* app,
                       const int* acts, const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params,
                       const void* ws, int M, int cap, int A, int L, int D, int N, int app_dim, int R, const GnnLimits& k = kGnn32) {
  if (plan_dims_bad(M, A, L, N, app_dim, k) || D < 1 || cap < 1 + A || R < 0) return kStoveInvalidValue;
  if (null_any(z_pool, emb_w, emb_b, gnn_params, rh_params) || null_any(first, parent, depth, Ns, Nsa, used, status, action) ||
      null_any(Qsa, min_gap) || ws == nullptr || (R > 0 && acts == nullptr))
    return kStoveInvalidValue;
  if (app_dim > 0 && app == nullptr) return kStoveInvalidValue;
  return 0;
}

// ---- stove_render_frames_any: frames of C x W x H pixels from glimpses of C x pw x ph (csrc/render.hip).  n_frames == 0 is a valid empty
// call; truth and sqerr come together; one of out / sqerr is wanted.  The frame and the patch set are indexed with ints.
inline int render_any(const float* bg, const float* patches, int frames_per_patch, const float* z, const float* truth, const float* out,
                      const float* sqerr, int n_frames, int n_obj, int C, int W, int H, int pw, int ph) {
  if (n_frames < 0 || n_obj < 1 || n_obj > kMaxObjects || C < 1 || C > 4 || W < 1 || H < 1 || pw < 1 || ph < 1 || frames_per_patch < 0)
    return kStoveInvalidValue;
  if (n_frames == 0) return 0;          // (arrays without elements have no address)
  if ((truth == nullptr) != (sqerr == nullptr) || (out == nullptr && sqerr == nullptr) || null_any(bg, patches, z)) return kStoveInvalidValue;
  if ((long long)C * W * H > 0x3fffffffLL || (long long)kMaxObjects * C * pw * ph > 0x3fffffffLL) return kStoveInvalidValue;
  return 0;
}

// ---- stove_env_step: M environments of N balls stepped (and rendered at res x res) in place (csrc/env.hip).  M == 0 is a valid empty
// call; action and frames are optional.  The action indices are device memory and are checked by the kernel (status).
constexpr int kEnvMaxObjects = 6;
inline int env_step(const double* x, const double* v, const double* r, const double* m, const int* collisions, const int* status, int M,
                    int N, int granularity, int res) {
  if (M < 0 || N < 1 || N > kEnvMaxObjects || granularity < 1 || res < 1) return kStoveInvalidValue;
  if (M == 0) return 0;          // (arrays without elements have no address)
  return (null_any(x, v, r, m) || null_any(collisions, status)) ? kStoveInvalidValue : 0;
}

// ---- stove_env_sequences: B whole sequences of T steps of N balls, billiards (kind 0) or gravity (kind 1), every state and frame written
// out (csrc/env_sequences.hip).  B == 0 is a valid empty call; actions and frames are optional, and gravity takes no actions.  The action
// indices are device memory and are checked by the kernel (status).
inline int env_sequences(const double* x0, const double* v0, const double* r, const double* m, const int* actions, const double* y,
                         const int* collisions, const int* in_bounds, const int* status, int B, int N, int T, int granularity, int res,
                         int kind) {
  if (B < 0 || N < 1 || N > kEnvMaxObjects || T < 1 || granularity < 1 || res < 1 || kind < 0 || kind > 1) return kStoveInvalidValue;
  if (kind == 1 && actions != nullptr) return kStoveInvalidValue;
  if ((long long)res * res > 0x0fffffffLL) return kStoveInvalidValue;          // (a frame's pixels are counted in int)
  if (B == 0) return 0;          // (arrays without elements have no address)
  return (null_any(x0, v0, r, m, y) || null_any(collisions, in_bounds, status)) ? kStoveInvalidValue : 0;
}

// ---- stove_env_draw_starts: the starts and, with `actions`, the action rows of B sequences of N balls drawn on the device
// (csrc/env_draw.hip).  B == 0 is a valid empty call; actions is optional, and with T == 0 nothing of it is written.
inline int env_draw_starts(const double* r, const double* x0, const double* v0, const int* tries, const int* status, int B, int N, int T,
                           int kind, int max_tries) {
  if (B < 0 || N < 1 || N > kEnvMaxObjects || T < 0 || kind < 0 || kind > 1 || max_tries < 1) return kStoveInvalidValue;
  if (B == 0) return 0;          // (arrays without elements have no address)
  return (null_any(r, x0, v0) || null_any(tries, status)) ? kStoveInvalidValue : 0;
}

// ---- stove_env_search: R trees per environment searched on M environments of N balls (csrc/env_search.hip).  M == 0 is a valid empty
// call, and so is runs == 0 (only `action` is written; draws may be NULL).  The table and the trees are device memory and are checked
// by the kernel (status).
constexpr int kEnvActions = 9;
inline int env_search(const double* x, const double* v, const double* r, const double* m, const int* draws, const int* first,
                      const int* parent, const int* depth, const int* Ns, const int* Nsa, const double* Qsa, const int* used,
                      const double* min_gap, const int* status, const int* action, int M, int R, int N, int D, int runs, int cap,
                      int granularity) {
  if (M < 0 || R < 1 || N < 1 || N > kEnvMaxObjects || D < 2 || runs < 0 || cap < 1 + kEnvActions || granularity < 1)
    return kStoveInvalidValue;
  if ((long long)M * R > 0x7fffffffLL || (long long)runs * D > 0x7fffffffLL) return kStoveInvalidValue;
  if (M == 0) return 0;          // (arrays without elements have no address)
  if (null_any(x, v, r, m) || null_any(first, parent, depth, Ns, Nsa, used, status, action) || null_any(Qsa, min_gap) ||
      (runs > 0 && draws == nullptr))
    return kStoveInvalidValue;
  return 0;
}

// ---- stove_ppo_collect: S steps of B environments of N balls under a policy of head width H (csrc/ppo_collect.hip).  B == 0 is a valid
// empty call; with S == 0 only obs (B, 1, 4N), next_value and status are written and the (B, S) arrays may be NULL.  Everything the
// pointers name is device memory: a non-finite policy output is found by the kernel (status).
constexpr int kPpoMaxHidden = 128;
inline int ppo_collect(const double* x, const double* v, const double* r, const double* m, const float* params, const float* u,
                       const float* obs, const int* actions, const float* rewards, const float* values, const float* logp,
                       const float* next_value, const float* returns, const int* status, int B, int S, int N, int H, int granularity) {
  if (B < 0 || S < 0 || N < 1 || N > kEnvMaxObjects || H < 1 || H > kPpoMaxHidden || granularity < 1) return kStoveInvalidValue;
  if ((long long)B * ((long long)S + 1) * 4 * N > 0x7fffffffLL) return kStoveInvalidValue;
  if (B == 0) return 0;          // (arrays without elements have no address)
  if (null_any(x, v, r, m) || null_any(params, obs, next_value) || status == nullptr) return kStoveInvalidValue;
  if (S > 0 && (null_any(u, rewards, values, logp, returns) || actions == nullptr)) return kStoveInvalidValue;
  return 0;
}

// ---- stove_ppo_collect_model: S imagined steps of B trajectories of N objects on the cl = 32 action-conditioned model under a policy of
// head width H (csrc/ppo_model.hip).  B == 0 is a valid empty call; with S == 0 only obs (B, 1, 4N), next_value and status are written
// and the (B, S) arrays and z_pred may be NULL.  pred is optional, app is required where app_dim > 0.  The state width 20 + app_dim
// stays within 32, as for stove_plan_expand; 0 <= lim_enc <= 32.
inline int ppo_collect_model(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                             const float* gnn_params, const float* rh_params, const float* u, const float* z_pred, const float* obs,
                             const int* actions, const float* rewards, const float* values, const float* logp, const float* next_value,
                             const float* returns, const int* status, int B, int S, int N, int H, int app_dim, int lim_enc) {
  if (B < 0 || S < 0 || N < 1 || N > kEnvMaxObjects || H < 1 || H > kPpoMaxHidden || app_dim < 0 || 20 + app_dim > 32 || lim_enc < 0 ||
      lim_enc > 32)
    return kStoveInvalidValue;
  if ((long long)B * ((long long)S + 1) * N * 32 > 0x7fffffffLL) return kStoveInvalidValue;
  if (B == 0) return 0;          // (arrays without elements have no address)
  if (null_any(z0, policy_params, emb_w, emb_b, gnn_params, rh_params, obs, next_value) || status == nullptr) return kStoveInvalidValue;
  if (app_dim > 0 && app == nullptr) return kStoveInvalidValue;
  if (S > 0 && (null_any(u, z_pred, rewards, values, logp, returns) || actions == nullptr)) return kStoveInvalidValue;
  return 0;
}
// ---- stove_ppo_collect_model_cl: the same call on a model of state-code length cl = 16 / 64 (csrc/ppo_model_cl.hip), `k` =
// gnn_limits_cl(cl): any other cl (32 included: it has the entry point above) has no limits and is refused.  A node's input row [state
// cl/2 | action embedding 4 | appearance] has to fit cl, so app_dim <= cl/2 - 4; 0 <= lim_enc <= cl; N <= 6 on both counts.
inline int ppo_collect_model_cl(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                                const float* gnn_params, const float* rh_params, const float* u, const float* z_pred, const float* obs,
                                const int* actions, const float* rewards, const float* values, const float* logp, const float* next_value,
                                const float* returns, const int* status, int B, int S, int N, int H, int app_dim, int lim_enc,
                                const GnnLimits& k) {
  if (S < 0 || N > kEnvMaxObjects || H < 1 || H > kPpoMaxHidden || app_dim < 0 || app_dim > k.hi || k.bad(B, N, k.lo + 4 + app_dim) ||
      lim_enc < 0 || lim_enc > k.hi)
    return kStoveInvalidValue;
  if ((long long)B * ((long long)S + 1) * N * k.hi > 0x7fffffffLL) return kStoveInvalidValue;
  if (B == 0) return 0;          // (arrays without elements have no address)
  if (null_any(z0, policy_params, emb_w, emb_b, gnn_params, rh_params, obs, next_value) || status == nullptr) return kStoveInvalidValue;
  if (app_dim > 0 && app == nullptr) return kStoveInvalidValue;
  if (S > 0 && (null_any(u, z_pred, rewards, values, logp, returns) || actions == nullptr)) return kStoveInvalidValue;
  return 0;
}

// ---- stove_ppo_collect_images: `warm` warm-up steps and S steps of B environments of N balls under the image policy of F stacked
// frames and head width H (csrc/ppo_image.hip).  B == 0 is a valid empty call; with S == 0 only the first window frames (B, F, 3, 32, 32),
// next_value and status are written and the (B, S) arrays may be NULL.
constexpr int kImgMaxFrames = 4, kImgMaxHidden = 512;
inline int ppo_collect_images(const double* x, const double* v, const double* r, const double* m, const float* params, const float* u,
                              const float* frames, const int* actions, const float* rewards, const float* values, const float* logp,
                              const float* next_value, const float* returns, const int* status, int B, int S, int N, int F, int H, int warm,
                              int granularity) {
  if (B < 0 || S < 0 || N < 1 || N > kEnvMaxObjects || F < 1 || F > kImgMaxFrames || H < 1 || H > kImgMaxHidden || warm < 1 || granularity < 1)
    return kStoveInvalidValue;
  if ((long long)B * ((long long)S + F) > 0x7fffffffLL) return kStoveInvalidValue;
  if (B == 0) return 0;          // (arrays without elements have no address)
  if (null_any(x, v, r, m) || null_any(params, frames, next_value) || status == nullptr) return kStoveInvalidValue;
  if (S > 0 && (null_any(u, rewards, values, logp, returns) || actions == nullptr)) return kStoveInvalidValue;
  return 0;
}

// ---- stove_ppo_update: up to max_steps of E x M optimiser steps on n collected rows (csrc/ppo_update.hip).  E == 0 and max_steps == 0
// are valid empty calls (one launch that writes status only).  Everything the pointers name is device memory: the indices of perm and
// the actions are checked by the kernel (status 2), a non-finite loss or norm is found there too (status 3).
inline int ppo_update(const float* params, const float* m, const float* v, const int* step, const float* obs, const int* actions,
                      const float* returns, const float* values, const float* logp, const float* adv, const int* perm, const float* losses,
                      const float* gnorm, const int* status, int n, int E, int M, int max_steps, int N, int H) {
  if (N < 1 || N > kEnvMaxObjects || H < 1 || H > kPpoMaxHidden || M < 1 || n < M || E < 0 || max_steps < 0) return kStoveInvalidValue;
  if ((long long)max_steps > (long long)E * M || (long long)E * n > 0x7fffffffLL || (long long)n * 4 * N > 0x7fffffffLL) return kStoveInvalidValue;
  if (null_any(params, m, v, obs, returns, values, logp, adv, losses, gnorm) || null_any(step, actions, perm, status)) return kStoveInvalidValue;
  return 0;
}

// ---- stove_ppo_update_images: up to max_steps of E x M optimiser steps of the image policy on n rows whose observations are windows
// of 3072 F floats at obs + (r / S) env_stride + (r % S) 3072 (csrc/ppo_image_update.hip).  E M == 0 and max_steps == 0 are valid empty
// calls (status alone is written; every other array and ws may then be NULL).  grad may be NULL.  Indices, actions and non-finite
// losses are the kernels' to find (status 2, 3).
inline int ppo_update_images(const float* params, const float* m, const float* v, const int* step, const float* obs, const int* actions,
                             const float* returns, const float* values, const float* logp, const float* adv, const int* perm,
                             const float* losses, const float* gnorm, const int* status, const void* ws, int n, int S, int env_stride, int E,
                             int M, int max_steps, int F, int H) {
  if (F < 1 || F > kImgMaxFrames || H < 1 || H > kImgMaxHidden || M < 1 || n < M || S < 1 || E < 0 || max_steps < 0 || env_stride < 0)
    return kStoveInvalidValue;
  if ((long long)max_steps > (long long)E * M || (long long)E * n > 0x7fffffffLL || (long long)n * 225 > 0x7fffffffLL) return kStoveInvalidValue;
  if (status == nullptr) return kStoveInvalidValue;
  if (max_steps == 0) return 0;
  if (null_any(params, m, v, obs, returns, values, logp, adv, losses, gnorm) || null_any(step, actions, perm) || ws == nullptr)
    return kStoveInvalidValue;
  return 0;
}

// ---- stove_gemm_bf16: C (M x N) = A (M x K) B^T (N x K) [+ bias + add]; leading dimensions cover their rows, B float4-addressable
inline int gemm(const float* A, const float* B, const float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor,
                int nsplit, int splitk, const float* ws) {
  if (M < 0 || N < 0) return kStoveInvalidValue;
  if (M == 0 || N == 0) return 0;
  if (K <= 0 || splitk < 1 || nsplit < 1 || nsplit > 3) return kStoveInvalidValue;
  if (null_any(A, B, C)) return kStoveInvalidValue;
  if (lda < (a_kmajor ? M : K) || ldb < (b_kmajor ? N : K) || ldc < N) return kStoveInvalidValue;
  if (misaligned16(B) || (ldb & 3) != 0 || ((b_kmajor ? N : K) & 3) != 0) return kStoveInvalidValue;
  if (splitk > 1 && (ws == nullptr || ldc != N)) return kStoveInvalidValue;
  return 0;
}

}  // namespace stove_validate
