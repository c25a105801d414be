// C ABI of libstove_hip.so (see include/stove_hip.h).  Single translation unit: the kernel
// files are included here so every launch sees its kernel without relocatable device code.
#include "../../include/stove_hip.h"
#include <algorithm>

#include "common.h"
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <atomic>
#include <type_traits>
#include "validate.h"
// argument checks shared with the sanitizer-built host driver (csrc/validate.h, tests/abi/validate_driver.cpp)
static_assert(stove_validate::kStoveInvalidValue == (int)hipErrorInvalidValue, "validate.h returns hipErrorInvalidValue");
#define STOVE_VALIDATE(expr)                      \
  do {                                            \
    const int v__ = stove_validate::expr;         \
    if (v__) return v__;                          \
  } while (0)
#include "spn_obj.hip"
#include "spn_obj_generic.hip"
#include "spn_bg.hip"
#include "spn_bg_generic.hip"
#include "scene.hip"
#include "scene_fused.hip"
#include "scene_colour.hip"
#include "gnn.hip"
#include "match.hip"
#include "gnn_small.hip"
#include "gnn_small_bwd.hip"
#include "gnn_cl.hip"
#include "gnn_sup.hip"
#include "lstm.hip"
#include "arena.hip"
#include "state.hip"
#include "gemm_bf16.hip"
#include "head_fused.hip"
#include "reward_head.hip"
#include "plan.hip"
#include "plan_tree.hip"
#include "render.hip"
#include "env.hip"
#include "env_sequences.hip"
#include "env_draw.hip"
#include "env_search.hip"
#include "ppo_collect.hip"
#include "ppo_model.hip"
#include "ppo_model_cl.hip"
#include "ppo_update.hip"
#include "ppo_image.hip"
#include "ppo_image_update.hip"

namespace stove {

__global__ void wave_sum_test_k(const float* __restrict__ in, float* __restrict__ out) {
  const int w = blockIdx.x * (blockDim.x >> 6) + wave_id();
  const float v = in[(size_t)w * 64 + lane_id()];
  const float s = wave_sum(v);
  out[(size_t)w * 64 + lane_id()] = s;
}

// tile [nb][100][2][64] -> patches (n,100), keep (n,100)
__global__ void tile_unpack_k(const float* __restrict__ tile, float* __restrict__ patches, float* __restrict__ keep,
                              int n, int n_batches) {
  const int total = n_batches * kPD * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int lane = i & 63, p = (i >> 6) % kPD, b = i / (64 * kPD);
    const int smp = b * 64 + lane;
    if (smp >= n) continue;
    const float* t = tile + ((size_t)b * kPD + p) * 2 * 64;
    if (patches) patches[(size_t)smp * kPD + p] = t[lane];
    if (keep) keep[(size_t)smp * kPD + p] = t[64 + lane];
  }
}

// which glimpse-tile kernel the scene forward runs: 1 (default) = lane per PIXEL with the tile transposed through LDS up to three
// objects, lane per glimpse beyond (28 % more VALU instructions in the transposing kernel -- 36 of 64 lanes idle in its second pass --
// which the VALU-bound six-object scene phase pays for: 5.45 against 5.42 ms per step); 0 = lane per glimpse always; 2 = lane per
// pixel always (the tests compare the two bit for bit at every object count)
static std::atomic<int> g_tile_lds{1};
static inline bool tile_transposed(int n_obj) {
  const int m = g_tile_lds.load();
  return m == 2 || (m == 1 && n_obj <= 3);
}
// ANY: the frame size / sampling convention at run time from `gm` (stove_scene_fwd_any); otherwise the tuned path's constants
template <int NMAX, bool ANY = false>
static int scene_tile_fwd(const float* frames, const float* z, float* xw, int n_obj, int np, hipStream_t st, FrameMap fm, SceneGeom gm = SceneGeom{}) {
  const int nb = (np + 63) / 64;
  const int grid = nb < 8192 ? nb : 8192;          // one workgroup per batch of 64 glimpses
  if (tile_transposed(n_obj)) {          // lane = pixel, tile transposed through LDS (scene_tile_fwd_t_k)
    STOVE_LAUNCH((scene_tile_fwd_t_k<NMAX, ANY>), dim3(grid), dim3(64 * kTileTWaves), 0, st, frames, z, xw, n_obj, np, nb, fm, gm);
    STOVE_LAUNCH_CHECK();
    return 0;
  }
  STOVE_LAUNCH((scene_tile_fwd_k<NMAX, ANY>), dim3(grid), dim3(256), 0, st, frames, z, xw, n_obj, np, nb, fm, gm);
  STOVE_LAUNCH_CHECK();
  return 0;
}
// SceneGeom of a W x H frame under either sampling convention of affine_grid / grid_sample (common.h)
static SceneGeom scene_geom(int W, int H, int align_corners) {
  SceneGeom g;
  g.W = W; g.H = H;
  g.cx = 0.5f * (W - 1); g.cy = 0.5f * (H - 1);
  if (align_corners) {
    g.pa = 2.0f / (kPatch - 1); g.pb = -1.0f;
    g.sxa = 0.5f * (W - 1); g.sya = 0.5f * (H - 1);
    g.fax = 2.0f / (W - 1); g.fbx = -1.0f; g.fay = 2.0f / (H - 1); g.fby = -1.0f;
  } else {
    g.pa = 2.0f / kPatch; g.pb = 1.0f / kPatch - 1.0f;
    g.sxa = 0.5f * W; g.sya = 0.5f * H;
    g.fax = 2.0f / W; g.fbx = 1.0f / W - 1.0f; g.fay = 2.0f / H; g.fby = 1.0f / H - 1.0f;
  }
  return g;
}

static inline int nmax_of(int n_obj) { return n_obj <= 3 ? 3 : (n_obj <= 6 ? 6 : 8); }

// The object-count ladder of the kernel templates: f(std::integral_constant<int, NMAX>) with the smallest NMAX of 3 / 6 / 8 that holds
// `n` objects (n may be an NMAX already: nmax_of, nmax_ch).  SIX = false: 3 / 8, for the kernels without a six-object instantiation
// (bg_mask_bwd_any_k, the colour kernels) -- the ladder is what instantiates them, so it must not name one.
template <bool SIX = true, class F>
static int with_nmax(int n, F f) {
  if (n <= 3) return f(std::integral_constant<int, 3>{});
  if constexpr (SIX) {
    if (n <= 6) return f(std::integral_constant<int, 6>{});
  }
  if (n <= 8) return f(std::integral_constant<int, 8>{});
  return (int)hipErrorInvalidValue;
}

// The other run-time choices that are template parameters of kernels (the GNN dynamics core), handed over the same way.  A ladder
// names exactly the instantiations that exist: what it passes to f is compiled.
template <int V>
using Int = std::integral_constant<int, V>;
template <class F>
static int with_flag(bool b, F f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(Int<n>) for a count n of 1 .. MAX that is a template parameter itself (env_search_k's objects)
template <int MAX, class F>
static int with_count(int n, F f) {
  if (n == MAX) return f(Int<MAX>{});
  if constexpr (MAX > 1) return with_count<MAX - 1>(n, f);
  return (int)hipErrorInvalidValue;
}
// f(NMX, ELU, NT) for a small graph of N objects: NMX = 4 / 6, the kernels built for up to four objects and up to six, NT = N where the count is a compile-time constant of the kernel
// (three objects; six where the kernel has that instantiation, SIX, and the call can use it, `six`), else 0.
template <bool SIX, class F>
static int with_small_graph(int N, bool elu, bool six, F f) {
  return with_flag(elu, [&](auto e) {
    if (N == 3) return f(Int<4>{}, e, Int<3>{});
    if (N <= 4) return f(Int<4>{}, e, Int<0>{});
    if constexpr (SIX) {
      if (N == 6 && six) return f(Int<6>{}, e, Int<6>{});
    }
    return f(Int<6>{}, e, Int<0>{});
  });
}

__global__ void fill_words_k(uint32_t* __restrict__ p, uint32_t v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

static inline size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

}  // namespace stove

using namespace stove;

extern "C" {

// 2: the GNN parameter image carries the LDS-order weight sections ([W | W^T | vectors | W packed | W^T packed],
//    stove_gnn_param_floats() floats); the measurement switches are explicit setters (stove_set_overlap,
//    ...) instead of environment reads; cross-capture events are owned by the caller
//    (stove_event_list_*).
// 3: stove_profile_report lines carry a fourth column, the time the kernel's launches cover.
// 4 (round 5): stove_gemm_bf16 takes nsplit = 3 (half pieces); the A/B entry points whose losing side is recorded are gone
//    (stove_set_tablegrad_placement, stove_lstm_cell_bwd_rows).
// 5: the scene likelihood and the object SPN for any frame size, glimpse size and vector widths (stove_scene_*_any,
//    stove_objspn_*_any), the fixed-Gaussian debug models (stove_gauss_ll_*), stove_scene_bwd_from.
// 6: the scene likelihood over 1 to 4 colour channels (stove_scene_saved_floats_ch, stove_scene_bwd_ws_bytes_ch, stove_scene_fwd_ch,
//    stove_scene_bwd_ch).
// 7: the GNN step, the inference recursion and the rollout at state-code lengths 16 and 64 (stove_gnn_param_floats_cl,
//    stove_gnn_grad_floats_cl, stove_gnn_bwd_ws_bytes_cl, stove_gnn_fwd_cl, stove_gnn_bwd_cl, stove_dynloop_fwd_cl, stove_dynloop_bwd_cl,
//    stove_rollout_fwd_cl).
//    (added since, nothing changed: stove_rollout_sample_fwd, stove_rollout_sample_fwd_cl -- the sampling rollout;
//     stove_plan_expand_ws_bytes, stove_plan_expand -- one expansion of a batch of search trees;
//     stove_rollout_bwd_ws_bytes, stove_rollout_bwd and their _cl siblings -- the backward of both rollouts;
//     stove_plan_search_ws_bytes, stove_plan_search -- a whole search of a batch of trees, the trees on the device;
//     stove_env_step -- a batch of avoidance / billiards environments stepped and rendered in place (env.hip);
//     stove_env_search -- tree search on those environments themselves, one launch per planning step (env_search.hip);
//     stove_env_sequences -- whole training sequences, billiards or gravity, every state and frame in one launch (env_sequences.hip);
//     stove_env_draw_starts -- their starts and action rows, drawn from a counter-based stream in one launch (env_draw.hip);
//     stove_render_frames_any -- frames of any size and channel count, with the squared pixel error fused in;
//     stove_ppo_param_floats, stove_ppo_collect -- the PPO arm: a batch of trajectories on states in one launch (ppo_collect.hip);
//     stove_ppo_update -- its update, every epoch and mini-batch in one launch (ppo_update.hip);
//     stove_ppo_collect_model -- the model-based PPO arm: a batch of imagined trajectories in one launch (ppo_model.hip);
//     stove_ppo_collect_model_cl -- the same on models of state-code length 16 and 64 (ppo_model_cl.hip);
//     stove_ppo_image_param_floats, stove_ppo_collect_images -- the PPO arm on images: a batch of trajectories in one launch (ppo_image.hip);
//     stove_ppo_update_images_ws_bytes, stove_ppo_update_images -- its update, every epoch and mini-batch in one call (ppo_image_update.hip);
//     stove_sup_rollout_fwd, stove_sup_rollout_bwd_ws_bytes, stove_sup_rollout_bwd, stove_sup_loss -- the state-supervised baseline:
//     teacher-forced warm-up and rollout in one launch each way, and its discounted loss (gnn_sup.hip))
int stove_abi_version(void) { return 7; }

const char* stove_error_string(int code) { return hipGetErrorString((hipError_t)code); }

int stove_selftest_wave_sum(const float* in, float* out, int n_waves, void* stream) {
  if (n_waves % 4) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(wave_sum_test_k, dim3(n_waves / 4), dim3(256), 0, (hipStream_t)stream, in, out);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- object SPN operator
size_t stove_objspn_tile_floats(int n) { return (size_t)((n + 63) / 64) * kObjX; }

int stove_objspn_fwd(const StoveSpnTables* t, const float* inputs, const float* marg, float* xw, float* out, int n,
                     void* stream) {
  STOVE_VALIDATE(objspn_fwd(t, inputs, xw, out, n));
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc = objspn_tile_from_arrays(inputs, marg, xw, n, st);
  if (rc) return rc;
  return objspn_forward(xw, t->obj_scope, t->obj_coef, t->obj_wsum, t->obj_wroot, out, nullptr, n, st);
}

size_t stove_objspn_bwd_ws_bytes(int n) { return (objspn_bwd_ws_floats(n) + stove_objspn_tile_floats(n)) * sizeof(float); }

int stove_objspn_bwd(const StoveSpnTables* t, const float* marg, const float* xw, const float* out, const float* dout,
                     float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n, void* stream) {
  STOVE_VALIDATE(objspn_bwd(t, marg, xw, out, dout, d_marg, g, ws, n));
  hipStream_t st = (hipStream_t)stream;
  float* dxw = (float*)ws;
  float* rest = dxw + stove_objspn_tile_floats(n);
  int rc = objspn_backward(xw, t->obj_scope, t->obj_leaf_slot, t->obj_coef, t->obj_wsum, t->obj_wroot, out, dout, dxw,
                           g->obj_coef, g->obj_wsum, g->obj_wroot, rest, n, st);
  if (rc) return rc;
  if (d_inputs == nullptr && d_marg == nullptr) return 0;
  if (d_marg != nullptr && marg == nullptr) return (int)hipErrorInvalidValue;
  return objspn_tile_to_arrays(dxw, marg, d_inputs, d_marg, n, st);
}

// ---------------------------------------------------------------- background SPN operator
size_t stove_bgspn_saved_floats(int n) { return bgspn_fwd_ws_floats(n); }

int stove_bgspn_fwd(const StoveSpnTables* t, const float* inputs, const float* marg, float* ell, float* out, int n,
                    void* stream) {
  STOVE_VALIDATE(bgspn_fwd(t, inputs, ell, out, n, 1024));
  if (n == 0) return 0;
  return bgspn_forward(inputs, marg, nullptr, 0, t->bg_side, t->bg_coef, t->bg_wroot, ell, out, n, (hipStream_t)stream);
}

size_t stove_bgspn_bwd_ws_bytes(int n) { return bgspn_bwd_ws_floats(n) * sizeof(float); }

int stove_bgspn_bwd(const StoveSpnTables* t, const float* inputs, const float* marg, const float* ell, const float* out,
                    const float* dout, float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n,
                    void* stream) {
  STOVE_VALIDATE(bgspn_bwd(t, inputs, marg, ell, out, dout, d_marg, g, ws, n, 1024));
  return bgspn_backward(inputs, marg, nullptr, 0, t->bg_side, t->bg_coef, t->bg_wroot, ell, out, dout, d_inputs, d_marg,
                        nullptr, g->bg_coef, g->bg_wroot, (float*)ws, n, (hipStream_t)stream);
}

// the same operator for any number of input dimensions (frame sizes other than 32 x 32): csrc/spn_bg_generic.hip
size_t stove_bgspn_saved_floats_d(int n, int n_pix) { return bgspn_any_saved_floats(n, n_pix); }
int stove_bgspn_fwd_d(const StoveSpnTables* t, const float* inputs, const float* marg, float* ell, float* out, int n, int n_pix, void* stream) {
  STOVE_VALIDATE(bgspn_fwd(t, inputs, ell, out, n, n_pix));
  if (n == 0) return 0;
  return bgspn_any_forward(inputs, marg, t->bg_side, t->bg_coef, t->bg_wroot, ell, out, n, n_pix, (hipStream_t)stream);
}
size_t stove_bgspn_bwd_ws_bytes_d(int n, int n_pix) { return bgspn_any_bwd_ws_floats(n, n_pix) * sizeof(float); }
int stove_bgspn_bwd_d(const StoveSpnTables* t, const float* inputs, const float* marg, const float* ell, const float* out, const float* dout,
                      float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n, int n_pix, void* stream) {
  STOVE_VALIDATE(bgspn_bwd(t, inputs, marg, ell, out, dout, d_marg, g, ws, n, n_pix));
  return bgspn_any_backward(inputs, marg, t->bg_side, t->bg_coef, t->bg_wroot, ell, out, dout, d_inputs, d_marg, g->bg_coef, g->bg_wroot,
                            (float*)ws, n, n_pix, (hipStream_t)stream);
}

// ---------------------------------------------------------------- fused scene likelihood
// Internal fork stream (one per device, created on first use): the background-SPN chain of a scene call runs on it next
// to the object-SPN chain -- they are independent until the assemble / tail kernels -- and is joined back before the call
// returns, so callers see plain single-stream semantics.  STOVE_NO_OVERLAP=1 keeps everything on the caller's stream.
static hipStream_t g_fork_user[16] = {nullptr};
static bool g_fork_user_set[16] = {false};
static std::mutex g_fork_mu;

static std::atomic<int> g_overlap{1};            // stove_set_overlap

static hipStream_t scene_fork_stream(hipStream_t st) {
  static hipStream_t side[16] = {nullptr};
  if (!g_overlap.load(std::memory_order_relaxed)) return st;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return st;
  std::lock_guard<std::mutex> lock(g_fork_mu);    // backward is called from the autograd thread, forward from the main one
  if (g_fork_user_set[dev]) return g_fork_user[dev] != nullptr ? g_fork_user[dev] : st;      // the caller's stream (NULL: no fork at all)
  if (side[dev] == nullptr && hipStreamCreateWithFlags(&side[dev], hipStreamNonBlocking) != hipSuccess) return st;
  return side[dev];
}

// Measurement switch (explicit state instead of an environment read; default 1).
// overlap 0: the scene calls run their background-SPN chain on the call's stream (no internal fork at all).
int stove_set_tile_lds(int mode) {
  if (mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
  g_tile_lds.store(mode);
  return 0;
}

int stove_set_overlap(int on) {
  g_overlap.store(on != 0, std::memory_order_relaxed);
  return 0;
}
// The caller owns the fork stream of `device` from now on (the scene calls run their background-SPN chain on it, forked from and joined
// into the call's stream): stream != NULL -- use this one; NULL -- no internal fork, everything on the call's stream.
// restore_default != 0: back to the library-owned stream that is created on first use.
int stove_set_fork_stream(int device, void* stream, int restore_default) {
  if (device < 0 || device >= 16) return (int)hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(g_fork_mu);
  g_fork_user_set[device] = restore_default == 0;
  g_fork_user[device] = restore_default == 0 ? (hipStream_t)stream : nullptr;
  return 0;
}

static int frame_map(int n_frames, int seq_frames, int seq_stride, FrameMap* fm) {
  *fm = FrameMap{0, 0};
  if (seq_frames == 0) return 0;                                   // dense
  if (seq_frames < 0 || seq_stride < seq_frames || n_frames % seq_frames != 0) return (int)hipErrorInvalidValue;
  if (seq_stride != seq_frames) *fm = FrameMap{seq_frames, seq_stride};
  return 0;
}

}  // extern "C": the host side that the three scene pipelines share has templates

// The tuned 32 x 32 / 10 x 10 pipeline (stove_scene_fwd*, stove_scene_bwd*), the one for any frame size / sampling convention
// (stove_scene_*_any) and the one over 1 to 4 colour channels (stove_scene_*_ch) share what follows: the buffer layouts, the call
// context with the fork / join / parameter-stream protocol, and one skeleton each for the forward and the backward.
namespace stove {

// offsets of consecutive sections of one buffer, each a multiple of 64 floats long
struct Layout {
  size_t total = 0;
  size_t take(size_t floats) {
    const size_t at = total;
    total += align64(floats);
    return at;
  }
};

// saved = [ head | obj_ll (np) | ovl (np) | bg_out (nf) | bg_ell | bg_aux | obj_scratch ]
//   head: the xw tile (tuned, any size), or patches | marg | obj, the object SPN's saved activations (colour)
//   bg_aux: the box coverage tables (tuned), or the mask image (any size, colour; frames up to kBgTabMax a side keep none)
//   obj_scratch: the object-SPN backward scratch at unit gradient (tuned, any size; the section only exists / is only written when the
//   forward is asked for it: with_grad)
struct SceneSaved {
  size_t xw, patches, marg, obj, obj_ll, ovl, bg_out, bg_ell, bg_aux, obj_scratch, total;
};
static void scene_saved_shared(Layout& l, SceneSaved& s, size_t nf, size_t np, size_t bg_ell, size_t bg_aux) {
  s.obj_ll = l.take(np);
  s.ovl = l.take(np);
  s.bg_out = l.take(nf);
  s.bg_ell = l.take(bg_ell);
  s.bg_aux = l.take(bg_aux);
}
// tuned and any size: they differ in the two background sections
static SceneSaved scene_saved_layout(int nf, int n_obj, bool with_grad, size_t bg_ell, size_t bg_aux) {
  const size_t np = (size_t)nf * n_obj;
  Layout l;
  SceneSaved s{};
  s.xw = l.take(stove_objspn_tile_floats((int)np));
  scene_saved_shared(l, s, nf, np, bg_ell, bg_aux);
  s.obj_scratch = l.take(with_grad ? objspn_scratch_floats((int)np) : 0);
  s.total = l.total;
  return s;
}

// ws = [ d_obj (np) | d_ovl (np) | dzc (np*NMAX*4) | dz_bg (np*4) | d_patch | d_marg | obj | d_mask | bg ]
//   d_patch, d_marg: the glimpse gradients (colour only); obj: the object SPN's table-gradient chunk partials (tuned, any size) or its
//   backward workspace (colour); d_mask: the mask gradient (any size; colour: C planes); bg: the background operator's workspace
struct SceneWs {
  size_t d_obj, d_ovl, dzc, dz_bg, d_patch, d_marg, obj, d_mask, bg, total;
};
static SceneWs scene_ws_layout(size_t np, int nmax, size_t d_glimpse, size_t obj, size_t d_mask, size_t bg) {
  Layout l;
  SceneWs s;
  s.d_obj = l.take(np);
  s.d_ovl = l.take(np);
  s.dzc = l.take(np * nmax * 4);
  s.dz_bg = l.take(np * 4);
  s.d_patch = l.take(d_glimpse);
  s.d_marg = l.take(d_glimpse);
  s.obj = l.take(obj);
  s.d_mask = l.take(d_mask);
  s.bg = l.take(bg);
  s.total = l.total;
  return s;
}

// frames up to kBgTabMax a side: the background kernels form the mask themselves from per-frame coverage tables (spn_bg_generic.hip), no
// mask image is kept
static bool scene_any_inline(int W, int H) { return W <= kBgTabMax && H <= kBgTabMax; }

// One scene call: its inputs, buffers and streams.  The background-SPN chain runs on the fork stream `sb` next to the object chain on
// the call's stream `st` -- they are independent until the assemble / finalize kernels; the table gradients, which only feed the
// optimiser, may go to the caller's parameter stream `sp`.  The call owns the guards of both, so every exit path joins what it forked.
struct SceneCall {
  const float *frames, *z;
  int nf, n_obj, np;
  hipStream_t st, root, sp, sb;     // root: the stream the fork is ordered behind (stove_scene_fwd_from); sb: set by fork()
  FrameMap fm{0, 0};
  // the pipelines with the geometry at run time (geometry()); the tuned one leaves these as they are
  SceneGeom gm{};
  SceneBoxes boxes{nullptr, 0, SceneGeom{}};
  bool inl = false;                 // scene_any_inline: no mask image
  int plane = 0, channels = 1;      // pixels of one colour plane; the background SPN sees channels * plane dimensions
  SceneSaved L{};
  SceneWs W{};
  const float* saved = nullptr;
  float* ws = nullptr;
  JoinGuard jb, jp;                 // armed by fork()

  SceneCall(const float* frames_, const float* z_, int n_frames, int n_obj_, void* stream, void* fork_from = nullptr, void* param_stream = nullptr)
      : frames(frames_), z(z_), nf(n_frames), n_obj(n_obj_), np(n_frames * n_obj_), st((hipStream_t)stream),
        root(fork_from != nullptr ? (hipStream_t)fork_from : st), sp(param_stream != nullptr ? (hipStream_t)param_stream : st), sb(st),
        jb(st, st), jp(st, st) {}
  void geometry(int W_, int H_, int align_corners, int channels_) {
    gm = scene_geom(W_, H_, align_corners);
    inl = scene_any_inline(W_, H_);
    boxes.z = inl ? z : nullptr; boxes.n_obj = n_obj; boxes.gm = gm;
    plane = W_ * H_;
    channels = channels_;
  }
  // fork: the background chain's inputs are ready in `root` order.  From here on `sb` is joined on every exit path (jb: the skeletons
  // join it before their last kernel) and so is the parameter stream on the error paths (jp: the caller joins it after a clean return)
  int fork() {
    sb = scene_fork_stream(st);
    STOVE_TRY(stream_after(sb, root));
    jb.from = sb; jb.done = sb == st;
    jp.from = sp; jp.done = sp == st;
    return 0;
  }
};

// Forward: fork, object chain (on c.st), background chain (on c.sb: MFMA-bound next to the VALU-bound object chain), join, assemble.
template <class Obj, class Bg>
static int scene_forward(SceneCall& c, float overlap_beta, float* ll, float* parts, Obj obj_chain, Bg bg_chain) {
  int rc = c.fork();
  if (rc) return rc;
  if ((rc = obj_chain())) return rc;
  if ((rc = bg_chain())) return rc;
  STOVE_TRY(c.jb.join());
  STOVE_LAUNCH(scene_assemble_fwd_k, dim3((c.nf + 255) / 256), dim3(256), 0, c.st, c.saved + c.L.bg_out, c.saved + c.L.obj_ll,
               c.saved + c.L.ovl, c.z, ll, parts, c.n_obj, c.nf, overlap_beta, logf(overlap_beta));
  STOVE_LAUNCH_CHECK();
  return 0;
}

// Backward: assemble, fork, what runs off the call's stream (the background chain on c.sb, which leaves dz_bg as `bg_parts` partial
// images; the tuned pipeline may also start its table gradients on c.sp here), the object chain (on c.st, leaves dzc with `nmax`
// entries per glimpse), join -- only the last kernel needs dz_bg --, finalize, and what the pipeline does once dz is out: the
// parameter stream is at least ordered behind c.st there.
template <class Side, class Obj, class After>
static int scene_backward(SceneCall& c, const float* dll, float* dz, float overlap_beta, int nmax, const float* dz_bg, int bg_parts,
                          Side side_chains, Obj obj_chain, After after_finalize) {
  STOVE_LAUNCH(scene_assemble_bwd_k, dim3((c.np + 255) / 256), dim3(256), 0, c.st, dll, c.z, c.ws + c.W.d_obj, c.ws + c.W.d_ovl, c.n_obj,
               c.np, overlap_beta);
  STOVE_LAUNCH_CHECK();
  int rc = c.fork();
  if (rc) return rc;
  if ((rc = side_chains())) return rc;
  if ((rc = obj_chain())) return rc;
  STOVE_TRY(c.jb.join());
  rc = with_nmax(nmax, [&](auto n) {
    STOVE_LAUNCH((scene_finalize_bwd_k<decltype(n)::value>), dim3((c.np + 255) / 256), dim3(256), 0, c.st, dll, c.z, c.saved + c.L.obj_ll,
                 dz_bg, c.ws + c.W.dzc, dz, c.n_obj, c.np, bg_parts);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
  if (rc) return rc;
  if ((rc = after_finalize())) return rc;
  c.jp.dismiss();
  return 0;
}

// Object chain of the tuned (ANY = false) and any-size pipelines: the 32 x 32 path's kernels, with the geometry at run time for ANY.
// with_grad != 0: the object SPN runs forward + backward at unit upstream gradient in one pass (objspn_fwd_unit_k) and leaves the
// per-glimpse backward scratch in `saved`.
template <bool ANY>
static int scene_obj_fwd(const SceneCall& c, const StoveSpnTables* t, float* saved, int with_grad) {
  float* xw = saved + c.L.xw;
  int rc = with_nmax(c.n_obj, [&](auto n) { return scene_tile_fwd<decltype(n)::value, ANY>(c.frames, c.z, xw, c.n_obj, c.np, c.st, c.fm, c.gm); });
  if (rc) return rc;
  if (with_grad)
    return objspn_forward_unit(xw, t->obj_scope, t->obj_coef, t->obj_wsum, t->obj_wroot, saved + c.L.obj_ll, saved + c.L.ovl,
                               saved + c.L.obj_scratch, c.np, c.st);
  return objspn_forward(xw, t->obj_scope, t->obj_coef, t->obj_wsum, t->obj_wroot, saved + c.L.obj_ll, saved + c.L.ovl, c.np, c.st);
}
// The object SPN's backward already ran, at unit upstream gradient, inside the forward: what is left is to apply d_obj[patch] where its
// scratch is consumed -- dL/d tile + transformer / mask backward in one pass over the leaf gradients (scene_pixtile_bwd_k) here, and
// the table gradients below.
template <bool ANY>
static int scene_obj_bwd(const SceneCall& c, const StoveSpnTables* t) {
  return with_nmax(c.n_obj, [&](auto n) {
    return scene_pixtile_bwd<decltype(n)::value, ANY>(c.frames, c.z, c.saved + c.L.xw, c.saved + c.L.obj_scratch, t->obj_leaf_slot, t->obj_coef,
                                                      c.ws + c.W.d_ovl, c.ws + c.W.dzc, c.n_obj, c.np, c.st, c.fm, c.ws + c.W.d_obj, c.gm);
  });
}
// table gradients of the object SPN on the parameter stream, behind everything c.st holds so far
static int scene_obj_tablegrads(const SceneCall& c, const StoveSpnTables* t, StoveSpnTableGrads* g, bool under = false) {
  STOVE_TRY(stream_after(c.sp, c.st));
  return objspn_backward_params(c.saved + c.L.xw, t->obj_scope, g->obj_coef, g->obj_wsum, g->obj_wroot, c.saved + c.L.obj_scratch,
                                c.ws + c.W.obj, c.ws + c.W.d_obj, c.np, c.sp, under);
}

// Background chain of the any-size and colour pipelines: the mask in closed form (bg_mask_any_k; one plane for all channels), the
// general-size operator of spn_bg_generic.hip over channels * plane dimensions ...
static int scene_bg_fwd_any(const SceneCall& c, const int32_t* side, const float* coef, const float* wroot, float* saved) {
  if (!c.inl) {
    const size_t tot = (size_t)c.nf * c.plane;
    STOVE_LAUNCH(bg_mask_any_k, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.sb, c.z, saved + c.L.bg_aux, c.nf, c.n_obj, c.gm);
    STOVE_LAUNCH_CHECK();
  }
  return bgspn_any_forward(c.frames, c.inl ? nullptr : saved + c.L.bg_aux, side, coef, wroot, saved + c.L.bg_ell, saved + c.L.bg_out, c.nf,
                           c.channels * c.plane, c.sb, c.fm, c.boxes, c.plane);
}
// ... backward: the operator's (d mask of every plane, table gradients), then the mask's backward to z (bg_mask_bwd_any_k, planes summed)
static int scene_bg_bwd_any(const SceneCall& c, const int32_t* side, const float* coef, const float* wroot, const float* dll, float* g_coef,
                            float* g_wroot) {
  float* d_mask = c.ws + c.W.d_mask;
  int rc = bgspn_any_backward(c.frames, c.inl ? nullptr : c.saved + c.L.bg_aux, side, coef, wroot, c.saved + c.L.bg_ell, c.saved + c.L.bg_out,
                              dll, nullptr, d_mask, g_coef, g_wroot, c.ws + c.W.bg, c.nf, c.channels * c.plane, c.sb, c.fm, c.boxes, c.plane);
  if (rc) return rc;
  return with_nmax<false>(c.n_obj, [&](auto n) {
    STOVE_LAUNCH((bg_mask_bwd_any_k<decltype(n)::value>), dim3(c.nf), dim3(256), 0, c.sb, c.z, (const float*)d_mask, c.ws + c.W.dz_bg, c.nf,
                 c.n_obj, c.gm, c.channels);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
}

}  // namespace stove

extern "C" {

// ---- the tuned pipeline: 32 x 32 frames, 10 x 10 glimpses, align_corners = False
static SceneSaved scene_saved_tuned(int nf, int n_obj, bool with_grad = true) {
  return scene_saved_layout(nf, n_obj, with_grad, bgspn_fwd_ws_floats(nf), bg_cover_floats(nf, n_obj));
}
static SceneWs scene_ws_tuned(int nf, int n_obj) {
  return scene_ws_layout((size_t)nf * n_obj, nmax_of(n_obj), 0, objspn_partial_floats(), 0, bgspn_bwd_ws_floats(nf, n_obj));
}
size_t stove_scene_saved_floats(int n_frames, int n_obj) { return scene_saved_tuned(n_frames, n_obj).total; }
size_t stove_scene_fwd_floats(int n_frames, int n_obj, int with_grad) { return scene_saved_tuned(n_frames, n_obj, with_grad != 0).total; }
size_t stove_scene_bwd_ws_bytes(int n_frames, int n_obj) { return scene_ws_tuned(n_frames, n_obj).total * sizeof(float); }

size_t stove_bg_dense_floats(void) { return (size_t)kBgDenseF; }
int stove_bg_dense(const int32_t* bg_side, const float* bg_coef, float* dense, void* stream) {
  STOVE_LAUNCH(bg_dense_fwd_k, dim3((kBgDenseF + 255) / 256), dim3(256), 0, (hipStream_t)stream, bg_side, bg_coef, dense);
  STOVE_LAUNCH_CHECK();
  return 0;
}
int stove_scene_fwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                    int seq_stride, float overlap_beta, float* ll, float* parts, float* saved, void* stream) {
  return stove_scene_fwd_from(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, overlap_beta, ll, parts, saved, stream, stream, 1);
}

// fork_from: the stream the internal background-SPN chain is ordered behind (its inputs -- frames, z, tables -- must be ready there).
// Normally `stream` itself.  A caller that runs the call on a stream which is itself a fork of a stream under hipGraph capture passes
// that capture's ORIGIN stream: the HIP 7.0 runtime cannot end a capture in which two forked streams wait on each other
// (fork from X, join into X, with X not the origin: hip::Stream::EndCapture recurses forever; tools/ubench/graph_ext2.hip).
// with_grad != 0: the object SPN runs forward + backward at unit upstream gradient in one pass (objspn_fwd_unit_k) and leaves
// the per-glimpse backward scratch in `saved` (stove_scene_fwd_floats(.., 1) = stove_scene_saved_floats floats): what
// stove_scene_bwd* needs.  0: likelihood only, `saved` of stove_scene_fwd_floats(.., 0) floats, no backward from it.
int stove_scene_fwd_from(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                         int seq_stride, float overlap_beta, float* ll, float* parts, float* saved, void* stream, void* fork_from,
                         int with_grad) {
  STOVE_VALIDATE(scene_fwd(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, ll, saved));
  if (n_frames == 0) return 0;
  SceneCall c(frames, z, n_frames, n_obj, stream, fork_from);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  c.L = scene_saved_tuned(n_frames, n_obj);
  c.saved = saved;
  return scene_forward(
      c, overlap_beta, ll, parts, [&] { return scene_obj_fwd<false>(c, t, saved, with_grad); },
      [&] {
        int rc = bgspn_forward(frames, nullptr, z, n_obj, t->bg_side, t->bg_coef, t->bg_wroot, saved + c.L.bg_ell, saved + c.L.bg_out, n_frames,
                               c.sb, c.fm, t->bg_dense);
        if (rc) return rc;
        return bg_cover_tables(z, saved + c.L.bg_aux, n_frames, n_obj, c.sb);       // for the backward of this z
      });
}

int stove_scene_bwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                    int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz, StoveSpnTableGrads* g,
                    void* ws_, void* stream) {
  return stove_scene_bwd_overlap(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, overlap_beta, saved, dll, dz, g, ws_, stream, stream);
}

int stove_scene_bwd_overlap(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                            int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz,
                            StoveSpnTableGrads* g, void* ws_, void* stream, void* param_stream) {
  return stove_scene_bwd_from(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, overlap_beta, saved, dll, dz, g, ws_, stream, param_stream, stream);
}

constexpr int kLateTableGradGlimpses = 16384;
// Where the object-SPN table gradients run when the caller gives a parameter stream: with up to four objects they are held back
// until dz is out and then run underneath the recursion's backward as objspn_tablegrad_under_k (one wave per SIMD in the registers
// and LDS that kernel leaves free).  Measured in round 2 (B = 256): the SPN backward phase 600 -> 495 us without them, the
// recursion's backward 470 -> 545 us with them on its SIMDs, the step 3.273 -> 3.254 ms.  (The round-1 placement -- right behind
// their producer, next to pix / bgspn_bwd -- was a switch until round 5.)
// Both workgroups must be resident on one CU: the recursion's dynamic LDS (smb_lds_floats<4>, gnn_small_bwd.hip), its 1 KB of
// static LDS (the waves' exchange rows, gnn_small.hip) and 512 B of allocation granule, plus the table-gradient kernel's tile,
// within 160 KB.  (Registers: 310 of a SIMD lane's 512 there, in granules of 8, so at most 200 here -- held by the kernel's
// amdgpu_num_vgpr attribute.)
static_assert(kTgLdsU + smb_lds_floats<4>() * (int)sizeof(float) + 64 * kSmWaves * (int)sizeof(float) + 512 <= 160 * 1024,
              "objspn_tablegrad_under_k no longer fits into the LDS that dyn_loop_bwd_small_k<4, ..> leaves free");

// fork_from: see stove_scene_fwd_from (the background chain's inputs -- frames, z, saved, dll -- must be ready in its order)
int stove_scene_bwd_from(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                         int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz,
                         StoveSpnTableGrads* g, void* ws_, void* stream, void* param_stream, void* fork_from) {
  STOVE_VALIDATE(scene_bwd(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, saved, dll, dz, g, ws_));
  if (n_frames == 0) return 0;
  SceneCall c(frames, z, n_frames, n_obj, stream, fork_from, param_stream);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  c.L = scene_saved_tuned(n_frames, n_obj);
  c.saved = saved;
  c.W = scene_ws_tuned(n_frames, n_obj);
  c.ws = (float*)ws_;
  // The object-SPN table gradients go to the parameter stream once dz is out (underneath what the caller enqueues next, the
  // recursion's backward) ...
  // ... for up to four objects: that recursion (dyn_loop_bwd_small_k<4, ..>: 253 + 58 registers, one wave per SIMD on every CU at
  // B = 256) is the latency-bound kernel with room beside it.  The five / six-object instantiation holds 256 + 192 of a SIMD lane's
  // 512 registers (hipcc -Rpass-analysis=kernel-resource-usage, round 5), so nothing wider than 64 registers can run beside it --
  // the 150-register table-gradient kernel would queue up behind it instead of under it -- and the seven / eight-object recursion
  // (gnn.hip) fills the matrix pipe itself (stretched 2.49 -> 3.20 ms by a co-runner, round 2)
  // ... and for a batch large enough that the recursion's backward is long (98 steps): at the reference's default training shape
  // (256 clips x 8 frames: 6 912 glimpses, a 35 us recursion) the held-back table gradients would be the head of a 260 us chain of
  // small launches on the parameter stream that outlasts the main stream by 110 us -- there they start at once, beside the data half
  const bool late = c.sp != c.st && n_obj <= 4 && c.np >= kLateTableGradGlimpses;
  return scene_backward(
      c, dll, dz, overlap_beta, nmax_of(n_obj), bgspn_dz_parts(c.ws + c.W.bg, n_frames), kBgHalves,
      [&] {
        if (!late) {
          const int rc = scene_obj_tablegrads(c, t, g);
          if (rc) return rc;
        }
        // (dz = null: the per-half partial images of dz_bg stay where bgspn_bwd_k wrote them; the finalize kernel sums them.  Without a
        // parameter stream the background's table gradients stay on the fork stream, joined before that kernel as well)
        return bgspn_backward(frames, nullptr, z, n_obj, t->bg_side, t->bg_coef, t->bg_wroot, saved + c.L.bg_ell, saved + c.L.bg_out, dll, nullptr,
                              nullptr, nullptr, g->bg_coef, g->bg_wroot, c.ws + c.W.bg, n_frames, c.sb, c.sp == c.st ? c.sb : c.sp, c.fm,
                              saved + c.L.bg_aux);
      },
      [&] { return scene_obj_bwd<false>(c, t); }, [&] { return late ? scene_obj_tablegrads(c, t, g, true) : 0; });
}

// ---------------------------------------------------------------- object RAT-SPN operator, any glimpse size / vector widths
static ObjAnyShape obj_any_shape(int R, int G, int S, int D, int Lmax) {
  ObjAnyShape sh;
  sh.R = R; sh.G = G; sh.S = S; sh.D = D; sh.Lmax = Lmax;
  return sh;
}
size_t stove_objspn_saved_floats_any(int n, int R, int G, int S, int D, int Lmax) { return objany_saved_floats(n, obj_any_shape(R, G, S, D, Lmax)); }
size_t stove_objspn_bwd_ws_bytes_any(int n, int R, int G, int S, int D, int Lmax) { return objany_bwd_ws_floats(n, obj_any_shape(R, G, S, D, Lmax)) * sizeof(float); }
int stove_objspn_fwd_any(const float* inputs, const float* marg, const int* lscope, const float* coef, const float* wsum, const float* wroot,
                         float* saved, float* out, int n, int R, int G, int S, int D, int Lmax, void* stream) {
  return objany_forward(inputs, marg, lscope, coef, wsum, wroot, saved, out, n, obj_any_shape(R, G, S, D, Lmax), (hipStream_t)stream);
}
int stove_objspn_bwd_any(const float* inputs, const float* marg, const int* lscope, const int* slot, const float* coef, const float* wsum,
                         const float* wroot, const float* saved, const float* dout, float* d_inputs, float* d_marg, float* g_coef,
                         float* g_wsum, float* g_wroot, void* ws, int n, int R, int G, int S, int D, int Lmax, void* stream) {
  return objany_backward(inputs, marg, lscope, slot, coef, wsum, wroot, saved, dout, d_inputs, d_marg, g_coef, g_wsum, g_wroot, (float*)ws, n,
                         obj_any_shape(R, G, S, D, Lmax), (hipStream_t)stream);
}

int stove_gauss_ll_fwd(const float* x, const float* marg, float* out, int n, int d, float mean, float scale, void* stream) {
  if (n == 0) return 0;
  if (d < 1 || !(scale > 0.0f) || x == nullptr || marg == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(gauss_ll_fwd_k, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, marg, out, n, d, mean, scale);
  STOVE_LAUNCH_CHECK();
  return 0;
}
int stove_gauss_ll_bwd(const float* x, const float* marg, const float* dout, float* dx, float* dm, int n, int d, float mean, float scale,
                       void* stream) {
  if (n == 0) return 0;
  if (d < 1 || !(scale > 0.0f) || x == nullptr || marg == nullptr || dout == nullptr) return (int)hipErrorInvalidValue;
  const size_t tot = (size_t)n * d;
  STOVE_LAUNCH(gauss_ll_bwd_k, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, marg, dout, dx, dm, n, d, mean, scale);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- fused scene likelihood, any frame size / sampling convention
// The object side is the 32 x 32 path's own kernels with the geometry at run time (scene_tile_fwd_k / scene_pixtile_bwd_k <.., ANY>,
// objspn_fwd_unit_k, the table-gradient kernels); the background side is the mask in closed form (bg_mask_any_k), the general-size
// operator of spn_bg_generic.hip, and the mask's backward to z (bg_mask_bwd_any_k).
// saved: bg_ell is (n x halves x 36), bg_aux the mask (n x n_pix)
static SceneSaved scene_saved_any(int nf, int n_obj, int n_pix, bool with_grad, bool inline_mask = false) {
  return scene_saved_layout(nf, n_obj, with_grad, bgspn_any_saved_floats(nf, n_pix), inline_mask ? 0 : (size_t)nf * n_pix);
}
static SceneWs scene_ws_any(int nf, int n_obj, int n_pix) {
  return scene_ws_layout((size_t)nf * n_obj, nmax_of(n_obj), 0, objspn_partial_floats(), (size_t)nf * n_pix, bgspn_any_bwd_ws_floats(nf, n_pix));
}
size_t stove_scene_saved_floats_any(int n_frames, int n_obj, int n_pix, int with_grad) { return scene_saved_any(n_frames, n_obj, n_pix, with_grad != 0).total; }
size_t stove_scene_bwd_ws_bytes_any(int n_frames, int n_obj, int n_pix) { return scene_ws_any(n_frames, n_obj, n_pix).total * sizeof(float); }

int stove_scene_fwd_any(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride,
                        int W, int H, int align_corners, float overlap_beta, float* ll, float* parts, float* saved, void* stream, int with_grad) {
  STOVE_VALIDATE(scene_fwd(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, ll, saved));
  if (n_frames == 0) return 0;
  if (W < 2 || H < 2 || n_obj < 1 || n_obj > 8) return (int)hipErrorInvalidValue;
  SceneCall c(frames, z, n_frames, n_obj, stream);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  c.geometry(W, H, align_corners, 1);
  c.L = scene_saved_any(n_frames, n_obj, W * H, true, c.inl);
  c.saved = saved;
  return scene_forward(
      c, overlap_beta, ll, parts, [&] { return scene_obj_fwd<true>(c, t, saved, with_grad); },
      [&] { return scene_bg_fwd_any(c, t->bg_side, t->bg_coef, t->bg_wroot, saved); });
}

int stove_scene_bwd_any(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride,
                        int W, int H, int align_corners, float overlap_beta, const float* saved, const float* dll, float* dz,
                        StoveSpnTableGrads* g, void* ws_, void* stream, void* param_stream) {
  STOVE_VALIDATE(scene_bwd(t, frames, z, n_frames, n_obj, seq_frames, seq_stride, saved, dll, dz, g, ws_));
  if (n_frames == 0) return 0;
  if (W < 2 || H < 2 || n_obj < 1 || n_obj > 8) return (int)hipErrorInvalidValue;
  SceneCall c(frames, z, n_frames, n_obj, stream, nullptr, param_stream);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  c.geometry(W, H, align_corners, 1);
  c.L = scene_saved_any(n_frames, n_obj, W * H, true, c.inl);
  c.saved = saved;
  c.W = scene_ws_any(n_frames, n_obj, W * H);
  c.ws = (float*)ws_;
  return scene_backward(
      c, dll, dz, overlap_beta, nmax_of(n_obj), c.ws + c.W.dz_bg, 1,
      [&] { return scene_bg_bwd_any(c, t->bg_side, t->bg_coef, t->bg_wroot, dll, g->bg_coef, g->bg_wroot); },
      [&] { return scene_obj_bwd<true>(c, t); },
      // the table gradients of the object SPN last (the background's are complete in `st` order: ordered into the parameter stream too)
      [&] { return scene_obj_tablegrads(c, t, g); });
}

// ---------------------------------------------------------------- fused scene likelihood over C colour channels
// Glimpses and masks of every channel in one pass (scene_colour_fwd_k), the general-size object SPN on C * pw * ph dimensions, the
// general-size background SPN on C * W * H dimensions with one mask plane for all channels; backward: the object SPN's data and table
// gradients, the glimpse backward to z (scene_colour_bwd_k), the background's mask backward with the C planes summed.
// the colour kernels come in two object-count instantiations (3 and 8: the 6-object one ran at the 8-object one's occupancy); dzc has
// nmax_ch(n_obj) entries per glimpse
static inline int nmax_ch(int n_obj) { return n_obj <= 3 ? 3 : 8; }
// saved = [ patches | marg | object-SPN saved | obj_ll | ovl | bg_out | bg_ell | mask (frames past kBgTabMax a side) ]
static SceneSaved scene_saved_ch(int nf, int n_obj, int C, int W, int H, const ObjAnyShape& sh) {
  const size_t np = (size_t)nf * n_obj;
  Layout l;
  SceneSaved s{};
  s.patches = l.take(np * sh.D);
  s.marg = l.take(np * sh.D);
  s.obj = l.take(objany_saved_floats((int)np, sh));
  scene_saved_shared(l, s, nf, np, bgspn_any_saved_floats(nf, C * W * H), scene_any_inline(W, H) ? 0 : (size_t)nf * W * H);
  s.total = l.total;
  return s;
}
// ws = [ d_obj | d_ovl | dzc | dz_bg | d_patch | d_marg | object-SPN ws | d_mask (C planes) | background ws ]
static SceneWs scene_ws_ch(int nf, int n_obj, int C, int W, int H, const ObjAnyShape& sh) {
  const size_t np = (size_t)nf * n_obj, n_pix = (size_t)C * W * H;
  return scene_ws_layout(np, nmax_ch(n_obj), np * sh.D, objany_bwd_ws_floats((int)np, sh), (size_t)nf * n_pix, bgspn_any_bwd_ws_floats(nf, (int)n_pix));
}
static GlimpseGeom glimpse_geom(int pw, int ph, int align_corners) {
  GlimpseGeom g;
  g.pw = pw; g.ph = ph;
  if (align_corners) {
    g.pax = 2.0f / (ph - 1); g.pbx = -1.0f; g.pay = 2.0f / (pw - 1); g.pby = -1.0f;
  } else {
    g.pax = 2.0f / ph; g.pbx = 1.0f / ph - 1.0f; g.pay = 2.0f / pw; g.pby = 1.0f / pw - 1.0f;
  }
  return g;
}
size_t stove_scene_saved_floats_ch(int n_frames, int n_obj, int channels, int W, int H, int R, int G, int S, int D, int Lmax, int with_grad) {
  (void)with_grad;                // the object SPN's saved activations are the same with and without a backward to come
  return scene_saved_ch(n_frames, n_obj, channels, W, H, obj_any_shape(R, G, S, D, Lmax)).total;
}
size_t stove_scene_bwd_ws_bytes_ch(int n_frames, int n_obj, int channels, int W, int H, int R, int G, int S, int D, int Lmax) {
  return scene_ws_ch(n_frames, n_obj, channels, W, H, obj_any_shape(R, G, S, D, Lmax)).total * sizeof(float);
}

int stove_scene_fwd_ch(const int32_t* lscope, const int32_t* slot, const float* coef, const float* wsum, const float* wroot, int R, int G, int S,
                       int D, int Lmax, const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats,
                       const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H,
                       int pw, int ph, int align_corners, float overlap_beta, float* ll, float* parts, float* saved, void* stream, int with_grad) {
  (void)slot;
  (void)with_grad;
  STOVE_VALIDATE(scene_ch_fwd(lscope, coef, wsum, wroot, R, G, S, D, Lmax, bg_side, bg_coef, bg_wroot, bg_coef_floats, frames, z, n_frames, n_obj,
                              seq_frames, seq_stride, channels, W, H, pw, ph, ll, saved));
  if (n_frames == 0) return 0;
  SceneCall c(frames, z, n_frames, n_obj, stream);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  const ObjAnyShape sh = obj_any_shape(R, G, S, D, Lmax);
  const GlimpseGeom gg = glimpse_geom(pw, ph, align_corners);
  c.geometry(W, H, align_corners, channels);
  c.L = scene_saved_ch(n_frames, n_obj, channels, W, H, sh);
  c.saved = saved;
  float *patches = saved + c.L.patches, *marg = saved + c.L.marg;
  return scene_forward(
      c, overlap_beta, ll, parts,
      [&] {      // glimpses + masks of every channel, the object SPN over C * pw * ph dimensions
        int rc = with_nmax<false>(n_obj, [&](auto n) {
          return scene_colour_fwd<decltype(n)::value>(frames, z, patches, marg, saved + c.L.ovl, n_obj, c.np, channels, c.st, c.fm, c.gm, gg);
        });
        if (rc) return rc;
        return objany_forward(patches, marg, lscope, coef, wsum, wroot, saved + c.L.obj, saved + c.L.obj_ll, c.np, sh, c.st);
      },
      [&] { return scene_bg_fwd_any(c, bg_side, bg_coef, bg_wroot, saved); });
}

int stove_scene_bwd_ch(const int32_t* lscope, const int32_t* slot, const float* coef, const float* wsum, const float* wroot, int R, int G, int S,
                       int D, int Lmax, const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats,
                       const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H,
                       int pw, int ph, int align_corners, float overlap_beta, const float* saved, const float* dll, float* dz, float* g_coef,
                       float* g_wsum, float* g_wroot, float* g_bg_coef, float* g_bg_wroot, void* ws_, void* stream, void* param_stream) {
  STOVE_VALIDATE(scene_ch_bwd(lscope, slot, coef, wsum, wroot, R, G, S, D, Lmax, bg_side, bg_coef, bg_wroot, bg_coef_floats, frames, z, n_frames,
                              n_obj, seq_frames, seq_stride, channels, W, H, pw, ph, saved, dll, dz, g_coef, g_wsum, g_wroot, g_bg_coef, g_bg_wroot,
                              ws_));
  if (n_frames == 0) return 0;
  SceneCall c(frames, z, n_frames, n_obj, stream, nullptr, param_stream);
  if (frame_map(n_frames, seq_frames, seq_stride, &c.fm)) return (int)hipErrorInvalidValue;
  const ObjAnyShape sh = obj_any_shape(R, G, S, D, Lmax);
  const GlimpseGeom gg = glimpse_geom(pw, ph, align_corners);
  c.geometry(W, H, align_corners, channels);
  c.L = scene_saved_ch(n_frames, n_obj, channels, W, H, sh);
  c.saved = saved;
  c.W = scene_ws_ch(n_frames, n_obj, channels, W, H, sh);
  c.ws = (float*)ws_;
  float *d_patch = c.ws + c.W.d_patch, *d_marg = c.ws + c.W.d_marg;
  return scene_backward(
      c, dll, dz, overlap_beta, nmax_ch(n_obj), c.ws + c.W.dz_bg, 1,
      [&] { return scene_bg_bwd_any(c, bg_side, bg_coef, bg_wroot, dll, g_bg_coef, g_bg_wroot); },
      [&] {      // the object SPN's data and table gradients, then the glimpse backward to z
        int rc = objany_backward(saved + c.L.patches, saved + c.L.marg, lscope, slot, coef, wsum, wroot, saved + c.L.obj, c.ws + c.W.d_obj, d_patch,
                                 d_marg, g_coef, g_wsum, g_wroot, c.ws + c.W.obj, c.np, sh, c.st);
        if (rc) return rc;
        return with_nmax<false>(n_obj, [&](auto n) {
          return scene_colour_bwd<decltype(n)::value>(frames, z, d_patch, d_marg, c.ws + c.W.d_ovl, c.ws + c.W.dzc, n_obj, c.np, channels, c.st, c.fm,
                                                      c.gm, gg);
        });
      },
      // every table gradient is complete in `st` order: the parameter stream is ordered behind it
      [&] { return (int)stream_after(c.sp, c.st); });
}

int stove_glimpse_mean(const float* x_color, const float* z, float* emb, int n_frames, int n_obj, int channels, void* stream) {
  const long long total = (long long)n_frames * n_obj;
  if (total == 0) return 0;
  if (total > 0x7fffffffLL || channels < 1 || channels > 4) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(glimpse_mean_k, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x_color, z, emb,
               n_frames * n_obj, n_obj, channels);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_objspn_mpe(const StoveSpnTables* t, const float* leaf_means, const float* inputs, float* xw, float* out,
                     int32_t* pick, int n, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = objspn_tile_from_arrays(inputs, nullptr, xw, n, st);
  if (rc) return rc;
  return objspn_mpe(xw, t->obj_scope, t->obj_coef, t->obj_wsum, t->obj_wroot, leaf_means, out, pick, n, st);
}

int stove_render_frames(const float* bg, const float* patches, int frames_per_patch, const float* z, float* out, int n_frames,
                        int n_obj, void* stream) {
  const long long total = (long long)n_frames * 1024;
  if (total == 0) return 0;
  if (frames_per_patch < 0 || n_obj < 0 || (total + 255) / 256 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(render_frames_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bg, patches,
               frames_per_patch, z, out, n_frames, n_obj);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- rendering at run-time sizes + squared pixel error (render.hip)
int stove_render_frames_any(const float* bg, const float* patches, int frames_per_patch, const float* z, const float* truth, float* out,
                            float* sqerr, int n_frames, int n_obj, int C, int W, int H, int pw, int ph, int align_corners, void* stream) {
  STOVE_VALIDATE(render_any(bg, patches, frames_per_patch, z, truth, out, sqerr, n_frames, n_obj, C, W, H, pw, ph));
  if (n_frames == 0) return 0;
  RenderGeom g;
  g.C = C; g.W = W; g.H = H; g.pw = pw; g.ph = ph;
  // affine_grid's base grid (a single pixel sits at 0 under either convention), grid_sample's unnormalisation
  const auto base = [&](int n, float* a, float* b) {
    if (n == 1) { *a = 0.0f; *b = 0.0f; }
    else if (align_corners) { *a = 2.0f / (n - 1); *b = -1.0f; }
    else { *a = 2.0f / n; *b = 1.0f / n - 1.0f; }
  };
  const auto unnorm = [&](int n, float* a, float* b) {
    if (align_corners) { *a = 0.5f * (n - 1); *b = 0.5f * (n - 1); }
    else { *a = 0.5f * n; *b = 0.5f * n - 0.5f; }
  };
  base(H, &g.col_a, &g.col_b);
  base(W, &g.row_a, &g.row_b);
  unnorm(ph, &g.px_a, &g.px_b);
  unnorm(pw, &g.py_a, &g.py_b);
  const int P = W * H;
  // the fused sum wants the whole frame in one workgroup; frames alone are cut into tiles of four positions per thread
  const int kTile = 4 * kRenderThreads;
  const int tiles = sqerr ? 1 : (P + kTile - 1) / kTile;
  const int tile_len = sqerr ? P : kTile;
  if (tiles > 65535) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)(frames_per_patch > 0 ? n_obj : 1) * C * pw * ph * sizeof(float);
  const dim3 grid((unsigned)n_frames, (unsigned)tiles), block(kRenderThreads);
  if (lds <= 56 * 1024) {
    STOVE_LAUNCH(render_frames_any_k<true>, grid, block, lds, (hipStream_t)stream, bg, patches, frames_per_patch, z, truth, out, sqerr, n_obj,
                 g, tile_len);
  } else {          // the frame's patch rows do not fit the LDS: the taps read global memory
    STOVE_LAUNCH(render_frames_any_k<false>, grid, block, 0, (hipStream_t)stream, bg, patches, frames_per_patch, z, truth, out, sqerr, n_obj,
                 g, tile_len);
  }
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_scene_glimpses(const float* frames, const float* z, int n_frames, int n_obj, float* tile, float* patches,
                         float* keep, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int np = n_frames * n_obj;
  if (np == 0) return 0;
  int rc = with_nmax(n_obj, [&](auto n) { return scene_tile_fwd<decltype(n)::value>(frames, z, tile, n_obj, np, st, FrameMap{0, 0}); });
  if (rc) return rc;
  const int nb = (np + 63) / 64;
  STOVE_LAUNCH(tile_unpack_k, dim3(nb < 2048 ? nb * 25 : 2048 * 25), dim3(256), 0, st, tile, patches, keep, np, nb);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- GNN dynamics core
// The small-graph recursion (gnn_small*.hip): kernels built for up to four objects (one node row per wave) and for up to six (two).
static bool small_graph(int N) { return N >= 2 && N <= 6; }
constexpr size_t kGnnLdsBytes = kGnnLdsFloats * sizeof(float);

size_t stove_gnn_param_floats(void) { return kGnnParams; }
size_t stove_gnn_grad_floats(void) { return kGnnGrads; }
int stove_gnn_blocks(int B, int N) {
  const int g = gnn_group_for(B, N);
  return (B + g - 1) / g;
}

int stove_gnn_fwd(const float* s_in, const float* params, float* result, float* pred, int B, int N, int sin_dim,
                  int lim_enc, int elu, void* stream) {
  STOVE_VALIDATE(gnn_fwd(s_in, params, result, B, N, sin_dim));
  if (B == 0) return 0;
  return STOVE_LAUNCH_LDS(gnn_step_fwd_k, dim3(stove_gnn_blocks(B, N)), dim3(256), kGnnLdsBytes, (hipStream_t)stream,
                          s_in, params, result, pred, B, N, gnn_group_for(B, N), sin_dim, lim_enc, elu);
}

size_t stove_gnn_bwd_ws_bytes(int B, int N) { return (size_t)stove_gnn_blocks(B, N) * kGnnGrads * sizeof(float); }

int stove_gnn_bwd(const float* s_in, const float* params, const float* d_result, const float* d_pred, float* d_s_in,
                  float* g_params, void* ws, int B, int N, int sin_dim, int lim_enc, int elu, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (g_params == nullptr) return (int)hipErrorInvalidValue;
  STOVE_VALIDATE(gnn_bwd(s_in, params, d_result, d_s_in, g_params, ws, B, N, sin_dim));
  if (B == 0) {
    hipMemsetAsync(g_params, 0, kGnnGrads * sizeof(float), st);
    return 0;
  }
  const int nb = stove_gnn_blocks(B, N);
  int rc = STOVE_LAUNCH_LDS(gnn_step_bwd_k, dim3(nb), dim3(256), kGnnLdsBytes, st, s_in, params, d_result, d_pred,
                            d_s_in, (float*)ws, B, N, gnn_group_for(B, N), sin_dim, lim_enc, elu, (long long*)nullptr);
  if (rc) return rc;
  STOVE_LAUNCH(reduce_chunks_k, dim3((kGnnGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, kGnnGrads, nb, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// debug: one fwd+bwd step with per-stage cycle stamps of block 0 (stamps: 64 int64 on the device)
int stove_gnn_debug_stamps(const float* s_in, const float* params, const float* d_result, float* d_s_in, void* ws,
                           long long* stamps, int B, int N, int sin_dim, int lim_enc, int elu, void* stream) {
  return STOVE_LAUNCH_LDS(gnn_step_bwd_k, dim3(stove_gnn_blocks(B, N)), dim3(256), kGnnLdsBytes, (hipStream_t)stream, s_in, params,
                          d_result, (const float*)nullptr, d_s_in, (float*)ws, B, N, gnn_group_for(B, N), sin_dim, lim_enc, elu, stamps);
}

// debug: device buffer ([4 waves][16] int64) that the small-graph time loops stamp their phases into (last step,
// workgroup 0); null = off.  Set by the measurement tools only.
static long long* g_sm_stamps = nullptr;
void stove_debug_set_stamps(long long* device_buffer) { g_sm_stamps = device_buffer; }

size_t stove_dynloop_act_floats(int B, int Ts, int N) {
  const int g = gnn_group_for(B, N);
  const size_t blockwise = (size_t)stove_gnn_blocks(B, N) * Ts * gnn_act_floats(N, g);
  if (small_graph(N)) {
    const size_t streams = (size_t)B * sm_act2_floats(N, Ts);
    return streams > blockwise ? streams : blockwise;
  }
  return blockwise;
}

// The small-graph kernels keep the piece interface of the round-3 pipelining experiment (the steps [ts0, ts1), the gradient carried
// between pieces: docs/experiments/r06_pipeline_pieces_removed.patch) -- taking it out changes the device code of the most
// latency-sensitive kernels, a measured change of its own.  The entry points run the whole range: 0, Ts, no carry -- unless a test
// has set a piece with stove_debug_set_piece: then the small-graph launches run the steps [ts0, ts1) of the Ts the tensors are laid
// out for.  Forward: a piece with ts0 > 0 starts from the state the previous piece left in z.  Backward: pieces are called from the
// last to the first over the same act / ws buffers; the gradient that flows from step ts0 into the state before it goes through
// `carry` (B, N, 18 floats on the device; written when ts0 > 0, read when ts1 < Ts); the piece with ts0 == 0 writes dz1 and runs the
// weight-gradient pass over the streams of ALL steps.  ts1 <= 0 (default) switches it off.
static int g_sm_ts0 = 0, g_sm_ts1 = 0;
static float* g_sm_carry = nullptr;
void stove_debug_set_piece(int ts0, int ts1, float* carry) {
  g_sm_ts0 = ts0;
  g_sm_ts1 = ts1;
  g_sm_carry = carry;
}
static bool sm_piece(int Ts, int& p0, int& p1) {      // false: a piece is set that is not a range of steps of these tensors
  p0 = g_sm_ts1 > 0 ? g_sm_ts0 : 0;
  p1 = g_sm_ts1 > 0 ? g_sm_ts1 : Ts;
  return p0 >= 0 && p0 < p1 && p1 <= Ts;
}
int stove_dynloop_fwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                      const float* params, float* z, float* zdyn, float* zdstd, float* mean, float* std_, float* pred, float* act,
                      int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                      void* stream) {
  STOVE_VALIDATE(dynloop_fwd(z1, zsup, zsstd, eps, extra, params, z, zdyn, zdstd, mean, std_, B, Ts, N, sin_dim));
  if (B == 0 || Ts == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  if (small_graph(N)) {      // small graphs: (half-)wave-per-node-row formulation, two barriers per step (gnn_small.hip)
    int p0, p1;
    if (!sm_piece(Ts, p0, p1)) return (int)hipErrorInvalidValue;
    auto launch = [&](auto save, auto nmx, auto e, auto nt, auto stamp) {
      constexpr int NMX = decltype(nmx)::value;
      return STOVE_LAUNCH_LDS((dyn_loop_fwd_small_k<decltype(save)::value, NMX, decltype(e)::value, decltype(nt)::value, decltype(stamp)::value>),
                              dim3(B), dim3(64 * kSmWaves), SmShape<NMX>::kLdsFloats * sizeof(float), (hipStream_t)stream, z1, zsup, zsstd, eps,
                              extra, params, z, zdyn, zdstd, mean, std_, pred, act, B, Ts, N, sin_dim, lim_enc, elu, kc, g_sm_stamps, p0, p1);
    };
    if (g_sm_stamps != nullptr && act != nullptr && !elu && N == 3)      // tools/loop_stamps.py: the one instantiation that stamps its phases
      return launch(Int<2>{}, Int<4>{}, std::false_type{}, Int<3>{}, std::true_type{});
    auto run = [&](auto save) {           // SAVE: 2 = keep the activations for the backward, 0 = none
      return with_small_graph<true>(N, elu, true, [&](auto nmx, auto e, auto nt) { return launch(save, nmx, e, nt, std::false_type{}); });
    };
    return act != nullptr ? run(Int<2>{}) : run(Int<0>{});
  }
  const int G = gnn_group_for(B, N);
  return with_flag(elu, [&](auto e) {
    return with_flag(N == 6 && G == 1, [&](auto n6) {
      return STOVE_LAUNCH_LDS((dyn_loop_fwd_k<decltype(e)::value, decltype(n6)::value>), dim3(stove_gnn_blocks(B, N)), dim3(256), kGnnLdsBytes,
                              (hipStream_t)stream, z1, zsup, zsstd, eps, extra, params, z, zdyn, zdstd, mean, std_, pred, act, B, Ts, N, G,
                              sin_dim, lim_enc, elu, kc);
    });
  });
}

size_t stove_dynloop_bwd_ws_bytes(int B, int N) { return stove_gnn_bwd_ws_bytes(B, N); }

static bool small_bwd_path(int N, const float* act) { return small_graph(N) && act != nullptr; }

// workspace of stove_dynloop_bwd for Ts steps: per-workgroup partial weight gradients, plus (small-graph path) the dY streams
size_t stove_dynloop_bwd_ws_bytes_ts(int B, int Ts, int N) {
  size_t f = stove_gnn_bwd_ws_bytes(B, N) / sizeof(float);
  if (small_graph(N)) f = (size_t)B * kGnnGrads + (size_t)B * sm_dy_floats(N, Ts);
  return f * sizeof(float);
}

int stove_dynloop_bwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                      const float* params, const float* z, const float* act, const float* dz, const float* dzdyn, const float* dmean,
                      const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd, float* dextra,
                      float* g_params, void* ws, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                      float vel_std, float lat_std, void* stream) {
  return stove_dynloop_bwd_overlap(z1, zsup, zsstd, eps, extra, params, z, act, dz, dzdyn, dmean, dstd, dpred, dz1, dzsup, dzsstd,
                                   dextra, g_params, ws, B, Ts, N, sin_dim, lim_enc, elu, pos_var, vel_std, lat_std, stream, stream);
}

int stove_dynloop_bwd_overlap(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                              const float* params, const float* z, const float* act, const float* dz, const float* dzdyn,
                              const float* dmean, const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd,
                              float* dextra, float* g_params, void* ws, int B, int Ts, int N, int sin_dim, int lim_enc, int elu,
                              float pos_var, float vel_std, float lat_std, void* stream, void* param_stream) {
  STOVE_VALIDATE(dynloop_bwd(z1, zsup, zsstd, eps, extra, params, z, dz1, dzsup, dzsstd, dextra, g_params, ws, B, Ts, N, sin_dim));
  hipStream_t st = (hipStream_t)stream;
  hipStream_t sp = param_stream != nullptr ? (hipStream_t)param_stream : st;
  LoopConst kc{pos_var, vel_std, lat_std};
  if (small_bwd_path(N, act)) {
    // small graphs: T-serial data-gradient chain (gnn_small_bwd.hip), then the weight gradients as a throughput pass
    float* gpart = (float*)ws;
    float* dy = gpart + (size_t)B * kGnnGrads;
    int p0, p1;
    if (!sm_piece(Ts, p0, p1) || ((p0 > 0 || p1 < Ts) && g_sm_carry == nullptr)) return (int)hipErrorInvalidValue;
    float* carry = g_sm_carry;
    // HEAD: the instantiations for the gradients the training step hands over; only three and six objects have them
    const bool head = dz != nullptr && dzdyn != nullptr && dmean != nullptr && dstd != nullptr && dpred == nullptr && sin_dim == 16 && lim_enc == 2;
    auto launch = [&](auto nmx, auto e, auto nt, auto hd, auto stamp) {
      constexpr int NMX = decltype(nmx)::value;
      return STOVE_LAUNCH_LDS((dyn_loop_bwd_small_k<NMX, decltype(e)::value, decltype(nt)::value, decltype(hd)::value, decltype(stamp)::value>),
                              dim3(B), dim3(64 * kSmWaves), smb_lds_floats<NMX>() * sizeof(float), st, zsup, zsstd, eps, params,
                              const_cast<float*>(act), dz, dzdyn, dmean, dstd, dpred, dz1, dzsup, dzsstd, dextra, dy, B, Ts, N, sin_dim, lim_enc,
                              elu, kc, g_sm_stamps, p0, p1, carry);
    };
    int rc;
    if (g_sm_stamps != nullptr && !elu && N == 3 && head) {       // tools/loop_stamps.py: the one instantiation that stamps its phases
      rc = launch(Int<4>{}, std::false_type{}, Int<3>{}, std::true_type{}, std::true_type{});
    } else {
      rc = with_small_graph<true>(N, elu, head, [&](auto nmx, auto e, auto nt) {
        constexpr int NT = decltype(nt)::value;
        if constexpr (NT == 6) {          // (reached with `head` only)
          return launch(nmx, e, nt, std::true_type{}, std::false_type{});
        } else {
          if constexpr (NT == 3) {
            if (head) return launch(nmx, e, nt, std::true_type{}, std::false_type{});
          }
          return launch(nmx, e, nt, std::false_type{}, std::false_type{});
        }
      });
    }
    if (rc) return rc;
    if (p0 > 0) return 0;                   // a piece that is not the first: the streams of the steps before it are still to come
    STOVE_TRY(stream_after(sp, st));        // the weight-gradient pass reads the dY streams; it only feeds the optimiser (second stream)
    rc = STOVE_LAUNCH_LDS(gnn_dw_small_k, dim3(B), dim3(256), kDwLdsFloats * sizeof(float), sp, act, (const float*)dy, gpart, B, Ts, N);
    if (rc) return rc;
    STOVE_LAUNCH(reduce_chunks_k, dim3((kGnnGrads + 31) / 32), dim3(256), 0, sp, (const float*)gpart, g_params, kGnnGrads, B, 0);
    STOVE_LAUNCH_CHECK();
    return 0;
  }
  const int nb = stove_gnn_blocks(B, N), G = gnn_group_for(B, N);
  int rc = with_flag(elu, [&](auto e) {
    return with_flag(N == 6 && G == 1, [&](auto n6) {
      return STOVE_LAUNCH_LDS((dyn_loop_bwd_k<decltype(e)::value, decltype(n6)::value>), dim3(nb), dim3(256), kGnnLdsBytes, st, z1, zsup, zsstd,
                              eps, extra, params, z, act, dz, dzdyn, dmean, dstd, dpred, dz1, dzsup, dzsstd, dextra, (float*)ws, B, Ts, N, G,
                              sin_dim, lim_enc, elu, kc);
    });
  });
  if (rc) return rc;
  STOVE_TRY(stream_after(sp, st));
  STOVE_LAUNCH(reduce_chunks_k, dim3((kGnnGrads + 31) / 32), dim3(256), 0, sp, (const float*)ws, g_params, kGnnGrads, nb, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_rollout_fwd(const float* z_last, const float* extra, const float* params, float* z_pred, float* zstd, float* pred,
                      int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std,
                      float lat_std, void* stream) {
  STOVE_VALIDATE(rollout_fwd(z_last, extra, params, z_pred, B, num, A, N, sin_dim));
  if (B == 0 || num == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  if (small_graph(N)) {      // (no instantiation for six objects of its own)
    return with_small_graph<false>(N, elu, false, [&](auto nmx, auto e, auto nt) {
      constexpr int NMX = decltype(nmx)::value;
      return STOVE_LAUNCH_LDS((rollout_fwd_small_k<NMX, decltype(e)::value, decltype(nt)::value>), dim3(B), dim3(64 * kSmWaves),
                              SmShape<NMX>::kLdsFloats * sizeof(float), (hipStream_t)stream, z_last, extra, params, z_pred, zstd, pred, B, num,
                              A < 1 ? 1 : A, N, sin_dim, lim_enc, elu, kc);
    });
  }
  return STOVE_LAUNCH_LDS(rollout_fwd_k, dim3(stove_gnn_blocks(B, N)), dim3(256), kGnnLdsBytes, (hipStream_t)stream, z_last, extra, params,
                          z_pred, zstd, pred, B, num, A < 1 ? 1 : A, N, gnn_group_for(B, N), sin_dim, lim_enc, elu, kc);
}

int stove_rollout_sample_fwd(const float* z_last, const float* extra, const float* params, const float* eps, float* z_pred,
                             float* log_q, float* zstd, float* pred, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu,
                             float pos_var, float vel_std, float lat_std, void* stream) {
  STOVE_VALIDATE(rollout_sample_fwd(z_last, extra, params, eps, z_pred, log_q, B, num, A, N, sin_dim));
  if (B == 0 || num == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  if (small_graph(N)) {      // the mean rollout's ladder
    return with_small_graph<false>(N, elu, false, [&](auto nmx, auto e, auto nt) {
      constexpr int NMX = decltype(nmx)::value;
      return STOVE_LAUNCH_LDS((rollout_sample_fwd_small_k<NMX, decltype(e)::value, decltype(nt)::value>), dim3(B), dim3(64 * kSmWaves),
                              SmShape<NMX>::kLdsFloats * sizeof(float), (hipStream_t)stream, z_last, extra, params, eps, z_pred, log_q, zstd,
                              pred, B, num, A < 1 ? 1 : A, N, sin_dim, lim_enc, elu, kc);
    });
  }
  return STOVE_LAUNCH_LDS(rollout_sample_fwd_k, dim3(stove_gnn_blocks(B, N)), dim3(256), kGnnLdsBytes, (hipStream_t)stream, z_last, extra,
                          params, eps, z_pred, log_q, zstd, pred, B, num, A < 1 ? 1 : A, N, gnn_group_for(B, N), sin_dim, lim_enc, elu, kc);
}

// An empty rollout backward (B == 0 or num == 0) on `st`: every output is zeros
static int rollout_bwd_empty(float* d_z_last, float* d_extra, float* g_params, size_t zw, size_t grads, int B, int A, int N, int E, hipStream_t st) {
  if (B > 0) STOVE_TRY(hipMemsetAsync(d_z_last, 0, (size_t)B * N * zw * sizeof(float), st));
  if (B > 0 && d_extra != nullptr && A > 0 && E > 0) STOVE_TRY(hipMemsetAsync(d_extra, 0, (size_t)B * A * N * E * sizeof(float), st));
  STOVE_TRY(hipMemsetAsync(g_params, 0, grads * sizeof(float), st));
  return 0;
}

size_t stove_rollout_bwd_ws_bytes(int B, int N) {
  if (B < 1 || N < 1 || N > stove_validate::kMaxObjects) return 0;
  return stove_gnn_bwd_ws_bytes(B, N);
}

int stove_rollout_bwd(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                      const float* d_z_pred, const float* d_log_q, const float* d_pred, float* d_z_last, float* d_extra,
                      float* g_params, void* ws, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                      float vel_std, float lat_std, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(rollout_bwd(z_last, extra, params, eps, z_pred, d_log_q, d_z_last, d_extra, g_params, ws, B, num, A, N, sin_dim));
  if (B == 0 || num == 0) return rollout_bwd_empty(d_z_last, d_extra, g_params, 18, kGnnGrads, B, A, N, sin_dim - 16, st);
  LoopConst kc{pos_var, vel_std, lat_std};
  const int nb = stove_gnn_blocks(B, N);
  int rc = STOVE_LAUNCH_LDS(rollout_bwd_k, dim3(nb), dim3(256), kGnnLdsBytes, st, z_last, extra, params, eps, z_pred, d_z_pred, d_log_q, d_pred,
                            d_z_last, d_extra, (float*)ws, B, num, A < 1 ? 1 : A, N, gnn_group_for(B, N), sin_dim, lim_enc, elu, kc);
  if (rc) return rc;
  STOVE_LAUNCH(reduce_chunks_k, dim3((kGnnGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, kGnnGrads, nb, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- GNN dynamics core at state-code lengths 16 / 64 (gnn_cl.hip)
size_t stove_gnn_param_floats_cl(int cl) { return cl == 16 ? GC<16>::kParams : (cl == 64 ? GC<64>::kParams : 0); }
size_t stove_gnn_grad_floats_cl(int cl) { return cl == 16 ? GC<16>::kGrads : (cl == 64 ? GC<64>::kGrads : 0); }
size_t stove_gnn_bwd_ws_bytes_cl(int cl, int B, int N) {
  if (B < 1 || N < 1 || N > 6) return 0;
  if (cl == 16) return (size_t)cl_blocks<16>(B, N) * GC<16>::kGrads * sizeof(float);
  if (cl == 64) return (size_t)cl_blocks<64>(B, N) * GC<64>::kGrads * sizeof(float);
  return 0;
}

int stove_gnn_fwd_cl(const float* s_in, const float* params, float* result, float* pred, int cl, int B, int N, int sin_dim,
                     int lim_enc, int elu, void* stream) {
  STOVE_VALIDATE(gnn_fwd(s_in, params, result, B, N, sin_dim, stove_validate::gnn_limits_cl(cl)));
  if (B == 0) return 0;
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    return STOVE_LAUNCH_LDS(gnn_cl_step_fwd_k<CL>, dim3(cl_blocks<CL>(B, N)), dim3(256), GC<CL>::kLdsFloats * sizeof(float), (hipStream_t)stream,
                            s_in, params, result, pred, B, N, cl_group_for<CL>(B, N), sin_dim, lim_enc, elu);
  });
}

int stove_gnn_bwd_cl(const float* s_in, const float* params, const float* d_result, const float* d_pred, float* d_s_in,
                     float* g_params, void* ws, int cl, int B, int N, int sin_dim, int lim_enc, int elu, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(gnn_bwd(s_in, params, d_result, d_s_in, g_params, ws, B, N, sin_dim, stove_validate::gnn_limits_cl(cl)));
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    if (B == 0) return (int)hipMemsetAsync(g_params, 0, GC<CL>::kGrads * sizeof(float), st);
    const int nb = cl_blocks<CL>(B, N);
    int rc = STOVE_LAUNCH_LDS(gnn_cl_step_bwd_k<CL>, dim3(nb), dim3(256), GC<CL>::kLdsFloats * sizeof(float), st, s_in, params, d_result, d_pred,
                              d_s_in, (float*)ws, B, N, cl_group_for<CL>(B, N), sin_dim, lim_enc, elu);
    if (rc) return rc;
    STOVE_LAUNCH(reduce_chunks_k, dim3((GC<CL>::kGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, GC<CL>::kGrads, nb, 0);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
}

int stove_dynloop_fwd_cl(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                         const float* params, float* z, float* zdyn, float* zdstd, float* mean, float* std_, float* pred,
                         int cl, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                         void* stream) {
  STOVE_VALIDATE(dynloop_fwd(z1, zsup, zsstd, eps, extra, params, z, zdyn, zdstd, mean, std_, B, Ts, N, sin_dim, stove_validate::gnn_limits_cl(cl)));
  if (B == 0 || Ts == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    return STOVE_LAUNCH_LDS(gnn_cl_loop_fwd_k<CL>, dim3(cl_blocks<CL>(B, N)), dim3(256), GC<CL>::kLdsFloats * sizeof(float), (hipStream_t)stream,
                            z1, zsup, zsstd, eps, extra, params, z, zdyn, zdstd, mean, std_, pred, B, Ts, N, cl_group_for<CL>(B, N), sin_dim,
                            lim_enc, elu, kc);
  });
}

int stove_dynloop_bwd_cl(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                         const float* params, const float* z, const float* dz, const float* dzdyn, const float* dmean,
                         const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd, float* dextra,
                         float* g_params, void* ws, int cl, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                         float vel_std, float lat_std, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(dynloop_bwd(z1, zsup, zsstd, eps, extra, params, z, dz1, dzsup, dzsstd, dextra, g_params, ws, B, Ts, N, sin_dim,
                             stove_validate::gnn_limits_cl(cl)));
  LoopConst kc{pos_var, vel_std, lat_std};
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    if (B == 0 || Ts == 0) return (int)hipMemsetAsync(g_params, 0, GC<CL>::kGrads * sizeof(float), st);
    const int nb = cl_blocks<CL>(B, N);
    int rc = STOVE_LAUNCH_LDS(gnn_cl_loop_bwd_k<CL>, dim3(nb), dim3(256), GC<CL>::kLdsFloats * sizeof(float), st, z1, zsup, zsstd, eps, extra,
                              params, z, dz, dzdyn, dmean, dstd, dpred, dz1, dzsup, dzsstd, dextra, (float*)ws, B, Ts, N,
                              cl_group_for<CL>(B, N), sin_dim, lim_enc, elu, kc);
    if (rc) return rc;
    STOVE_LAUNCH(reduce_chunks_k, dim3((GC<CL>::kGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, GC<CL>::kGrads, nb, 0);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
}

int stove_rollout_fwd_cl(const float* z_last, const float* extra, const float* params, float* z_pred, float* zstd, float* pred,
                         int cl, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std,
                         float lat_std, void* stream) {
  STOVE_VALIDATE(rollout_fwd(z_last, extra, params, z_pred, B, num, A, N, sin_dim, stove_validate::gnn_limits_cl(cl)));
  if (B == 0 || num == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    return STOVE_LAUNCH_LDS(gnn_cl_rollout_k<CL>, dim3(cl_blocks<CL>(B, N)), dim3(256), GC<CL>::kLdsFloats * sizeof(float), (hipStream_t)stream,
                            z_last, extra, params, z_pred, zstd, pred, B, num, A < 1 ? 1 : A, N, cl_group_for<CL>(B, N), sin_dim, lim_enc, elu,
                            kc);
  });
}

int stove_rollout_sample_fwd_cl(const float* z_last, const float* extra, const float* params, const float* eps, float* z_pred,
                                float* log_q, float* zstd, float* pred, int cl, int B, int num, int A, int N, int sin_dim, int lim_enc,
                                int elu, float pos_var, float vel_std, float lat_std, void* stream) {
  STOVE_VALIDATE(rollout_sample_fwd(z_last, extra, params, eps, z_pred, log_q, B, num, A, N, sin_dim, stove_validate::gnn_limits_cl(cl)));
  if (B == 0 || num == 0) return 0;
  LoopConst kc{pos_var, vel_std, lat_std};
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    return STOVE_LAUNCH_LDS(gnn_cl_rollout_sample_k<CL>, dim3(cl_blocks<CL>(B, N)), dim3(256), GC<CL>::kLdsFloats * sizeof(float),
                            (hipStream_t)stream, z_last, extra, params, eps, z_pred, log_q, zstd, pred, B, num, A < 1 ? 1 : A, N,
                            cl_group_for<CL>(B, N), sin_dim, lim_enc, elu, kc);
  });
}

size_t stove_rollout_bwd_ws_bytes_cl(int cl, int B, int N) { return stove_gnn_bwd_ws_bytes_cl(cl, B, N); }

int stove_rollout_bwd_cl(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                         const float* d_z_pred, const float* d_log_q, const float* d_pred, float* d_z_last, float* d_extra,
                         float* g_params, void* ws, int cl, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu,
                         float pos_var, float vel_std, float lat_std, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(rollout_bwd(z_last, extra, params, eps, z_pred, d_log_q, d_z_last, d_extra, g_params, ws, B, num, A, N, sin_dim,
                             stove_validate::gnn_limits_cl(cl)));
  LoopConst kc{pos_var, vel_std, lat_std};
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    using K = GC<CL>;
    if (B == 0 || num == 0) return rollout_bwd_empty(d_z_last, d_extra, g_params, K::ZW, K::kGrads, B, A, N, sin_dim - K::D, st);
    const int nb = cl_blocks<CL>(B, N);
    int rc = STOVE_LAUNCH_LDS(gnn_cl_rollout_bwd_k<CL>, dim3(nb), dim3(256), K::kLdsFloats * sizeof(float), st, z_last, extra, params, eps,
                              z_pred, d_z_pred, d_log_q, d_pred, d_z_last, d_extra, (float*)ws, B, num, A < 1 ? 1 : A, N,
                              cl_group_for<CL>(B, N), sin_dim, lim_enc, elu, kc);
    if (rc) return rc;
    STOVE_LAUNCH(reduce_chunks_k, dim3((K::kGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, K::kGrads, nb, 0);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
}

// ---------------------------------------------------------------- state-supervised baseline (gnn_sup.hip)
int stove_sup_rollout_fwd(const float* x, const float* latent0, const float* params, float* pred, float* codes, int cl, int B, int V,
                          int R, int N, int elu, void* stream) {
  STOVE_VALIDATE(sup_rollout_fwd(x, latent0, params, pred, cl, B, V, R, N));
  if (B == 0) return 0;
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    return STOVE_LAUNCH_LDS(gnn_sup_rollout_k<CL>, dim3(cl_blocks<CL>(B, N)), dim3(256), SupC<CL>::kLdsFloats * sizeof(float), (hipStream_t)stream,
                            x, latent0, params, pred, codes, B, V, R, N, cl_group_for<CL>(B, N), elu);
  });
}

size_t stove_sup_rollout_bwd_ws_bytes(int cl, int B, int N) { return stove_gnn_bwd_ws_bytes_cl(cl, B, N); }

int stove_sup_rollout_bwd(const float* x, const float* params, const float* codes, const float* d_pred, float* d_latent0,
                          float* g_params, void* ws, int cl, int B, int V, int R, int N, int elu, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(sup_rollout_bwd(x, params, codes, d_pred, g_params, ws, cl, B, V, R, N));
  return with_cl(cl, [&](auto w) {
    constexpr int CL = decltype(w)::value;
    using K = GC<CL>;
    if (B == 0) return (int)hipMemsetAsync(g_params, 0, K::kGrads * sizeof(float), st);
    const int nb = cl_blocks<CL>(B, N);
    int rc = STOVE_LAUNCH_LDS(gnn_sup_rollout_bwd_k<CL>, dim3(nb), dim3(256), SupC<CL>::kLdsFloats * sizeof(float), st, params, codes, d_pred,
                              d_latent0, (float*)ws, B, V, R, N, cl_group_for<CL>(B, N), elu);
    if (rc) return rc;
    STOVE_LAUNCH(reduce_chunks_k, dim3((K::kGrads + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, K::kGrads, nb, 0);
    STOVE_LAUNCH_CHECK();
    return 0;
  });
}

int stove_sup_loss(const float* pred, const float* future, float* losses, float* d_pred, int B, int R, int N, int end, int with_delta,
                   double discount, void* stream) {
  STOVE_VALIDATE(sup_loss(pred, future, losses, d_pred, B, R, N, end));
  STOVE_LAUNCH(sup_loss_k, dim3(1), dim3(kSupLossThreads), 0, (hipStream_t)stream, pred, future, losses, d_pred, B, R, N, end, with_delta, discount);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- flat parameter arena
static SpnArenaPlan arena_plan(const StoveSpnArenaPlan* p) {
  SpnArenaPlan q;
  q.obj_mu = p->obj_mu; q.obj_rho = p->obj_rho; q.obj_sum = p->obj_sum;
  q.bg_mu = p->bg_mu; q.bg_rho = p->bg_rho; q.bg_gidx = p->bg_gidx;
  q.obj_root = p->obj_root; q.bg_root = p->bg_root;
  q.obj_vmin = p->obj_vmin; q.obj_vmax = p->obj_vmax; q.bg_vmin = p->bg_vmin; q.bg_vmax = p->bg_vmax;
  return q;
}

int stove_spn_bake(const float* arena, const StoveSpnArenaPlan* plan, float* obj_coef, float* obj_wsum, float* obj_wroot,
                   float* bg_coef, float* bg_wroot, void* stream) {
  const int nb = (kAObjCoef + kABgCoef + 255) / 256;
  STOVE_LAUNCH(spn_bake_k, dim3(nb + kASoftBlocks), dim3(256), 0, (hipStream_t)stream, arena, arena_plan(plan), obj_coef, obj_wsum, obj_wroot,
               bg_coef, bg_wroot, nb);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_spn_bake_bwd(const float* arena, const StoveSpnArenaPlan* plan, const StoveSpnTableGrads* g, float* grad_arena, void* stream) {
  const int nb = (kAObjCoef + kABgCoef + 255) / 256;
  STOVE_LAUNCH(spn_bake_bwd_k, dim3(nb + kASoftBlocks), dim3(256), 0, (hipStream_t)stream, arena, arena_plan(plan), (const float*)g->obj_coef,
               (const float*)g->obj_wsum, (const float*)g->obj_wroot, (const float*)g->bg_coef, (const float*)g->bg_wroot, grad_arena, nb);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_arena_gather(const float* arena, const int32_t* src, float* image, int n, void* stream) {
  if (n == 0) return 0;
  STOVE_LAUNCH(arena_gather_k, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, arena, src, image, n);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_arena_scatter_add(const float* gimage, const int32_t* src, float* grad_arena, int n, void* stream) {
  if (n == 0) return 0;
  STOVE_LAUNCH(arena_scatter_add_k, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, gimage, src, grad_arena, n);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_sum_chunks(const float* parts, float* out, size_t n, int chunks, void* stream) {
  if (n == 0) return 0;
  if (n % 4 != 0 || chunks < 1) return (int)hipErrorInvalidValue;
  const int n4 = (int)(n / 4);
  STOVE_LAUNCH(sum_chunks4_k, dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, parts, out, n4, chunks, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

size_t stove_gemm_bf16_ws_floats(int M, int N, int splitk) { return splitk > 1 ? (size_t)splitk * M * N : 0; }

int stove_gemm_bf16(const float* A, const float* B, const float* bias, const float* add, float* C, int M, int N, int K, int lda,
                    int ldb, int ldc, int a_kmajor, int b_kmajor, int nsplit, int splitk, int tile, float* ws, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  STOVE_VALIDATE(gemm(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, nsplit, splitk, ws));
  if (M == 0 || N == 0) return 0;
  if (K <= 0 || splitk < 1 || nsplit < 1 || nsplit > 3 || tile < 0 || (tile > 3 && (tile < 11 || tile > 15))) return (int)hipErrorInvalidValue;
  // tile 11 / 12: measurement variants of the 256 x 128 NT kernel (tools/gemm_bf16_bench.py): no loads in the loop / no MFMAs
  if (tile == 11 && !a_kmajor && !b_kmajor && nsplit == 2) return gemm_launch<false, false, 2, 256, 128, 1>(A, B, bias, add, C, M, N, K, lda, ldb, ldc, 1, st);
  if (tile == 12 && !a_kmajor && !b_kmajor && nsplit == 2) return gemm_launch<false, false, 2, 256, 128, 2>(A, B, bias, add, C, M, N, K, lda, ldb, ldc, 1, st);
  // 13 / 14: the same two variants of the 256 x 256 tile
  if (tile == 13 && !a_kmajor && !b_kmajor && nsplit == 2) return gemm_launch<false, false, 2, 256, 256, 1, false, 64, 128>(A, B, bias, add, C, M, N, K, lda, ldb, ldc, 1, st);
  if (tile == 14 && !a_kmajor && !b_kmajor && nsplit == 2) return gemm_launch<false, false, 2, 256, 256, 2, false, 64, 128>(A, B, bias, add, C, M, N, K, lda, ldb, ldc, 1, st);
  if (tile == 15 && !a_kmajor && !b_kmajor && nsplit == 2) return gemm_launch<false, false, 2, 256, 256, 3, false, 64, 128>(A, B, bias, add, C, M, N, K, lda, ldb, ldc, 1, st);
  if (tile > 3) tile = 1;
  // float4 granularity along the contiguous dimension of an operand / of C, or the element-wise slow path for it
  // (fc1 of the recognition network has 50 columns)
  auto odd = [](const void* p, int ld, int extent) { return ((uintptr_t)p & 15) != 0 || (ld & 3) != 0 || (extent & 3) != 0; };
  const int scalar_bits = (odd(A, lda, a_kmajor ? M : K) ? 1 : 0) | (odd(B, ldb, b_kmajor ? N : K) ? 2 : 0) |
                          ((odd(C, ldc, N) || (bias != nullptr && ((uintptr_t)bias & 15)) || (add != nullptr && ((uintptr_t)add & 15))) ? 4 : 0);
  // split-K: no epilogue terms, except add == C (accumulate into C, e.g. a gradient view), applied by the slice sum
  const bool acc_c = splitk > 1 && add != nullptr && add == C;
  if (acc_c) add = nullptr;
  // ... or a dense (M x N, float4-addressable) add term of fewer than 16 slices: added by the slice sum, like the bias
  const float* sum_add = (splitk > 1 && splitk < 16 && add != nullptr && (((uintptr_t)add & 15) == 0)) ? add : nullptr;
  if (sum_add != nullptr) add = nullptr;
  const float* sum_bias = splitk > 1 ? bias : nullptr;      // split-K: the bias is added by the slice sum (fewer than 16 slices)
  if (splitk > 1 && splitk < 16) bias = nullptr;
  if (splitk > 1 && (ws == nullptr || bias != nullptr || add != nullptr || ldc != N || (scalar_bits & 4))) return (int)hipErrorInvalidValue;
  if (scalar_bits & 2) return (int)hipErrorInvalidValue;           // B has to be float4-addressable
  float* out = splitk > 1 ? ws : C;
  const int ldo = splitk > 1 ? N : ldc;
  if (tile == 0) tile = 1;
  int rc;
  if (nsplit == 3) {
    // round 5: hi / lo pieces in IEEE half instead of bf16 (11 + 11 significant bits: the product is as good as an fp32 one) for
    // operands inside half's range -- the forward products x W_ih^T, h W_hh^T of the recognition network.  K-contiguous,
    // float4-addressable operands.
    if (a_kmajor || b_kmajor || scalar_bits) return (int)hipErrorInvalidValue;
    rc = tile == 3 ? gemm_launch<false, false, 2, 256, 256, 0, false, 64, 128, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)
       : tile == 1 ? gemm_launch<false, false, 2, 256, 128, 0, false, 64, 64, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)
                   : gemm_launch<false, false, 2, 128, 128, 0, false, 64, 64, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits);
  } else if (scalar_bits & 1) {        // element-wise A: the two layouts fc1's backward needs (d_a1 W1 and d_a1^T h), 128 x 128 tile
    if (!b_kmajor) return (int)hipErrorInvalidValue;
    if (a_kmajor) rc = nsplit == 2 ? gemm_launch<true, true, 2, 128, 128, 0, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)
                                   : gemm_launch<true, true, 1, 128, 128, 0, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits);
    else rc = nsplit == 2 ? gemm_launch<false, true, 2, 128, 128, 0, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)
                          : gemm_launch<false, true, 1, 128, 128, 0, true>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits);
  } else {
#define STOVE_GEMM_TILE(AK, BK_, NS)                                                                                \
  rc = tile == 3 ? gemm_launch<AK, BK_, NS, 256, 256, 0, false, 64, 128>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)           \
     : tile == 1 ? gemm_launch<AK, BK_, NS, 256, 128>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)           \
                 : gemm_launch<AK, BK_, NS, 128, 128>(A, B, bias, add, out, M, N, K, lda, ldb, ldo, splitk, st, scalar_bits)
#define STOVE_GEMM_CASE(AK, BK_)             \
  do {                                       \
    if (nsplit == 2) {                       \
      STOVE_GEMM_TILE(AK, BK_, 2);           \
    } else {                                 \
      STOVE_GEMM_TILE(AK, BK_, 1);           \
    }                                        \
  } while (0)
  if (!a_kmajor && !b_kmajor) STOVE_GEMM_CASE(false, false);
  else if (!a_kmajor && b_kmajor) STOVE_GEMM_CASE(false, true);
  else if (a_kmajor && b_kmajor) STOVE_GEMM_CASE(true, true);
  else STOVE_GEMM_CASE(true, false);
  }
#undef STOVE_GEMM_CASE
#undef STOVE_GEMM_TILE
  if (rc) return rc;
  if (splitk > 1) {
    const int n4 = (int)((size_t)M * N / 4);
    if (splitk >= 16)
      STOVE_LAUNCH(sum_chunks4_par_k, dim3((n4 + 63) / 64), dim3(256), 0, st, (const float*)ws, C, n4, splitk, acc_c ? 1 : 0);
    else
      STOVE_LAUNCH(sum_chunks4_k, dim3((n4 + 255) / 256), dim3(256), 0, st, (const float*)ws, C, n4, splitk, acc_c ? 1 : 0, sum_bias, N / 4, sum_add);
    STOVE_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------- reward head of the action-conditioned model
size_t stove_reward_head_param_floats(void) { return (size_t)kRhParams; }
size_t stove_reward_head_saved_floats(int items, int n_obj) { return (size_t)items * ((size_t)n_obj * 32 + 32 + 16 + 8); }
static int reward_head_blocks(int items) {
  const int b = (items + kRhWaves - 1) / kRhWaves;
  return b < 1 ? 1 : (b > 256 ? 256 : b);
}
size_t stove_reward_head_bwd_ws_floats(int items) { return (size_t)reward_head_blocks(items) * kRhWaves * kRhParams; }

int stove_reward_head_fwd(const float* pred, const float* params, float* reward, float* saved, int items, int n_obj, void* stream) {
  if (items == 0) return 0;
  if (n_obj < 1 || pred == nullptr || params == nullptr || reward == nullptr || saved == nullptr) return (int)hipErrorInvalidValue;
  float* H0 = saved;
  float* Q = H0 + (size_t)items * n_obj * 32;
  float* A1 = Q + (size_t)items * 32;
  float* A2 = A1 + (size_t)items * 16;
  STOVE_LAUNCH(reward_head_fwd_k, dim3(reward_head_blocks(items)), dim3(64 * kRhWaves), 0, (hipStream_t)stream, pred, params, reward, H0, Q, A1, A2,
               items, n_obj);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_reward_head_bwd(const float* pred, const float* params, const float* reward, const float* saved, const float* d_reward, float* d_pred,
                          float* g_params, float* ws, int items, int n_obj, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (items == 0) {
    (void)hipMemsetAsync(g_params, 0, kRhParams * sizeof(float), st);
    return 0;
  }
  if (n_obj < 1 || ws == nullptr || d_pred == nullptr || g_params == nullptr) return (int)hipErrorInvalidValue;
  const float* H0 = saved;
  const float* Q = H0 + (size_t)items * n_obj * 32;
  const float* A1 = Q + (size_t)items * 32;
  const float* A2 = A1 + (size_t)items * 16;
  const int blocks = reward_head_blocks(items);
  STOVE_LAUNCH(reward_head_bwd_k, dim3(blocks), dim3(64 * kRhWaves), 0, st, pred, params, reward, H0, Q, A1, A2, d_reward, d_pred, ws, items, n_obj);
  STOVE_LAUNCH_CHECK();
  STOVE_LAUNCH(reduce_chunks_k, dim3((kRhParams + 31) / 32), dim3(256), 0, st, (const float*)ws, g_params, kRhParams, blocks * kRhWaves, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_small_linear(const float* x, const float* W, const float* b, float* y, int rows, int in_dim, int out_dim, int w_transposed, void* stream) {
  if (rows == 0) return 0;
  if (in_dim < 1 || out_dim < 1 || in_dim > 64 || out_dim > 64) return (int)hipErrorInvalidValue;
  const size_t total = (size_t)rows * out_dim;
  if ((total + 255) / 256 > 0x7fffffffULL) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(small_linear_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, W, b, y, rows, in_dim, out_dim, w_transposed);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- planning: one expansion of M search trees (plan.hip)
size_t stove_reward_head_param_floats_cl(int cl) { return cl == 16 ? RhCl<16>::kParams : (cl == 64 ? RhCl<64>::kParams : 0); }

namespace {
struct PlanWs {
  size_t z_in, extra, z_pred, pred, ok, bytes;          // byte offsets
  PlanWs(int cl, int M, int A, int L, int N, int app_dim) {
    const size_t rows = (size_t)M * A, steps = 1 + (size_t)L, zw = (size_t)cl / 2 + 2;
    z_in = 0;
    extra = z_in + align64(rows * N * zw * sizeof(float));
    z_pred = extra + align64(rows * steps * N * (4 + app_dim) * sizeof(float));
    pred = z_pred + align64(rows * steps * N * zw * sizeof(float));
    ok = pred + align64(rows * steps * N * cl * sizeof(float));
    bytes = ok + align64((size_t)M * sizeof(int));
  }
};
}  // namespace

size_t stove_plan_expand_ws_bytes(int M, int A, int L, int N, int app_dim) {
  return stove_validate::plan_dims_bad(M, A, L, N, app_dim) ? 0 : PlanWs(32, M, A, L, N, app_dim).bytes;
}
size_t stove_plan_expand_ws_bytes_cl(int cl, int M, int A, int L, int N, int app_dim) {
  return stove_validate::plan_dims_bad(M, A, L, N, app_dim, stove_validate::gnn_limits_cl(cl)) ? 0 : PlanWs(cl, M, A, L, N, app_dim).bytes;
}

// the three launches of one expansion at state-code length cl = 16 / 32 / 64 (arguments validated by the caller)
static int plan_expand_launch(float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app, const int* acts,
                              const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, float* q, float* r_first,
                              float* r_roll, void* ws, int cl, int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                              float pos_var, float vel_std, float lat_std, float gamma, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const PlanWs w(cl, M, A, L, N, app_dim);
  char* base = (char*)ws;
  float* z_in = (float*)(base + w.z_in);
  float* extra = (float*)(base + w.extra);
  float* z_pred = (float*)(base + w.z_pred);
  float* pred = (float*)(base + w.pred);
  int* ok = (int*)(base + w.ok);
  const int rows = M * A, sin_dim = cl / 2 + 4 + app_dim;
  STOVE_LAUNCH(plan_prep_k, dim3(M), dim3(kPlanPrepThreads), 0, st, (const float*)z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, z_in, extra,
               ok, cap, A, L, D, N, app_dim, cl / 2 + 2);
  STOVE_LAUNCH_CHECK();
  const int rc = cl == 32 ? stove_rollout_fwd(z_in, extra, gnn_params, z_pred, nullptr, pred, rows, 1 + L, 1 + L, N, sin_dim, lim_enc, elu, pos_var,
                                              vel_std, lat_std, stream)
                          : stove_rollout_fwd_cl(z_in, extra, gnn_params, z_pred, nullptr, pred, cl, rows, 1 + L, 1 + L, N, sin_dim, lim_enc, elu,
                                                 pos_var, vel_std, lat_std, stream);
  if (rc) return rc;
#define STOVE_PLAN_FINISH(CL)                                                                                                               \
  STOVE_LAUNCH(plan_finish_k<CL>, dim3(reward_head_blocks(rows)), dim3(64 * kRhWaves), 0, st, (const float*)pred, (const float*)z_pred, rh_params, \
               (const int*)ok, child, len_s, z_pool, q, r_first, r_roll, rows, cap, A, L, D, N, gamma)
  if (cl == 32) STOVE_PLAN_FINISH(32);
  else if (cl == 16) STOVE_PLAN_FINISH(16);
  else STOVE_PLAN_FINISH(64);
#undef STOVE_PLAN_FINISH
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_plan_expand(float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app, const int* acts,
                      const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, float* q, float* r_first,
                      float* r_roll, void* ws, int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu, float pos_var,
                      float vel_std, float lat_std, float gamma, void* stream) {
  STOVE_VALIDATE(plan_expand(z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, ws, M, cap, A, L, D, N, app_dim));
  return plan_expand_launch(z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, r_first, r_roll, ws, 32, M, cap, A, L, D,
                            N, app_dim, lim_enc, elu, pos_var, vel_std, lat_std, gamma, stream);
}

int stove_plan_expand_cl(float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app, const int* acts,
                         const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, float* q, float* r_first,
                         float* r_roll, void* ws, int cl, int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                         float pos_var, float vel_std, float lat_std, float gamma, void* stream) {
  STOVE_VALIDATE(plan_expand(z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, ws, M, cap, A, L, D, N, app_dim,
                             stove_validate::gnn_limits_cl(cl)));
  return plan_expand_launch(z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, r_first, r_roll, ws, cl, M, cap, A, L, D,
                            N, app_dim, lim_enc, elu, pos_var, vel_std, lat_std, gamma, stream);
}

// ---------------------------------------------------------------- planning: a whole search, the trees on the device (plan_tree.hip)
namespace {
struct PlanSearchWs {          // the expansion's workspace, then q (M, A), the index vectors select writes and its walk's gap (M,) double
  size_t q, leaf, child, len_s, gap, bytes;
  PlanSearchWs(int cl, int M, int A, int L, int N, int app_dim) {
    q = PlanWs(cl, M, A, L, N, app_dim).bytes;
    leaf = q + align64((size_t)M * A * sizeof(float));
    child = leaf + align64((size_t)M * sizeof(int));
    len_s = child + align64((size_t)M * sizeof(int));
    gap = len_s + align64((size_t)M * sizeof(int));
    bytes = gap + align64((size_t)M * sizeof(double));
  }
};
}  // namespace

size_t stove_plan_search_ws_bytes(int M, int A, int L, int N, int app_dim) {
  return stove_validate::plan_dims_bad(M, A, L, N, app_dim) ? 0 : PlanSearchWs(32, M, A, L, N, app_dim).bytes;
}
size_t stove_plan_search_ws_bytes_cl(int cl, int M, int A, int L, int N, int app_dim) {
  return stove_validate::plan_dims_bad(M, A, L, N, app_dim, stove_validate::gnn_limits_cl(cl)) ? 0 : PlanSearchWs(cl, M, A, L, N, app_dim).bytes;
}

// the 5 R + 1 launches of one search at state-code length cl (arguments validated by the caller)
static int plan_search_launch(float* z_pool, int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap,
                              int* status, int* action, int* sel_trace, const float* app, const int* acts, const float* emb_w,
                              const float* emb_b, const float* gnn_params, const float* rh_params, void* ws, int cl, int M, int cap, int A, int L,
                              int D, int N, int app_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std, float gamma, int R,
                              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const PlanSearchWs w(cl, M, A, L, N, app_dim);
  char* base = (char*)ws;
  float* q = (float*)(base + w.q);
  int* leaf = (int*)(base + w.leaf);
  int* child = (int*)(base + w.child);
  int* len_s = (int*)(base + w.len_s);
  double* gap = (double*)(base + w.gap);
  const int* ok = (const int*)(base + PlanWs(cl, M, A, L, N, app_dim).ok);
  const double c = 1.0;          // the reference's exploration constant (MCTS.c)
  for (int i = 0; i < R; ++i) {
    STOVE_LAUNCH(plan_tree_select_k, dim3(M), dim3(64), 0, st, first, parent, depth, Ns, Nsa, Qsa, used, gap, status, leaf, child, len_s,
                 sel_trace != nullptr ? sel_trace + (size_t)i * M : nullptr, c, cap, A, D);
    STOVE_LAUNCH_CHECK();
    const int rc = plan_expand_launch(z_pool, leaf, child, len_s, app, acts + (size_t)i * M * A * L, emb_w, emb_b, gnn_params, rh_params, q, nullptr,
                                      nullptr, ws, cl, M, cap, A, L, D, N, app_dim, lim_enc, elu, pos_var, vel_std, lat_std, gamma, stream);
    if (rc) return rc;
    STOVE_LAUNCH(plan_tree_backprop_k, dim3(M), dim3(64), 0, st, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, (const int*)leaf,
                 (const int*)child, (const double*)gap, (const float*)q, ok, cap, A, D);
    STOVE_LAUNCH_CHECK();
  }
  STOVE_LAUNCH(plan_tree_action_k, dim3((M + 63) / 64), dim3(64), 0, st, first, Nsa, action, M, cap, A);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_plan_search(float* z_pool, int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap,
                      int* status, int* action, int* sel_trace, const float* app, const int* acts, const float* emb_w, const float* emb_b,
                      const float* gnn_params, const float* rh_params, void* ws, int M, int cap, int A, int L, int D, int N, int app_dim,
                      int lim_enc, int elu, float pos_var, float vel_std, float lat_std, float gamma, int R, void* stream) {
  STOVE_VALIDATE(plan_search(z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, app, acts, emb_w, emb_b, gnn_params,
                             rh_params, ws, M, cap, A, L, D, N, app_dim, R));
  return plan_search_launch(z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, sel_trace, app, acts, emb_w, emb_b,
                            gnn_params, rh_params, ws, 32, M, cap, A, L, D, N, app_dim, lim_enc, elu, pos_var, vel_std, lat_std, gamma, R, stream);
}

int stove_plan_search_cl(float* z_pool, int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap,
                         int* status, int* action, int* sel_trace, const float* app, const int* acts, const float* emb_w, const float* emb_b,
                         const float* gnn_params, const float* rh_params, void* ws, int cl, int M, int cap, int A, int L, int D, int N,
                         int app_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std, float gamma, int R, void* stream) {
  STOVE_VALIDATE(plan_search(z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, app, acts, emb_w, emb_b, gnn_params,
                             rh_params, ws, M, cap, A, L, D, N, app_dim, R, stove_validate::gnn_limits_cl(cl)));
  return plan_search_launch(z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, sel_trace, app, acts, emb_w, emb_b,
                            gnn_params, rh_params, ws, cl, M, cap, A, L, D, N, app_dim, lim_enc, elu, pos_var, vel_std, lat_std, gamma, R, stream);
}

// ---------------------------------------------------------------- the environments the planner plays: step and frame (env.hip)
static_assert(stove_validate::kEnvMaxObjects == env_step::kMaxObjects, "validate.h admits what env_step.h holds");
int stove_env_step(double* x, double* v, const double* r, const double* m, const int* action, int* collisions, int* status, float* frames,
                   int M, int N, int granularity, int res, int use_colors, int drift, double hw, double t, double friction,
                   double action_force, void* stream) {
  STOVE_VALIDATE(env_step(x, v, r, m, collisions, status, M, N, granularity, res));
  if (M == 0) return 0;
  const env_step::Params p{N, granularity, drift != 0 ? 1 : 0, hw, t, friction, action_force};
  STOVE_LAUNCH(env_step_k, dim3(M), dim3(kEnvThreads), 0, (hipStream_t)stream, x, v, r, m, action, collisions, status, frames, p, res,
               use_colors != 0 ? 1 : 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- data synthesis: whole sequences in one launch (env_sequences.hip)
int stove_env_sequences(const double* x0, const double* v0, const double* r, const double* m, const int* actions, double* y, float* frames,
                        int* collisions, int* in_bounds, int* status, int B, int N, int T, int granularity, int res, int use_colors,
                        int drift, int kind, double hw, double t, double friction, double action_force, void* stream) {
  STOVE_VALIDATE(env_sequences(x0, v0, r, m, actions, y, collisions, in_bounds, status, B, N, T, granularity, res, kind));
  if (B == 0) return 0;
  const env_step::Params p{N, granularity, drift != 0 ? 1 : 0, hw, t, friction, action_force};
  STOVE_LAUNCH(env_sequences_k, dim3(B), dim3(kSeqThreads), 0, (hipStream_t)stream, x0, v0, r, m, actions, y, frames, collisions, in_bounds,
               status, p, T, res, use_colors != 0 ? 1 : 0, kind);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- data synthesis: starts and action rows drawn in one launch (env_draw.hip)
int stove_env_draw_starts(const double* r, double* x0, double* v0, int* actions, int* tries, int* status, uint32_t seed_lo, uint32_t seed_hi,
                          int B, int N, int T, int kind, int max_tries, double hw, double v_factor, void* stream) {
  STOVE_VALIDATE(env_draw_starts(r, x0, v0, tries, status, B, N, T, kind, max_tries));
  if (B == 0) return 0;
  const uint64_t seed0 = ((uint64_t)seed_hi << 32) | seed_lo;
  const int rc = with_count<6>(N, [&](auto n) {
    STOVE_LAUNCH(env_draw_starts_k<decltype(n)::value>, dim3((B + kDrawWaves - 1) / kDrawWaves), dim3(kDrawThreads), 0, (hipStream_t)stream,
                 r, x0, v0, actions, tries, status, seed0, B, T, kind, max_tries, hw, v_factor);
    return 0;
  });
  if (rc) return rc;
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- planning on the true environment: a whole search in one launch (env_search.hip)
static_assert(stove_validate::kEnvActions == env_search::kActions, "validate.h sizes the trees for env_search.h's action count");
int stove_env_search(const double* x, const double* v, const double* r, const double* m, const int* draws, int* first, int* parent, int* depth,
                     int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap, int* status, int* action, int M, int R, int N, int D,
                     int runs, int cap, int granularity, int drift, double hw, double t, double friction, double action_force, void* stream) {
  STOVE_VALIDATE(env_search(x, v, r, m, draws, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, M, R, N, D, runs, cap,
                            granularity));
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int T = M * R;
  const env_step::Params p{N, granularity, drift != 0 ? 1 : 0, hw, t, friction, action_force};
  if (runs > 0) {
    const int rc = with_count<6>(N,[&](auto n) {
      env_search_launch<decltype(n)::value>(st, T, x, v, r, m, draws, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, p, R, runs, cap, D);
      return 0;
    });
    if (rc) return rc;
    STOVE_LAUNCH_CHECK();
  }
  STOVE_LAUNCH(env_search_action_k, dim3((M + kEnvSearchThreads - 1) / kEnvSearchThreads), dim3(kEnvSearchThreads), 0, st, (const int*)first,
               (const int*)Nsa, action, M, R, cap);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- the PPO arm: a batch of trajectories in one launch (ppo_collect.hip)
static_assert(stove_validate::kPpoMaxHidden == ppo_policy::kMaxHidden, "validate.h admits what ppo_policy.h holds");
size_t stove_ppo_param_floats(int N, int H, int deep) {
  if (N < 1 || N > env_step::kMaxObjects || H < 1 || H > ppo_policy::kMaxHidden) return 0;
  return ppo_policy::param_floats(ppo_policy::Shape{N, H, deep != 0 ? 1 : 0});
}
int stove_ppo_collect(double* x, double* v, const double* r, const double* m, const float* params, const float* u, float* obs, int* actions,
                      float* rewards, float* values, float* logp, float* next_value, float* returns, int* status, int B, int S, int N, int H,
                      int deep, int granularity, int drift, double hw, double t, double friction, double action_force, double discount,
                      void* stream) {
  STOVE_VALIDATE(ppo_collect(x, v, r, m, params, u, obs, actions, rewards, values, logp, next_value, returns, status, B, S, N, H, granularity));
  if (B == 0) return 0;
  const env_step::Params p{N, granularity, drift != 0 ? 1 : 0, hw, t, friction, action_force};
  const ppo_policy::Shape sh{N, H, deep != 0 ? 1 : 0};
  const size_t n = ppo_policy::param_floats(sh), lds = ppo_lds_bytes(n);
  const dim3 grid((B + kPpoWaves - 1) / kPpoWaves), block(kPpoThreads);
  return with_flag(ppo_staged(n), [&](auto staged) {
    return STOVE_LAUNCH_LDS(ppo_collect_k<decltype(staged)::value>, grid, block, lds, (hipStream_t)stream, x, v, r, m, params, u, obs, actions, rewards,
                            values, logp, next_value, returns, status, p, sh, B, S, (float)discount, (int)n);
  });
}

// ---------------------------------------------------------------- the model-based PPO arm: imagined trajectories in one launch (ppo_model.hip)
// the launch of both entry points on a validated argument block: cl = 32 on the small-graph step (one object on gnn_forward), cl = 16 /
// 64 on cl_forward (ppo_model_cl.hip), one kernel per width for every object count
static int ppo_collect_model_launch(int cl, PmArgs A, float pos_var, float vel_std, float lat_std, void* stream) {
  if (A.B == 0) return 0;
  (void)pos_var; (void)vel_std; (void)lat_std;          // (the scales of the predicted deviations, which this rollout does not put out)
  const size_t n = ppo_policy::param_floats(A.sh);
  A.n_params = (int)n;
  const dim3 grid(A.B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (cl != 32)
    return with_cl(cl, [&](auto w) {
      constexpr int CL = decltype(w)::value;
      A.staged = pc_staged<CL>(n) ? 1 : 0;
      return STOVE_LAUNCH_LDS(ppo_collect_model_cl_k<CL>, grid, block, pc_lds_bytes<CL>(n), st, PM_LAUNCH_ARGS(A));
    });
  if (!small_graph(A.N))          // one object: gnn_forward's arithmetic, as stove_rollout_fwd steps it
    return STOVE_LAUNCH_LDS(ppo_collect_model_one_k, grid, block, kPm1LdsBytes, st, PM_LAUNCH_ARGS(A));
  return with_small_graph<false>(A.N, A.elu != 0, false, [&](auto nmx, auto e, auto nt) {
    constexpr int NMX = decltype(nmx)::value;
    A.staged = pm_staged<NMX>(n) ? 1 : 0;
    return STOVE_LAUNCH_LDS((ppo_collect_model_k<NMX, decltype(e)::value, decltype(nt)::value>), grid, block, pm_lds_bytes<NMX>(n), st, PM_LAUNCH_ARGS(A));
  });
}

int stove_ppo_collect_model(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                            const float* gnn_params, const float* rh_params, const float* u, float* z_pred, float* pred, float* obs,
                            int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status, int B,
                            int S, int N, int H, int deep, int app_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                            float hw, float discount, void* stream) {
  STOVE_VALIDATE(ppo_collect_model(z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, obs, actions, rewards, values, logp,
                                   next_value, returns, status, B, S, N, H, app_dim, lim_enc));
  return ppo_collect_model_launch(32, PmArgs{z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, pred, obs, actions, rewards,
                                             values, logp, next_value, returns, status, {N, H, deep != 0 ? 1 : 0}, B, S, N, app_dim, lim_enc,
                                             elu != 0 ? 1 : 0, hw, discount, 0, 0},
                                  pos_var, vel_std, lat_std, stream);
}

// the same at state-code lengths 16 / 64
int stove_ppo_collect_model_cl(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                               const float* gnn_params, const float* rh_params, const float* u, float* z_pred, float* pred, float* obs,
                               int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status,
                               int cl, int B, int S, int N, int H, int deep, int app_dim, int lim_enc, int elu, float pos_var, float vel_std,
                               float lat_std, float hw, float discount, void* stream) {
  STOVE_VALIDATE(ppo_collect_model_cl(z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, obs, actions, rewards, values,
                                      logp, next_value, returns, status, B, S, N, H, app_dim, lim_enc, stove_validate::gnn_limits_cl(cl)));
  return ppo_collect_model_launch(cl, PmArgs{z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, pred, obs, actions, rewards,
                                             values, logp, next_value, returns, status, {N, H, deep != 0 ? 1 : 0}, B, S, N, app_dim, lim_enc,
                                             elu != 0 ? 1 : 0, hw, discount, 0, 0},
                                  pos_var, vel_std, lat_std, stream);
}

// ---------------------------------------------------------------- the PPO arm on images: a batch of trajectories in one launch (ppo_image.hip)
static_assert(stove_validate::kImgMaxFrames == ppo_image::kMaxFrames && stove_validate::kImgMaxHidden == ppo_image::kMaxHidden,
              "validate.h admits what ppo_image.h holds");
size_t stove_ppo_image_param_floats(int F, int H, int deep) {
  const ppo_image::Shape sh{F, H, deep != 0 ? 1 : 0};
  return ppo_image::served(sh) ? ppo_image::param_floats(sh) : 0;
}
int stove_ppo_collect_images(double* x, double* v, const double* r, const double* m, const float* params, const float* u, float* frames,
                             int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status, int B,
                             int S, int N, int F, int H, int deep, int warm, int granularity, int drift, int use_colors, double hw, double t,
                             double friction, double action_force, double discount, void* stream) {
  STOVE_VALIDATE(ppo_collect_images(x, v, r, m, params, u, frames, actions, rewards, values, logp, next_value, returns, status, B, S, N, F, H,
                                    warm, granularity));
  if (B == 0) return 0;
  const env_step::Params p{N, granularity, drift != 0 ? 1 : 0, hw, t, friction, action_force};
  const ppo_image::Shape sh{F, H, deep != 0 ? 1 : 0};
  return STOVE_LAUNCH_LDS(ppo_collect_images_k, dim3(B), dim3(kImgThreads), img_lds_bytes(F), (hipStream_t)stream, x, v, r, m, params, u, frames,
                          actions, rewards, values, logp, next_value, returns, status, p, sh, S, warm, use_colors != 0 ? 1 : 0, (float)discount);
}

// ---------------------------------------------------------------- the PPO arm: the whole update in one launch (ppo_update.hip)
int stove_ppo_update(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns,
                     const float* values, const float* logp, const float* adv, const int* perm, float* losses, float* gnorm, int* status, int n,
                     int E, int M, int max_steps, int N, int H, int deep, float clip, float value_coef, float entropy_coef, float lr, float eps,
                     float max_grad_norm, int clipped_value_loss, void* stream) {
  STOVE_VALIDATE(ppo_update(params, m, v, step, obs, actions, returns, values, logp, adv, perm, losses, gnorm, status, n, E, M, max_steps, N, H));
  const ppo_policy::Shape sh{N, H, deep != 0 ? 1 : 0};
  const ppo_update::Hyper hy{clip, value_coef, entropy_coef, lr, eps, max_grad_norm, clipped_value_loss != 0 ? 1 : 0};
  const size_t lds = upd_lds_bytes(sh);
  const dim3 grid(1), block(kUpdThreads);
  hipStream_t st = (hipStream_t)stream;
  return with_flag(upd_staged(sh), [&](auto staged) {
    return with_flag(sh.deep != 0, [&](auto dp) {
      return STOVE_LAUNCH_LDS(ppo_update_k<decltype(staged)::value, decltype(dp)::value>, grid, block, lds, st, params, m, v, step, obs, actions,
                              returns, values, logp, adv, perm, losses, gnorm, status, sh, hy, n, M, max_steps);
    });
  });
}

// ---------------------------------------------------------------- the PPO arm on images: the whole update in one call (ppo_image_update.hip)
size_t stove_ppo_update_images_ws_bytes(int n, int M, int F, int H, int deep) {
  const ppo_image::Shape sh{F, H, deep != 0 ? 1 : 0};
  if (!ppo_image::served(sh) || M < 1 || n < M) return 0;
  return piu_ws(n / M, sh).bytes;
}
int stove_ppo_update_images(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns,
                            const float* values, const float* logp, const float* adv, const int* perm, float* losses, float* gnorm, float* grad,
                            int* status, void* ws, int n, int S, int env_stride, int E, int M, int max_steps, int F, int H, int deep, float clip,
                            float value_coef, float entropy_coef, float lr, float eps, float max_grad_norm, int clipped_value_loss,
                            void* stream) {
  STOVE_VALIDATE(ppo_update_images(params, m, v, step, obs, actions, returns, values, logp, adv, perm, losses, gnorm, status, ws, n, S, env_stride,
                                   E, M, max_steps, F, H));
  const ppo_image::Shape sh{F, H, deep != 0 ? 1 : 0};
  const ppo_update::Hyper hy{clip, value_coef, entropy_coef, lr, eps, max_grad_norm, clipped_value_loss != 0 ? 1 : 0};
  return piu_run(params, m, v, step, obs, actions, returns, values, logp, adv, perm, losses, gnorm, grad, status, ws, n, S, env_stride, M,
                 max_steps, sh, hy, (hipStream_t)stream);
}

// ---------------------------------------------------------------- stream ordering / graph replay helpers
int stove_stream_after(void* to, void* from) { return (int)stream_after((hipStream_t)to, (hipStream_t)from); }

// Events that order two DIFFERENT captures against each other (stream_after) must live as long as the graphs holding their
// record / wait nodes.  A caller that captures opens a list first: every such event created while it is open is appended, and
// the caller destroys the list together with its graphs (stove_amd/graphed.py).  With no list open they are never destroyed.
void* stove_event_list_begin(void) {
  std::lock_guard<std::mutex> g(event_list_mu());
  auto* v = new std::vector<hipEvent_t>();
  event_list_current() = v;
  return (void*)v;
}
int stove_event_list_end(void* list) {
  std::lock_guard<std::mutex> g(event_list_mu());
  if (event_list_current() == (std::vector<hipEvent_t>*)list) event_list_current() = nullptr;
  return list == nullptr ? 0 : (int)((std::vector<hipEvent_t>*)list)->size();
}
int stove_event_list_destroy(void* list) {
  if (list == nullptr) return 0;
  std::lock_guard<std::mutex> g(event_list_mu());
  auto* v = (std::vector<hipEvent_t>*)list;
  if (event_list_current() == v) event_list_current() = nullptr;
  hipError_t e = hipSuccess;
  for (hipEvent_t ev : *v) {
    const hipError_t d = hipEventDestroy(ev);
    if (e == hipSuccess) e = d;
  }
  delete v;
  return (int)e;
}

// test / debugging utility: n 32-bit words at p <- value (tests poison a captured step's memory pool between replays)
int stove_fill_words(void* p, uint32_t value, size_t n_words, void* stream) {
  if (n_words == 0) return 0;
  const size_t blocks = (n_words + 256 * 8 - 1) / (256 * 8);
  STOVE_LAUNCH(fill_words_k, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)p, value, n_words);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_capture_begin(void* stream) { return (int)hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed); }

int stove_capture_end(void* stream, void** graph_out, int* n_nodes) {
  hipGraph_t g = nullptr;
  if (graph_out == nullptr) return (int)hipErrorInvalidValue;
  *graph_out = nullptr;
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &g);
  if (e != hipSuccess) return (int)e;
  size_t n = 0;
  e = hipGraphGetNodes(g, nullptr, &n);
  if (n_nodes != nullptr) *n_nodes = (int)n;
  *graph_out = (void*)g;
  return (int)e;
}

int stove_graph_instantiate(void* graph, void** exec_out) {
  if (exec_out == nullptr) return (int)hipErrorInvalidValue;
  *exec_out = nullptr;
  if (graph == nullptr) return 0;
  hipGraph_t g = (hipGraph_t)graph;
  size_t n = 0;
  hipError_t e = hipGraphGetNodes(g, nullptr, &n);
  if (e == hipSuccess && n > 0) {
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e == hipSuccess) *exec_out = (void*)x;
  }
  const hipError_t d = hipGraphDestroy(g);
  return (int)(e != hipSuccess ? e : d);
}

int stove_graph_launch(void* exec, void* stream) { return (int)hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)stream); }

int stove_graph_destroy(void* exec) { return exec == nullptr ? 0 : (int)hipGraphExecDestroy((hipGraphExec_t)exec); }

int stove_bw_transform(const float* x, float* out, int n_frames, int channels, int pixels, void* stream) {
  if (n_frames == 0) return 0;
  if (pixels % 4 != 0 || channels < 1) return (int)hipErrorInvalidValue;
  const long long total = (long long)n_frames * (pixels / 4);
  if (total > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(bw_transform_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, n_frames, channels, pixels / 4);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_bw_transform_u8(const unsigned char* x, float* out, int n_frames, int channels, int pixels, void* stream) {
  if (n_frames == 0) return 0;
  if (pixels % 4 != 0 || channels < 1) return (int)hipErrorInvalidValue;
  const long long total = (long long)n_frames * (pixels / 4);
  if (total > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(bw_transform_u8_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, n_frames, channels, pixels / 4);
  STOVE_LAUNCH_CHECK();
  return 0;
}

size_t stove_colsum_ws_floats(int rows, int cols) {
  const int chunks = rows < 512 ? (rows < 1 ? 1 : rows) : 512;
  return (size_t)(chunks + 16) * cols;
}

// one level: `rows` rows -> `used` partial rows (returned), each the sum of `per` consecutive rows
static int colsum_level(const float* a, float* part, int rows, int cols, int max_chunks, hipStream_t st) {
  const int chunks = rows < max_chunks ? rows : max_chunks;
  const int per = (rows + chunks - 1) / chunks;
  const int used = (rows + per - 1) / per;
  if (cols <= 64) {
    int cpad = 1;
    while (cpad < cols) cpad <<= 1;
    STOVE_LAUNCH(colsum_narrow_part_k, dim3(used), dim3(256), 0, st, a, part, rows, cols, cpad, per);
  } else {
    STOVE_LAUNCH(colsum_part_k, dim3(used, (cols / 4 + 255) / 256), dim3(256), 0, st, a, part, rows, cols / 4, per);
  }
  return used;
}

int stove_colsum(const float* a, float* out, float* ws, int rows, int cols, void* stream) { return stove_colsum2(a, out, nullptr, 0, ws, rows, cols, stream); }

int stove_colsum2(const float* a, float* out, float* out2, int accumulate, float* ws, int rows, int cols, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (cols <= 0 || (cols % 4 != 0 && cols > 64)) return (int)hipErrorInvalidValue;
  if (rows == 0) {
    if (!accumulate) {
      hipMemsetAsync(out, 0, sizeof(float) * cols, st);
      if (out2 != nullptr) hipMemsetAsync(out2, 0, sizeof(float) * cols, st);
    }
    return 0;
  }
  // 512 row chunks keep the first pass at HBM speed; a second pass folds them to <= 16 so that the final fixed-order
  // sum is short (a single 512-way pass over 1024 columns has only 32 workgroups and is latency-bound: 30 us)
  int used = colsum_level(a, ws, rows, cols, 512, st);
  STOVE_LAUNCH_CHECK();
  const float* src = ws;
  if (used > 16) {
    float* ws2 = ws + (size_t)(rows < 512 ? rows : 512) * cols;
    used = colsum_level(ws, ws2, used, cols, 16, st);
    STOVE_LAUNCH_CHECK();
    src = ws2;
  }
  STOVE_LAUNCH(reduce_chunks_k, dim3((cols + 31) / 32), dim3(256), 0, st, src, out, cols, used, accumulate, out2);      // both outputs in one launch
  STOVE_LAUNCH_CHECK();
  return 0;
}

static int small_tn_chunks(int rows) { return rows < 64 ? 1 : (rows / 64 < 512 ? rows / 64 : 512); }
size_t stove_small_tn_ws_floats(int rows, int M, int N) { return (size_t)small_tn_chunks(rows) * M * N; }

int stove_small_tn(const float* a, const float* b, float* out, float* ws, int rows, int M, int N, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M < 1 || N < 1 || M * N > 256) return (int)hipErrorInvalidValue;
  if (rows == 0) {
    hipMemsetAsync(out, 0, sizeof(float) * M * N, st);
    return 0;
  }
  const int chunks = small_tn_chunks(rows), per = (rows + chunks - 1) / chunks;
  STOVE_LAUNCH(small_tn_part_k, dim3(chunks), dim3(256), 0, st, a, b, ws, rows, M, N, per);
  STOVE_LAUNCH_CHECK();
  STOVE_LAUNCH(reduce_chunks_k, dim3((M * N + 31) / 32), dim3(256), 0, st, (const float*)ws, out, M * N, chunks, 0);
  STOVE_LAUNCH_CHECK();
  return 0;
}

size_t stove_flat_adam_ws_bytes(int nseg) { return (size_t)nseg * sizeof(int) + ADAM_SCAN_BLOCKS * sizeof(float); }

int stove_flat_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t numel,
                    const int* seg_of4, const unsigned char* seg_trainable, float* seg_steps, int nseg, void* ws, float* grad_norm_out,
                    const float* hyper_dev, float lr, float beta1, float beta2, float eps, float max_norm, int clip, void* stream) {
  if (numel == 0 || nseg == 0) return 0;
  if (numel % 4 != 0 || ws == nullptr || seg_of4 == nullptr || seg_trainable == nullptr || seg_steps == nullptr)
    return (int)hipErrorInvalidValue;
  AdamHyper k;
  k.lr = lr; k.b1 = beta1; k.b2 = beta2; k.eps = eps; k.max_norm = max_norm;
  const int n4 = (int)(numel / 4);
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  int* flags = reinterpret_cast<int*>(part + ADAM_SCAN_BLOCKS);          // cleared by the caller once, by adam_tick_k ever after
  STOVE_LAUNCH(grad_scan_k, dim3(ADAM_SCAN_BLOCKS), dim3(256), 0, st, grads, seg_of4, flags, part, n4);
  STOVE_LAUNCH(flat_adam_k, dim3((n4 + 255) / 256), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, seg_of4,
               seg_trainable, (const float*)seg_steps, (const int*)flags, (const float*)part, grad_norm_out, hyper_dev, k, clip & 1, n4);
  STOVE_LAUNCH(adam_tick_k, dim3((nseg + 255) / 256), dim3(256), 0, st, seg_trainable, seg_steps, flags, nseg, (clip >> 1) & 1);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- SuPAIR state pipeline / ELBO assembly
static ZpConst zp_const(const float* span_low) {
  ZpConst k;
  for (int d = 0; d < 8; ++d) {
    k.span[d] = span_low[d];
    k.low[d] = span_low[8 + d];
  }
  return k;
}

int stove_supair_state_fwd(const float* codes, const float* span_low, float* zc, float* pos, long long* idx, float* zfix,
                           unsigned char* hits, float* zl, float* sl, float* init6, int n, int T, int o, int skip, int fix,
                           int mode, void* stream) {
  return stove_supair_state_fwd2(codes, span_low, zc, pos, idx, zfix, hits, zl, sl, init6, 6, nullptr, 0, n, T, o, skip, fix, mode, stream);
}

int stove_supair_state_fwd2(const float* codes, const float* span_low, float* zc, float* pos, long long* idx, float* zfix,
                            unsigned char* hits, float* zl, float* sl, float* init, int init_ld, const float* lat_noise, int lat_dim,
                            int n, int T, int o, int skip, int fix, int mode, void* stream) {
  if (init_ld < 6 + (lat_noise != nullptr ? lat_dim : 0) || lat_dim < 0) return (int)hipErrorInvalidValue;
  float* init6 = init;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return 0;
  if (T < 2 || skip < 1 || skip >= T || o < 1 || o > kMatchN) return (int)hipErrorInvalidValue;
  const int M = n * T * o;
  if (codes != nullptr) {        // codes == NULL: zc (constrained states) and idx (a matching) are the caller's; only the last stage runs
    STOVE_LAUNCH(zp_constrain_k, dim3((M * 8 + 255) / 256), dim3(256), 0, st, codes, zp_const(span_low), zc, pos, M);
    STOVE_LAUNCH_CHECK();
    int rc = stove_match_objects(pos, idx, nullptr, n, T, o, 2, mode, stream);
    if (rc) return rc;
  }
  STOVE_LAUNCH(supair_state_fwd_k, dim3((M + 255) / 256), dim3(256), 0, st, (const float*)zc, (const long long*)idx, zfix, hits, zl, sl,
               init6, n, T, o, skip, fix, init_ld, lat_noise, lat_dim);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_supair_state_bwd(const float* zc, const long long* idx, const unsigned char* hits, const float* zfix, const float* g_zfix,
                           const float* g_zl, const float* g_sl, const float* g_init6, const float* span_low, float* gfix_ws,
                           float* g_codes, int n, int T, int o, int skip, void* stream) {
  return stove_supair_state_bwd2(zc, idx, hits, zfix, g_zfix, g_zl, g_sl, g_init6, 6, span_low, gfix_ws, g_codes, n, T, o, skip, stream);
}

int stove_supair_state_bwd2(const float* zc, const long long* idx, const unsigned char* hits, const float* zfix, const float* g_zfix,
                            const float* g_zl, const float* g_sl, const float* g_init6, int init_ld, const float* span_low, float* gfix_ws,
                            float* g_codes, int n, int T, int o, int skip, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return 0;
  const int M = n * T * o;
  (void)gfix_ws;      // (until round 5 the intermediate of a two-launch form; the argument stays for the ABI)
  STOVE_LAUNCH(supair_state_bwd_k, dim3((M + 255) / 256), dim3(256), 0, st, zc, idx, hits, zfix, g_zfix, g_zl, g_sl, g_init6, zp_const(span_low),
               g_codes, n, T, o, skip, init_ld);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_noise_normal(float* out, size_t n, unsigned long long* state, void* stream) {
  if (n == 0) return 0;
  if (((uintptr_t)out & 15) != 0 || state == nullptr) return (int)hipErrorInvalidValue;
  const size_t threads = (n + 3) / 4;
  if ((threads + 255) / 256 > 0x7fffffffULL) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(noise_normal_k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n, (const unsigned long long*)state);
  STOVE_LAUNCH(noise_tick_k, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_zall_fwd(const float* zfix, const float* zs, float* zall, int n, int T, int o, int skip, void* stream) {
  if (n == 0) return 0;
  const int M = n * (T - 1) * o;
  STOVE_LAUNCH(zall_fwd_k, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, zfix, zs, zall, n, T, o, skip);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_zall_bwd(const float* zfix, const float* zs, const float* g_zall, const float* dz_in, float* g_zfix, float* g_zs, int n, int T, int o,
                   int skip, void* stream) {
  if (n == 0) return 0;
  const int M = n * T * o + n * (T - skip) * o;
  STOVE_LAUNCH(zall_bwd_k, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, zfix, zs, g_zall, dz_in, g_zfix, g_zs, n, T, o, skip);
  STOVE_LAUNCH_CHECK();
  return 0;
}

static TransStd trans_std(const float* s16) {
  TransStd t;
  for (int d = 0; d < 16; ++d) t.s[d] = s16[d];
  return t;
}

int stove_elbo_fwd(const float* zs, const float* mean, const float* std_, const float* zdyn, const float* lik, const float* trans_std16,
                   float* part_ws, float* out3, int n, int T, int o, int skip, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || skip < 1 || skip >= T) return (int)hipErrorInvalidValue;
  STOVE_LAUNCH(elbo_part_k, dim3(n), dim3(256), 0, st, zs, mean, std_, zdyn, lik, trans_std(trans_std16), part_ws, T, o, skip);
  STOVE_LAUNCH_CHECK();
  STOVE_LAUNCH(elbo_final_k, dim3(1), dim3(256), 0, st, (const float*)part_ws, out3, n, T, skip);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_elbo_bwd(const float* zs, const float* mean, const float* std_, const float* zdyn, const float* trans_std16, const float* g_out,
                   float* g_zs, float* g_mean, float* g_std, float* g_zdyn, float* g_lik, int n, int T, int o, int skip, void* stream) {
  if (n == 0) return 0;
  const size_t M = (size_t)n * (T - skip) * o * 18 + (size_t)n * (T - 1);
  STOVE_LAUNCH(elbo_bwd_k, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, zs, mean, std_, zdyn, trans_std(trans_std16), g_out,
               g_zs, g_mean, g_std, g_zdyn, g_lik, n, T, o, skip);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- LSTM cell (recognition network)
// ---------------------------------------------------------------- recognition-network head
// ---- fused output head (csrc/head_fused.hip): H = 256, HID <= 64, OUT = 8 ------------------------------------------------------
static int enc_head_groups(int rows) {
  const int tiles = (rows + 15) / 16;
  int g = (tiles + 3) / 4;
  return g < 1 ? 1 : (g > 102 ? 102 : g);       // 102 groups x 5 roles = 510 workgroups: all resident at 2 per CU (a second round of
                                                // workgroups would start when the first ends and double the kernel's time)
}

int stove_enc_head_fwd(const float* h, const float* W1, const float* b1, const float* W2, const float* b2, float* h1, float* codes, int rows,
                       int H, int HID, int OUT, int frames, int fc1_split, void* stream) {
  if (H != kEhH || HID < 1 || HID > kEhHid || OUT != kEhOut || frames < 0 || (frames > 0 && rows % frames != 0)) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  static_assert(2 * kEhHid * kEhLdB == sizeof(float) * kEhHid * kEhLd, "the two bf16 images of W1 take the fp32 image's place");
  const size_t lds = sizeof(float) * kEhHid * kEhLd;
  const int tiles = (rows + 15) / 16;
  const int grid = (tiles + 3) / 4 < 512 ? (tiles + 3) / 4 : 512;
  int rc;
  if (fc1_split) {       // fc1 as three half-piece MFMAs per product (the default); else on v_mfma_f32_16x16x4_f32 (encoder_gemm = 'fp32')
    rc = (int)hipFuncSetAttribute((const void*)enc_head_fwd_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc) return rc;
    STOVE_LAUNCH((enc_head_fwd_k<true>), dim3(grid), dim3(256), lds, (hipStream_t)stream, h, W1, b1, W2, b2, h1, codes, rows, HID, frames);
  } else {
    rc = (int)hipFuncSetAttribute((const void*)enc_head_fwd_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc) return rc;
    STOVE_LAUNCH((enc_head_fwd_k<false>), dim3(grid), dim3(256), lds, (hipStream_t)stream, h, W1, b1, W2, b2, h1, codes, rows, HID, frames);
  }
  STOVE_LAUNCH_CHECK();
  return 0;
}

size_t stove_enc_head_bwd_ws_floats(int rows, int HID) { return (size_t)enc_head_groups(rows) * eh_part_floats(HID); }

int stove_enc_head_bwd(const float* dcodes, const float* h1, const float* h, const float* W1, const float* W2, float* gh, float* gW1,
                       float* gb1, float* gW2, float* gb2, int accumulate, float* ws, int rows, int H, int HID, int OUT, int frames, void* stream) {
  if (H != kEhH || HID < 1 || HID > kEhHid || OUT != kEhOut || frames < 0 || (frames > 0 && rows % frames != 0)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int P = eh_part_floats(HID);
  if (rows == 0) {
    if (!accumulate) {
      hipMemsetAsync(gW1, 0, sizeof(float) * HID * kEhH, st);
      hipMemsetAsync(gW2, 0, sizeof(float) * kEhOut * HID, st);
      hipMemsetAsync(gb1, 0, sizeof(float) * HID, st);
      hipMemsetAsync(gb2, 0, sizeof(float) * kEhOut, st);
    }
    return 0;
  }
  const int groups = enc_head_groups(rows);
  const size_t lds = sizeof(float) * kEhBwdLds;
  int rc;
  if (HID <= 50) {
    rc = (int)hipFuncSetAttribute((const void*)enc_head_bwd_k<14>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc) return rc;
    STOVE_LAUNCH(enc_head_bwd_k<14>, dim3(groups * 5), dim3(256), lds, st, dcodes, h1, h, W1, W2, gh, ws, rows, HID, groups, frames);
  } else {
    rc = (int)hipFuncSetAttribute((const void*)enc_head_bwd_k<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc) return rc;
    STOVE_LAUNCH(enc_head_bwd_k<16>, dim3(groups * 5), dim3(256), lds, st, dcodes, h1, h, W1, W2, gh, ws, rows, HID, groups, frames);
  }
  STOVE_LAUNCH_CHECK();
  (void)P;
  STOVE_LAUNCH(enc_head_reduce_k, dim3((eh_part_floats(HID) + 31) / 32), dim3(256), 0, st, (const float*)ws, gW1, gW2, gb1, gb2, HID, groups, accumulate);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_lstm_cell_fwd(const float* gx, const float* gh, const float* c_prev, float* c, float* h, int n, int H, int fast, void* stream) {
  if (n == 0) return 0;
  if (H % 4) return (int)hipErrorInvalidValue;
  const size_t total = (size_t)n * (H / 4);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (fast) STOVE_LAUNCH(lstm_cell_fwd_k<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, gx, gh, c_prev, c, h, n, H);
  else STOVE_LAUNCH(lstm_cell_fwd_k<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, gx, gh, c_prev, c, h, n, H);
  STOVE_LAUNCH_CHECK();
  return 0;
}

int stove_lstm_cell_bwd(const float* gx, const float* gh, const float* c_prev, const float* c, const float* dh,
                        const float* dc_in, float* dg, float* dc_out, float* dgx_sum, const float* dg_more, int n_more, int n, int H,
                        int fast, void* stream) {
  if (n == 0) return 0;
  if (H % 4 || n_more < 0 || (n_more > 0 && dg_more == nullptr)) return (int)hipErrorInvalidValue;
  const size_t more_stride = (size_t)n * 4 * H;
  const size_t total = (size_t)n * (H / 4);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (fast) STOVE_LAUNCH(lstm_cell_bwd_k<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, gx, gh, c_prev, c, dh, dc_in, dg, dc_out, dgx_sum, dg_more,
                         n_more, more_stride, n, H);
  else STOVE_LAUNCH(lstm_cell_bwd_k<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, gx, gh, c_prev, c, dh, dc_in, dg, dc_out, dgx_sum, dg_more,
                    n_more, more_stride, n, H);
  STOVE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- profiling hooks
void stove_profile_enable(int on) {
  std::lock_guard<std::mutex> g(prof_mu());
  prof_on() = on != 0;
}

// Synchronises every recorded event pair, aggregates by kernel name and writes lines
// "name\ttotal_ms\tcount\twall_ms\n" (wall_ms: the union of the launches' time spans) into buf (at most cap bytes); returns the
// number of bytes needed.
size_t stove_profile_report(char* buf, size_t cap) {
  std::lock_guard<std::mutex> g(prof_mu());
  struct Agg {
    std::string name;
    double total = 0.0;
    long count = 0;
    std::vector<std::pair<double, double>> spans;      // [start, end) in ms since the first recorded launch
  };
  std::vector<Agg> agg;
  auto& recs = prof_recs();
  for (auto& r : recs) (void)hipEventSynchronize(r.b);
  for (auto& r : recs) {
    float ms = 0.0f, t0 = 0.0f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    (void)hipEventElapsedTime(&t0, recs.front().a, r.a);
    Agg* e = nullptr;
    for (auto& x : agg)
      if (x.name == r.name) {
        e = &x;
        break;
      }
    if (e == nullptr) {
      agg.push_back(Agg());
      e = &agg.back();
      e->name = r.name;
    }
    e->total += ms;
    e->count += 1;
    e->spans.push_back({(double)t0, (double)t0 + ms});
  }
  for (auto& r : recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  recs.clear();
  std::string out;
  for (auto& e : agg) {
    // launches of one kernel on two streams overlap in time (the recognition network's row chunks): the time they COVER
    std::sort(e.spans.begin(), e.spans.end());
    double wall = 0.0, lo = 0.0, hi = -1.0;
    for (auto& sp : e.spans) {
      if (hi < lo || sp.first > hi) {
        if (hi >= lo) wall += hi - lo;
        lo = sp.first;
        hi = sp.second;
      } else if (sp.second > hi) {
        hi = sp.second;
      }
    }
    if (hi >= lo) wall += hi - lo;
    out += e.name + "\t" + std::to_string(e.total) + "\t" + std::to_string(e.count) + "\t" + std::to_string(wall) + "\n";
  }
  if (buf != nullptr && cap > 0) {
    const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return out.size() + 1;
}

// ---------------------------------------------------------------- temporal object matching
int stove_match_objects(const float* feat, long long* idx, float* perm, int B, int T, int N, int F, int mode, void* stream) {
  if (B == 0 || T == 0) return 0;
  if (N < 1 || N > kMatchN || F < 1 || F > kMatchF || mode < 0 || mode > 3) return (int)hipErrorInvalidValue;
  const bool serial = mode == 3;       // '3_only' through the frame-by-frame walk (the check of match3_table_k in the tests)
  if (serial) mode = 0;
  const size_t lds = (size_t)T * N * (F + 1) * sizeof(float);
  if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  // the lane-parallel kernel wins where the serial walk of lane 0 has real work per frame (the greedy matcher, more than
  // three objects: 580 -> 170 us for six); for three objects and the nearest-slot rules the serial walk is shorter
  if (!serial && mode == 0 && N == 3 && F == 2)
    STOVE_LAUNCH((match3_table_k<2>), dim3(B), dim3(64), lds, st, feat, idx, B, T);
  else if (!serial && mode == 0 && N == 3 && F == 5)
    STOVE_LAUNCH((match3_table_k<5>), dim3(B), dim3(64), lds, st, feat, idx, B, T);
  else if (mode == 1 && perm == nullptr && (size_t)T * N * 5 + T + 8 <= 64 * 1024) {
    // greedy: per-frame assignments in parallel, then the composition walk (match.hip); scratch = the tail bytes of idx itself
    STOVE_LAUNCH(match_greedy_frames_k, dim3((B * T + 255) / 256), dim3(256), 0, st, feat, idx, B, T, N, F);
    STOVE_LAUNCH(match_greedy_compose_k, dim3(B), dim3(64), (size_t)((T * N + T + 3) & ~3) + (size_t)T * N * sizeof(int), st, feat, idx, B, T, N, F);
  } else if (mode == 1 || N > 3)
    STOVE_LAUNCH(match_objects_par_k, dim3(B), dim3(64), lds, st, feat, idx, B, T, N, F, mode);
  else if (N == 3 && F == 2)
    STOVE_LAUNCH((match_objects_k<3, 2>), dim3(B), dim3(64), lds, st, feat, idx, perm, B, T, N, F, mode);
  else if (N == 3 && F == 5)
    STOVE_LAUNCH((match_objects_k<3, 5>), dim3(B), dim3(64), lds, st, feat, idx, perm, B, T, N, F, mode);
  else
    STOVE_LAUNCH((match_objects_k<0, 0>), dim3(B), dim3(64), lds, st, feat, idx, perm, B, T, N, F, mode);
  STOVE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
