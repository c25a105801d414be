/* libstove_hip.so -- C ABI of the MI355X (gfx950) STOVE hot path.
 *
 * The reference (jlko/STOVE) has no FFI: the path sits behind Python modules whose work is a
 * stream of ATen ops.  Each entry point below replaces one such op chain; the comment names
 * the reference lines (relative to the reference repo root) it stands in for.  The Python
 * modules in stove_amd/ (same names/signatures as the reference's) bind these with ctypes.
 *
 * Conventions:
 *   - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch allocates), float32 unless noted; `stream` is a hipStream_t passed as void*.
 *   - functions only enqueue work on `stream`: no allocation, no free, no synchronisation;
 *     re-entrant and thread-safe; safe under hipGraph capture.  The library reads nothing from
 *     the environment; its only process state is listed in one place ("process state" below):
 *     the per-device fork stream, two measurement switches, the open event list, the profiler.
 *   - workspaces are sized by the matching *_ws_bytes() query and need no initialisation.
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch
 *     (stove_error_string() names it).
 *   - all gradients are OVERWRITTEN, never accumulated.
 */
#ifndef STOVE_HIP_H
#define STOVE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int stove_abi_version(void);
const char* stove_error_string(int code);

/* Baked parameter tables of the two random SPNs (built by stove_amd/spn/rat_spn.py from the
 * reference-layout parameters: vector_list.L.i.{means,sigma_params,params}).
 * Object SPN (probabilistic_models.py:8-22; R=6 replicas, 4 leaves x S=25 pixels, G=K=10):
 *   obj_scope     int32 [R*4][S]        pixel index of leaf row i          (region_graph.py:54-95)
 *   obj_leaf_slot int32 [R][100]        L*S+i of pixel p inside replica r
 *   obj_coef      f32   [R*4][S][G][3]  (a,b,c): leaf log-density = sum_p w_p (a x^2 + b x + c)   (rat_torch.py:83-109)
 *   obj_wsum      f32   [R*2][G*G][K]   softmax(params, 0) of the 12 inner sum nodes            (rat_torch.py:202-222)
 *   obj_wroot     f32   [R][K*K]        softmax over all R*K*K root weights
 * Background SPN (probabilistic_models.py:25-39; R=3, two 512-pixel leaves, G=6):
 *   bg_side       int32 [R][1024]       0/1: which leaf of replica r owns pixel p
 *   bg_coef       f32   [R][1024][G][3]
 *   bg_wroot      f32   [R][G*G]        softmax over all R*G*G root weights, row j2*G+j1
 */
typedef struct StoveSpnTables {
  const int32_t* obj_scope;
  const int32_t* obj_leaf_slot;
  const float* obj_coef;
  const float* obj_wsum;
  const float* obj_wroot;
  const int32_t* bg_side;
  const float* bg_coef;
  const float* bg_wroot;
  const float* bg_dense;   /* optional: bg_coef as the operand image of the scene forward's leaf GEMM (stove_bg_dense), made
                            * ahead of time by the caller; NULL = stove_scene_fwd builds it itself at the head of its chain */
} StoveSpnTables;

/* bg_coef / bg_side -> the dense (3072 x 48, fragment-ordered) coefficient image StoveSpnTables.bg_dense points at;
 * it depends on the parameters only.  dense: stove_bg_dense_floats() floats. */
size_t stove_bg_dense_floats(void);
int stove_bg_dense(const int32_t* bg_side, const float* bg_coef, float* dense, void* stream);

/* Gradients w.r.t. the baked tables (same shapes as above). */
typedef struct StoveSpnTableGrads {
  float* obj_coef;
  float* obj_wsum;
  float* obj_wroot;
  float* bg_coef;
  float* bg_wroot;
} StoveSpnTableGrads;

/* ---- RatSpn.forward(inputs, marginalized) for the object SPN (rat_torch.py:354-357 as called
 * at supair.py:76).  inputs/marg: (n,100) row-major, marg may be NULL.  out: (n,).
 * `xw` is the saved activation for the backward: ceil(n/64)*100*2*64 floats. */
size_t stove_objspn_tile_floats(int n);
int stove_objspn_fwd(const StoveSpnTables* t, const float* inputs, const float* marg, float* xw, float* out,
                     int n, void* stream);
size_t stove_objspn_bwd_ws_bytes(int n);
/* d_inputs/d_marg (n,100) may be NULL. */
int stove_objspn_bwd(const StoveSpnTables* t, const float* marg, const float* xw, const float* out, const float* dout,
                     float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n, void* stream);

/* ---- RatSpn.forward for the background SPN (supair.py:67).  inputs/marg: (n,1024).
 * `ell` is the saved activation: stove_bgspn_saved_floats(n) floats. */
size_t stove_bgspn_saved_floats(int n);
int stove_bgspn_fwd(const StoveSpnTables* t, const float* inputs, const float* marg, float* ell, float* out,
                    int n, void* stream);
size_t stove_bgspn_bwd_ws_bytes(int n);
int stove_bgspn_bwd(const StoveSpnTables* t, const float* inputs, const float* marg, const float* ell, const float* out,
                    const float* dout, float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n,
                    void* stream);

/* The same operator over n_pix input dimensions (the reference builds the background SPN over c x w x h, probabilistic_models.py:25-39;
 * its stock gravity / multibilliards frames are 50 x 50): tables bg_side [R][n_pix], bg_coef [R][n_pix][G][3], bg_wroot [R][G*G];
 * inputs / marg / d_inputs / d_marg (n, n_pix).  General-size kernels (csrc/spn_bg_generic.hip), not the tuned 1024-pixel ones. */
size_t stove_bgspn_saved_floats_d(int n, int n_pix);
int stove_bgspn_fwd_d(const StoveSpnTables* t, const float* inputs, const float* marg, float* ell, float* out, int n, int n_pix, void* stream);
size_t stove_bgspn_bwd_ws_bytes_d(int n, int n_pix);
int stove_bgspn_bwd_d(const StoveSpnTables* t, const float* inputs, const float* marg, const float* ell, const float* out, const float* dout,
                      float* d_inputs, float* d_marg, StoveSpnTableGrads* g, void* ws, int n, int n_pix, void* stream);

/* ---- Supair.likelihood (supair.py:44-110), fused: masks_from_z (:278-356), patches_from_z
 * (:241-276), both SPN sweeps, patch scaling + Exponential(beta) overlap prior (:79-94).
 * frames: (n_frames,1024) one-channel frames; z: (n_frames*n_obj,4) = [sx,sy,x,y].
 * seq_frames / seq_stride: the frames may be a time-slice of longer clips handed over WITHOUT a copy (Stove.forward scores
 * x[:, 1:], stove.py:731-736): frame f is row (f / seq_frames) * seq_stride + f % seq_frames behind `frames`; 0, 0 = dense.
 * ll: (n_frames,) log p(x,z); parts: (n_frames,3) = bg, patches, overlap (may be NULL).
 * saved: stove_scene_saved_floats() floats kept for the backward.  The object SPN's backward is linear in the upstream
 * gradient of a glimpse, so the forward runs it at once, at a gradient of 1, while the sample's leaf and sum-node values are
 * still in registers, and leaves the per-glimpse scratch (2 904 B) in `saved`; stove_scene_bwd* applies dL/d(glimpse
 * likelihood) where that scratch is consumed.  A caller that will never differentiate uses stove_scene_fwd_from(.., with_grad 0)
 * with the smaller buffer of stove_scene_fwd_floats(.., 0): same ll / parts bit for bit, no backward from it. */
size_t stove_scene_saved_floats(int n_frames, int n_obj);
size_t stove_scene_fwd_floats(int n_frames, int n_obj, int with_grad);     /* with_grad != 0: == stove_scene_saved_floats */
int stove_scene_fwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                    int seq_stride, float overlap_beta, float* ll, float* parts, float* saved, void* stream);
size_t stove_scene_bwd_ws_bytes(int n_frames, int n_obj);
/* dll: (n_frames,) -> dz: (n_frames*n_obj,4) and table gradients. */
int stove_scene_bwd(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                    int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz, StoveSpnTableGrads* g,
                    void* ws, void* stream);
/* The same with the parameter-gradient passes (leaf / sum / root table gradients: they only feed the optimiser) on a
 * second stream, so that they overlap with what the caller enqueues on `stream` next -- in STOVE the latency-bound
 * backward of the recursion, which leaves most of every CU idle.  dz is complete in `stream` order when the call
 * returns; *g is complete in `param_stream` order.  param_stream NULL or == stream: identical to stove_scene_bwd. */
int stove_scene_bwd_overlap(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                    int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz, StoveSpnTableGrads* g,
                    void* ws, void* stream, void* param_stream);
/* ---- RatSpn.forward / backward of the OBJECT SPN for any glimpse size and vector widths (reference probabilistic_models.py:8-22
 * with config.patch_width / patch_height / obj_spn_num_gauss / obj_spn_num_sums other than 10 / 10 / 10 / 10, config.py:99-100,
 * 119-120; the entry points above are the tuned kernels of the default shape).  R replicas (children of the root sum), each the
 * product of two sum vectors of S nodes over the G x G product of two Gaussian leaves; D dimensions, leaves of up to Lmax pixels.
 *   lscope (R*4, Lmax) int32: pixels of leaf (r, 2 j + side), padded with -1;   slot (R, D) int32: l * Lmax + i of pixel p in replica r
 *   coef (R*4, Lmax, G, 3) = (a, b, c) per pixel and component;  wsum (R*2, G*G, S) softmaxed over G*G;  wroot (R, S*S) softmaxed
 * marg NULL = nothing marginalised.  saved: stove_objspn_saved_floats_any floats; ws: stove_objspn_bwd_ws_bytes_any bytes.
 * d_inputs / d_marg may be NULL; g_* are overwritten.  Limits: R <= 8, G, S <= 16, D <= 1024. */
size_t stove_objspn_saved_floats_any(int n, int R, int G, int S, int D, int Lmax);
size_t stove_objspn_bwd_ws_bytes_any(int n, int R, int G, int S, int D, int Lmax);
int stove_objspn_fwd_any(const float* inputs, const float* marg, const int* lscope, const float* coef, const float* wsum,
                         const float* wroot, float* saved, float* out, int n, int R, int G, int S, int D, int Lmax, void* stream);
int stove_objspn_bwd_any(const float* inputs, const float* marg, const int* lscope, const int* slot, const float* coef,
                         const float* wsum, const float* wroot, const float* saved, const float* dout, float* d_inputs,
                         float* d_marg, float* g_coef, float* g_wsum, float* g_wroot, void* ws, int n, int R, int G, int S, int D,
                         int Lmax, void* stream);
/* ---- the reference's fixed-Gaussian debug models (SimpleBG / SimpleObj, probabilistic_models.py:42-90; config.debug_bg_model /
 * debug_obj_spn): out[r] = sum_p (1 - marg[r][p]) log Normal(mean, scale)(x[r][p]), marg unclamped as there; dx / dm may be NULL. */
int stove_gauss_ll_fwd(const float* x, const float* marg, float* out, int n, int d, float mean, float scale, void* stream);
int stove_gauss_ll_bwd(const float* x, const float* marg, const float* dout, float* dx, float* dm, int n, int d, float mean, float scale,
                       void* stream);
/* The same likelihood for any frame size and either sampling convention of the spatial transformer (reference supair.py:44-110 with
 * config width/height != 32 -- the reference's stock gravity / multibilliards data are 50 x 50, envs.py:771-773 -- or the
 * torch-1.0.1 convention align_corners=True its published runs used).  frames: rows of W*H floats (W = the size of the last
 * tensor dimension, the x direction of grid_sample); 10 x 10 glimpses and single-channel frames as above.  The object side runs the
 * 32 x 32 path's kernels with the geometry at run time; the background side the general-size SPN operator (stove_bgspn_fwd_d) on
 * the closed-form mask.  t->bg_coef is [3][W*H][6][3], t->bg_side (W*H) int32, t->bg_dense unused.  saved / ws sizes below;
 * *g complete in `param_stream` order (NULL = `stream`), dz in `stream` order. */
size_t stove_scene_saved_floats_any(int n_frames, int n_obj, int n_pix, int with_grad);
size_t stove_scene_bwd_ws_bytes_any(int n_frames, int n_obj, int n_pix);
int stove_scene_fwd_any(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                        int seq_stride, int W, int H, int align_corners, float overlap_beta, float* ll, float* parts, float* saved,
                        void* stream, int with_grad);
int stove_scene_bwd_any(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                        int seq_stride, int W, int H, int align_corners, float overlap_beta, const float* saved, const float* dll,
                        float* dz, StoveSpnTableGrads* g, void* ws, void* stream, void* param_stream);
/* The same likelihood over `channels` colour planes (1..4; reference supair.py:44-110 with config.channels = 3, debug_bw = False).
 * frames: rows of channels*W*H floats in (c, W-major plane) order; glimpses of pw x ph pixels (patch_width x patch_height) in either
 * sampling convention.  The object SPN is the general-size one of stove_objspn_fwd_any over D = channels*pw*ph dimensions (its tables
 * and limits, R, G, S, D, Lmax); the background tables are bg_side [3][channels*W*H], bg_coef [3][channels*W*H][6][3] (bg_coef_floats
 * floats), bg_wroot [3][36].  The occlusion mask is the same in every channel.  saved / ws sizes below; dz in `stream` order, the table
 * gradients (overwritten) complete in `param_stream` order (NULL = `stream`).  hipErrorInvalidValue for channels outside 1..4,
 * D != channels*pw*ph, bg_coef_floats != 3*channels*W*H*6*3, n_obj outside 1..8, object-SPN shapes past the limits above, null
 * pointers.  with_grad: accepted for symmetry with stove_scene_fwd_any (the saved activations are the same). */
size_t stove_scene_saved_floats_ch(int n_frames, int n_obj, int channels, int W, int H, int R, int G, int S, int D, int Lmax, int with_grad);
size_t stove_scene_bwd_ws_bytes_ch(int n_frames, int n_obj, int channels, int W, int H, int R, int G, int S, int D, int Lmax);
int stove_scene_fwd_ch(const int32_t* lscope, const int32_t* slot, const float* coef, const float* wsum, const float* wroot, int R, int G, int S,
                       int D, int Lmax, const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats,
                       const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H,
                       int pw, int ph, int align_corners, float overlap_beta, float* ll, float* parts, float* saved, void* stream, int with_grad);
int stove_scene_bwd_ch(const int32_t* lscope, const int32_t* slot, const float* coef, const float* wsum, const float* wroot, int R, int G, int S,
                       int D, int Lmax, const int32_t* bg_side, const float* bg_coef, const float* bg_wroot, size_t bg_coef_floats,
                       const float* frames, const float* z, int n_frames, int n_obj, int seq_frames, int seq_stride, int channels, int W, int H,
                       int pw, int ph, int align_corners, float overlap_beta, const float* saved, const float* dll, float* dz, float* g_coef,
                       float* g_wsum, float* g_wroot, float* g_bg_coef, float* g_bg_wroot, void* ws, void* stream, void* param_stream);
/* The same with the stream the internal background-SPN chain forks from given explicitly (NULL = `stream`).  For callers that run the
 * scene calls on a stream which is itself a fork inside a hipGraph capture: pass the capture's origin stream, where frames, z, saved
 * and dll must then be ready (the HIP 7.0 runtime cannot end a capture in which two forked streams wait on each other). */
int stove_scene_fwd_from(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                         int seq_stride, float overlap_beta, float* ll, float* parts, float* saved, void* stream, void* fork_from,
                         int with_grad);
int stove_scene_bwd_from(const StoveSpnTables* t, const float* frames, const float* z, int n_frames, int n_obj, int seq_frames,
                         int seq_stride, float overlap_beta, const float* saved, const float* dll, float* dz,
                         StoveSpnTableGrads* g, void* ws, void* stream, void* param_stream, void* fork_from);

/* Stove.object_embedding (stove.py:565-590): emb (n_frames*n_obj, channels) = mean over the 10x10 glimpse of object k of
 * colour frame x_color (n_frames, channels, 32, 32); z (n_frames*n_obj, 4) = [sx, sy, x, y].  No gradients. */
int stove_glimpse_mean(const float* x_color, const float* z, float* emb, int n_frames, int n_obj, int channels, void* stream);

/* ---- MPE reconstruction of glimpses by the object SPN (Supair.spn_mpe, supair.py:382-424, with RatSpn.reconstruct,
 * rat_torch.py:359-372): inputs (n,100) glimpses, no marginalisation.  Every sum node keeps its best child
 * (argmax_k child_k + log w_k, first on ties); the walk from the root selects one replica and one Gaussian per leaf;
 * out (n,100) = those components' means on their scopes, clamped to [0,1].  leaf_means: f32 [R*4][25][10], leaf order of
 * obj_scope.  pick (n,5) int32 = (replica, component of each of its 4 leaves), may be NULL.  `xw`: scratch of
 * stove_objspn_tile_floats(n) floats.  No gradients. */
int stove_objspn_mpe(const StoveSpnTables* t, const float* leaf_means, const float* inputs, float* xw, float* out,
                     int32_t* pick, int n, void* stream);

/* ---- frame rendering (Supair.reconstruct_from_z, supair.py:484-498): out (n_frames,1024) =
 * clamp(bg + sum_k grid_sample(patch_k, inverse transform of z_k), 0, 1).  bg (1024,), z (n_frames*n_obj,4) = [sx,sy,x,y],
 * patches (.,100): row (f / frames_per_patch) * n_obj + k; frames_per_patch == 0: the single row 0 for every object. */
int stove_render_frames(const float* bg, const float* patches, int frames_per_patch, const float* z, float* out, int n_frames,
                        int n_obj, void* stream);

/* ---- frame rendering at run-time sizes, with the squared pixel error fused in (csrc/render.hip): the composed paste of
 * Supair.reconstruct_from_z per channel, out (n_frames, C*W*H) = clamp(bg + sum_k grid_sample(patch_k, inverse transform of z_k), 0, 1),
 * bilinear, zero padding, either align_corners convention.  A frame plane is W rows of H columns, a patch plane pw rows of ph columns
 * (the width / height order of that code); the transform's x runs along the columns.  bg (C*W*H,), patches (., C*pw*ph) flattened
 * (channel, row, column) and indexed as in stove_render_frames, z (n_frames*n_obj, 4) = [sx, sy, x, y].
 * truth (n_frames, C*W*H) and sqerr (n_frames,) come together or not at all: sqerr[f] = sum over the frame's C*W*H pixels of
 * (clamped frame - truth)^2, summed in a fixed order without atomics (bit-identical between calls, and with or without `out`).
 * out may be NULL (no frame is written then), but not together with sqerr.  n_frames == 0 launches nothing.
 * With sqerr a frame is one workgroup whatever its size (that is what keeps the sum in one fixed order): meant for many small
 * frames; a few very large ones are rendered faster without truth (tiled) and summed by the caller.
 * hipErrorInvalidValue, nothing launched: a NULL bg / patches / z, truth without sqerr or the reverse, neither out nor sqerr,
 * n_obj outside 1..8, C outside 1..4, a size < 1, frames_per_patch < 0, n_frames < 0.  No gradients. */
int stove_render_frames_any(const float* bg, const float* patches, int frames_per_patch, const float* z, const float* truth, float* out,
                            float* sqerr, int n_frames, int n_obj, int C, int W, int H, int pw, int ph, int align_corners, void* stream);

/* ---- glimpses + masks alone (supair.py:241-356), for the Supair.patches_from_z /
 * masks_from_z API: patches, marg_patch: (n_frames*n_obj,100); overlap: (n_frames*n_obj,).
 * `tile` is scratch of stove_objspn_tile_floats(n_frames*n_obj) floats. */
int stove_scene_glimpses(const float* frames, const float* z, int n_frames, int n_obj, float* tile,
                         float* patches, float* keep, void* stream);

/* ---- Dynamics.forward / core (dynamics.py:181-265): one GNN step.
 * params: the parameter image of stove_gnn_param_floats() floats built by
 * stove_amd/video_prediction/dynamics.py + ops._gnn_image (W | W^T | vectors | W packed | W^T packed: the last two hold every layer
 * once more in the [K/4][OUT][4] order the small-graph recursion kernels copy into LDS; layout in csrc/gnn.hip).
 * s_in (B,N,sin_dim): [state 16 | action embedding 4 | appearance 3] as configured (16 <= sin_dim <= 32);
 * result (B,N,32) = means|stds (dynamics.py:216), pred (B,N,32) = dynamic_pred (:208), may be NULL.
 * elu: 0 = leaky_relu(0.01) (the reference default, dynamics.py:109), 1 = elu. */
size_t stove_gnn_param_floats(void);
size_t stove_gnn_grad_floats(void);
int stove_gnn_blocks(int B, int N);
int stove_gnn_fwd(const float* s_in, const float* params, float* result, float* pred, int B, int N, int sin_dim,
                  int lim_enc, int elu, void* stream);
size_t stove_gnn_bwd_ws_bytes(int B, int N);
/* g_params: gradient image of stove_gnn_grad_floats() floats (W layout + vectors). d_pred may be NULL. */
int stove_gnn_bwd(const float* s_in, const float* params, const float* d_result, const float* d_pred, float* d_s_in,
                  float* g_params, void* ws, int B, int N, int sin_dim, int lim_enc, int elu, void* stream);

/* debug/measurement: one forward+backward GNN step that also writes the cycle counter at every stage
 * boundary of workgroup 0 into stamps[0..63] (int64, device). */
int stove_gnn_debug_stamps(const float* s_in, const float* params, const float* d_result, float* d_s_in, void* ws,
                           long long* stamps, int B, int N, int sin_dim, int lim_enc, int elu, void* stream);

/* ---- the inference recursion of Stove.stove_forward (stove.py:696-713) with Dynamics.constrain_z_dyn
 * (dynamics.py:147-179) and Stove.full_state (stove.py:103-170) fused, all Ts = T-skip steps in one launch.
 * z1 (B,N,18) state at t=skip-1 [sx,sy/sx,x,y,vx,vy,latent]; zsup,zsstd (B,Ts,N,6) SuPAIR means/stds for
 * t=skip..T-1; eps (B,Ts,N,18) standard-normal draws; extra (B,Ts,N,sin_dim-16) or NULL.
 * outputs (B,Ts,N,.): z 18, zdyn 16, zdstd 16, mean 18, std 18, pred 32 (NULL to skip). */
/* act: saved activations (stove_dynloop_act_floats() floats, ~9 KB per sequence-step at N=3), written by the forward and
 * read by the backward.
 * DOMAIN (2 <= N <= 6, forward and rollout): layers 2 and 3 of the relation / attention chains multiply on IEEE-half hi / lo pieces
 * (three v_mfma_f32_16x16x32_f16 per product): their input activations must stay below 65 504 in magnitude (beyond it the pieces are
 * inf and the outputs inf / NaN -- never finite garbage); an operand keeps max(2^-22 |x|, 2^-25) of absolute precision, i.e. weights
 * below 1/4 lose relative, not absolute, accuracy (tests/test_gpu_dynamics.py::test_recursion_forward_chains_domain_*).
 * The backward normalises every gradient column by a power of two first and has no such bound.
 * With 2 <= N <= 6 objects the small-graph kernels run (csrc/gnn_small*.hip: one wave per node row up to
 * four objects, one HALF-wave per node row and two tiles of edge columns for five and six): act is then REQUIRED by the backward
 * (the layout is a set of per-sequence streams), and the backward consists of a T-serial data-gradient launch plus a
 * weight-gradient launch over the streams; its workspace is sized by stove_dynloop_bwd_ws_bytes_ts.  For N > 6 (MFMA kernels of
 * csrc/gnn.hip) act may be NULL in both calls: the backward then recomputes each step. */
size_t stove_dynloop_act_floats(int B, int Ts, int N);
int stove_dynloop_fwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                      const float* params, float* z, float* zdyn, float* zdstd, float* mean, float* std_, float* pred,
                      float* act, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                      void* stream);
size_t stove_dynloop_bwd_ws_bytes(int B, int N);
size_t stove_dynloop_bwd_ws_bytes_ts(int B, int Ts, int N);   /* the one to use (covers the streamed per-step gradients) */
/* upstream gradients dz,dzdyn,dmean,dstd,dpred may each be NULL. */
int stove_dynloop_bwd(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                      const float* params, const float* z, const float* act, const float* dz, const float* dzdyn,
                      const float* dmean, const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd, float* dextra,
                      float* g_params, void* ws, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                      float vel_std, float lat_std, void* stream);

/* The same with the weight-gradient work (g_params) on a second stream; the data gradients (dz1, dzsup, dzsstd, dextra) are
 * complete in `stream` order, g_params in `param_stream` order (see stove_scene_bwd_overlap). */
int stove_dynloop_bwd_overlap(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                              const float* params, const float* z, const float* act, const float* dz, const float* dzdyn,
                              const float* dmean, const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd,
                              float* dextra, float* g_params, void* ws, int B, int Ts, int N, int sin_dim, int lim_enc, int elu,
                              float pos_var, float vel_std, float lat_std, void* stream, void* param_stream);


/* ---- reward head of the action-conditioned dynamics model (dynamics.py:62-70, 254-263):
 *   reward = sigmoid(head1(sum over objects of head0(dynamic_pred))),  head0 = Linear(32,32) ReLU Linear(32,32),
 *   head1 = Linear(32,16) ReLU Linear(16,8) ReLU Linear(8,1), one kernel each way (cl = 32).
 * pred (items, n_obj, 32): the dynamics core's `dynamic_pred` rows, items = sequences x steps; reward (items).
 * params: the ten tensors in module order, nn.Linear layout, one after the other (stove_reward_head_param_floats() = 2785 floats):
 *   head0.0.weight (32,32) | .bias | head0.2.weight (32,32) | .bias | head1.0.weight (16,32) | .bias | head1.2.weight (8,16) | .bias |
 *   head1.4.weight (1,8) | .bias.  saved: stove_reward_head_saved_floats(items, n_obj) floats written by the forward, read by the backward.
 * bwd: d_reward (items) -> d_pred (items, n_obj, 32) and g_params (2785 floats, same layout; fixed summation order);
 * ws: stove_reward_head_bwd_ws_floats(items) floats. */
size_t stove_reward_head_param_floats(void);
size_t stove_reward_head_saved_floats(int items, int n_obj);
size_t stove_reward_head_bwd_ws_floats(int items);
int stove_reward_head_fwd(const float* pred, const float* params, float* reward, float* saved, int items, int n_obj, void* stream);
int stove_reward_head_bwd(const float* pred, const float* params, const float* reward, const float* saved, const float* d_reward, float* d_pred,
                          float* g_params, float* ws, int items, int n_obj, void* stream);

/* y (rows, out) = x (rows, in) W^T + b for a narrow layer (in, out <= 64; the action embedding Linear(action_space, 4 N) of
 * dynamics.py:238-244), exact fp32 FMAs; b NULL = no bias; w_transposed != 0: W is (in, out) (the layer's backward dx = dy W). */
int stove_small_linear(const float* x, const float* W, const float* b, float* y, int rows, int in_dim, int out_dim, int w_transposed, void* stream);

/* ---- Stove.rollout (stove.py:777-861), mean prediction: z_last (B,N,18) [sx,sy,...] ->
 * z_pred (B,num,N,18); zstd (B,num,N,16) and pred (B,num,N,32) optional; extra (B,A,N,E) cycled (t % A). */
int stove_rollout_fwd(const float* z_last, const float* extra, const float* params, float* z_pred, float* zstd, float* pred,
                      int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std,
                      float lat_std, void* stream);

/* ---- Stove.rollout(sample=True) (stove.py:836-841), all steps in one launch: eps (B,num,N,16) standard-normal draws;
 * per step z = mean + sd eps with mean the mean rollout's prediction from the DRAWN previous state and sd = zstd; z_pred receives
 * [scale, z] and z feeds the next step; log_q (B,num,N,16) = log N(z; mean, sd) = -eps^2/2 - log sd - log(2 pi)/2.  eps and log_q are
 * required (NULL: hipErrorInvalidValue, nothing launched), zstd and pred optional; everything else as stove_rollout_fwd, whose
 * z_pred this call reproduces bit for bit at eps = 0. */
int stove_rollout_sample_fwd(const float* z_last, const float* extra, const float* params, const float* eps, float* z_pred,
                             float* log_q, float* zstd, float* pred, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu,
                             float pos_var, float vel_std, float lat_std, void* stream);

/* ---- Backward of stove_rollout_fwd (eps NULL) and of stove_rollout_sample_fwd (eps: the draws the forward was given), all steps in
 * one launch plus the fixed-order reduction of the weight gradients; one stream, no synchronisation (the call can be captured).
 * z_pred is the forward's output: step t is recomputed from z_pred[:, t-1] (z_last at t = 0; when sampling, the drawn state), so no
 * activations are stored.  Upstream gradients: d_z_pred (B,num,N,18), d_log_q (B,num,N,16), d_pred (B,num,N,32); each may be NULL
 * (= zeros), d_log_q only with eps.  zstd and eps get no gradient.  Outputs, every element written by the call: d_z_last (B,N,18)
 * (the scale columns receive the sum of d_z_pred's over the steps), d_extra (B,A,N,E) (NULL exactly when extra is; row t % A
 * accumulates its steps in a fixed order, a row no step reads is zero), g_params (stove_gnn_grad_floats() floats, [dW | dvectors]).
 * B == 0 or num == 0: the outputs are zeros.  ws: stove_rollout_bwd_ws_bytes(B, N) bytes (0 for a B or N the call rejects).
 * NULL required pointer, d_log_q without eps, NULL ws, N or sin_dim out of range: hipErrorInvalidValue, nothing launched.
 * No atomics: two calls on the same inputs agree bit for bit. */
size_t stove_rollout_bwd_ws_bytes(int B, int N);
int stove_rollout_bwd(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                      const float* d_z_pred, const float* d_log_q, const float* d_pred, float* d_z_last, float* d_extra,
                      float* g_params, void* ws, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                      float vel_std, float lat_std, void* stream);

/* ---- One expansion of M search trees on the learned model (reference mcts/mcts_stove.py:95-137, 186-196; csrc/plan.hip), cl = 32,
 * action-conditioned.  z_pool (M, cap, N, 18): the trees' node states, resident on the device.  Per tree m: leaf[m] the pool slot of
 * the selected leaf, child[m] the first of A consecutive slots that receive its children, len_s[m] the reference's key length of the
 * leaf (the root counts 1; 1 <= len_s <= D).  app (M, N, app_dim) per-tree appearance (NULL with app_dim = 0); acts (M A, L) action
 * indices in [0, A) of the random rollout; emb_w (4 N, A), emb_b (4 N): the action-embedding nn.Linear; gnn_params: the image
 * stove_rollout_fwd takes; rh_params: the reward head's stove_reward_head_param_floats() floats.
 * Row (m, a) runs the mean rollout 1 + L steps from z_pool[m, leaf[m]]: action a, then acts[m A + a, k] at step 1 + k; a step's extra
 * inputs are column `action` of emb_w plus emb_b, viewed (N, 4), followed by the tree's appearance.  The state after step 0 goes to
 * z_pool[m, child[m] + a] (bit for bit stove_rollout_fwd's); with r0, rk the reward head on steps 0 and 1 + k,
 *   q[m,a] = (r0 - 1) gamma^len_s + (sum_{k < min(2 D - len_s + 1, L)} (rk - 1)) (sum_{j = len_s}^{D - 1} gamma^j)
 * in a fixed summation order.  Outputs q (M, A), r_first (M, A), r_roll (M, A, L); the last two may be NULL.
 * Three launches on `stream`, no host synchronisation (the call can be captured).  ws: stove_plan_expand_ws_bytes() bytes (0 for
 * dimensions the call rejects).  Host-checkable arguments (NULL pointers, M, A, L, N, D < 1, N > 8, 20 + app_dim > 32, A > 64,
 * cap < 1 + A): hipErrorInvalidValue, nothing launched.  A tree with leaf, child .. child + A - 1, len_s or any of its action indices
 * out of range reads and writes nothing out of bounds: its q / r_first / r_roll rows are NaN and the pool is not written for it. */
size_t stove_plan_expand_ws_bytes(int M, int A, int L, int N, int app_dim);
int stove_plan_expand(float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app,
                      const int* acts, const float* emb_w, const float* emb_b, const float* gnn_params,
                      const float* rh_params, float* q, float* r_first, float* r_roll, void* ws,
                      int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                      float pos_var, float vel_std, float lat_std, float gamma, void* stream);

/* ---- A whole search of M trees with the trees on the device (csrc/plan_tree.hip, csrc/plan_tree.h; the host forest of
 * stove_amd/mcts/mcts_stove.py is the specification).  Per tree `cap` entries, slot 0 the root: first (first child slot or -1), parent,
 * depth (key length - 1), Ns, Nsa (M, cap) int32, Qsa (M, cap) double; used (M,) the next free slot; z_pool (M, cap, N, 18) as in
 * stove_plan_expand.  For i = 0 .. R-1, on `stream`, nothing synchronised and nothing read by the host: select (UCT descent with the
 * reference's carried best value and action, c = 1; the leaf's child slots -- its own if it has them, else A fresh ones from `used`;
 * sel_trace[i, m] = leaf if sel_trace is given), the three launches of stove_plan_expand with acts + i M A L (acts (R, M A, L)),
 * backpropagate of the q they wrote; then action[m] = first-index argmax of Nsa over the root's children (0 for a root without).
 * min_gap (M,) in/out: lowered to the smallest finite gap between the two best UCT candidates of any level walked.  Qsa equals the host
 * forest's bit for bit (no contraction; log is the only library call, in the exploration term).
 * status (M,) in/out: 0 fine; 1 the tree ran out of slots (a fresh leaf with used + A > cap); 2 a walk or index check failed (arrays
 * or action indices out of range).  A tree with non-zero status is frozen: arrays and pool slots as before the offending iteration
 * (sel_trace -1 from there on), the other trees unaffected; nothing is read or written out of bounds.  No atomics.
 * ws: stove_plan_search_ws_bytes() bytes (0 for dimensions the call rejects).  What stove_plan_expand rejects, a NULL array, R < 0:
 * hipErrorInvalidValue, nothing launched.  R == 0 is valid: only `action` is written (acts may then be NULL). */
size_t stove_plan_search_ws_bytes(int M, int A, int L, int N, int app_dim);
int stove_plan_search(float* z_pool, int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used,
                      double* min_gap, int* status, int* action, int* sel_trace, const float* app, const int* acts,
                      const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, void* ws,
                      int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                      float pos_var, float vel_std, float lat_std, float gamma, int R, void* stream);

/* ---- The environments the planner plays: M avoidance / billiards environments stepped once and rendered, in place (csrc/env.hip,
 * csrc/env_step.h; stove_amd/envs/envs.py -- PhysicsEnv.step, BillardsEnv.simulate_physics, AvoidanceTask.step, draw_image -- is the
 * specification).  x, v (M, N, 2) double in/out; r, m (M, N) double; 1 <= N <= 6.  action (M,) indices into the nine directions of
 * AvoidanceTask.action_selection (0: acting with zero force; ball 0 gets direction * action_force * t), or NULL: plain billiards, ball 0
 * left alone and no collision counts as controlled.  `granularity` substeps of: x += t eps v; friction; walls on the next position;
 * (nothing more with `drift`); the i > j pair loop with the controlled-ball rule.  collisions (M,): 1 if a controlled collision
 * happened.  frames (M, 3, res, res) float or NULL: draw_image of the new state in float64 (BALL_COLOURS with use_colors, else ball i
 * on channel i % 3), clamped at 1, rounded to float32 once.  Every operation on the state is an IEEE double add, multiply, divide or
 * sqrt, uncontracted: x and v equal stove_amd/envs/batched.py's host arithmetic bit for bit.
 * status (M,): 0 stepped; 2 the environment's action index is outside [0, 9) -- its x, v, collisions and frame are not written, the
 * other environments are unaffected.  One launch on `stream`, no synchronisation (the call can be captured), no atomics.  A NULL x, v,
 * r, m, collisions or status, M < 0, N outside 1 .. 6, granularity < 1, res < 1: hipErrorInvalidValue, nothing launched.  M == 0 is a
 * valid empty call. */
int stove_env_step(double* x, double* v, const double* r, const double* m, const int* action, int* collisions, int* status,
                   float* frames, int M, int N, int granularity, int res, int use_colors, int drift, double hw, double t,
                   double friction, double action_force, void* stream);

/* ---- Data synthesis: B whole sequences of T steps in one launch (csrc/env_sequences.hip, csrc/env_step.h, csrc/env_gravity.h;
 * stove_amd/envs/synth.py's numpy arithmetic is the specification, itself held to stove_amd/envs/envs.py).  x0, v0 (B, N, 2), r, m (B, N)
 * double, the start states: read only; 1 <= N <= 6.  kind 0: billiards, stepped as stove_env_step steps, with actions (B, T) -- step s of
 * sequence b takes actions[b][s] -- or NULL for plain billiards.  kind 1: gravity (PhysicsEnv.step with the centre-of-mass shift +
 * GravityEnv.simulate_physics: G = 0.5, softening 1e-5, the pull to the middle, forces clipped to [-1, 1]); it takes no actions, and r is
 * used by the frames only.  y (B, T, N, 4): (x, v) after each step.  frames (B, T, 3, res, res) float or NULL: the frame of y[b][s], as
 * stove_env_step paints it.  collisions (B, T): 1 if step s had a controlled collision (0 for gravity).  in_bounds (B,): the number of
 * (step, ball, axis) position coordinates strictly inside (0, hw), the integer behind the reference's acceptance rule for generated runs.
 * The states equal the specification's bit for bit (IEEE double add, multiply, divide, sqrt, uncontracted; norms as sqrt(a a + b b), cubes
 * as d d d); frames agree to one float32 ulp.
 * status (B,): 0 done; 2 one of the sequence's T action indices is outside [0, 9) -- none of its y, frames, collisions or in_bounds rows
 * is written, the other sequences are unaffected.  One launch on `stream`, one workgroup per sequence, no synchronisation, no atomics.
 * A NULL x0, v0, r, m, y, collisions, in_bounds or status, B < 0, N outside 1 .. 6, T < 1, granularity < 1, res < 1 or res^2 >= 2^28, kind
 * outside {0, 1}, kind 1 with actions: hipErrorInvalidValue, nothing launched.  B == 0 is a valid empty call. */
int stove_env_sequences(const double* x0, const double* v0, const double* r, const double* m, const int* actions, double* y,
                        float* frames, int* collisions, int* in_bounds, int* status, int B, int N, int T, int granularity, int res,
                        int use_colors, int drift, int kind, double hw, double t, double friction, double action_force, void* stream);

/* ---- Data synthesis: the starts and action rows of B sequences drawn in one launch (csrc/env_draw.hip, csrc/env_draw.h;
 * stove_amd/envs/synth.py's draw_starts_counter is the specification).  Sequence b is a pure function of its seed, seed0 + b with seed0 =
 * seed_hi 2^32 + seed_lo, through Philox4x32-10 counters (stream, attempt, block): NOT the numbers numpy's RandomState gives the host
 * path, the same distributions.  r (B, N) double, the radii: read only; 1 <= N <= 6.  kind 0, billiards (PhysicsEnv.init_x / init_v):
 * attempt k draws x = u hw / 2 + hw / 4 and is good iff every ball lies inside [r, hw - r] and no pair is closer than r_i + r_j; the
 * start is the good attempt with the lowest index among 0 .. max_tries - 1; v is 2 N normals scaled to the norm 0.5, times
 * uniform(1 / v_factor, v_factor) where v_factor > 0.  kind 1, gravity (GravityEnv.init_x / init_v): x = u 0.9 hw / 2 + hw / 2, good iff
 * all pairs are farther apart than hw / 3; the lowest good attempt among 0 .. 999, else attempt 999 (max_tries is not consulted); v from
 * the sign draw and two normals per ball around v_factor.  x0, v0 (B, N, 2) double.  tries (B,): the index of the attempt taken plus one.
 * actions (B, T) or NULL: MonteCarloActionPolicy(9, 0.2 + 0.1 u)'s row, indices in [0, 9); drawn whatever the status.
 * status (B,): 0 drawn; 1 no good billiards attempt among max_tries -- x0 and v0 rows zero, tries = max_tries.  Every element of every
 * output is written.  The values equal the specification's bit for bit (integer arithmetic up to the uniform double, then IEEE double
 * add, multiply, divide, sqrt, uncontracted; the logarithm is env_draw.h's own).  One launch on `stream`, one wave per sequence, no
 * synchronisation (the call can be captured), no LDS, no atomics.  A NULL r, x0, v0, tries or status, B < 0, N outside 1 .. 6, T < 0,
 * max_tries < 1, kind outside {0, 1}: hipErrorInvalidValue, nothing launched.  B == 0 is a valid empty call. */
int stove_env_draw_starts(const double* r, double* x0, double* v0, int* actions, int* tries, int* status, uint32_t seed_lo,
                          uint32_t seed_hi, int B, int N, int T, int kind, int max_tries, double hw, double v_factor, void* stream);

/* ---- Tree search on those environments themselves (csrc/env_search.hip, csrc/env_search.h; the host forest EnvForest of
 * stove_amd/mcts/mcts_env.py is the specification): R independent trees per environment, T = M R, tree e R + k searching from
 * environment e's state x, v (M, N, 2), r, m (M, N) double, which is read only.  Nine actions, c = 1, rollout depth D >= 2.  Trees as in
 * stove_plan_search: per tree `cap` entries, slot 0 the root, first, parent, depth, Ns, Nsa (T, cap) int32, Qsa (T, cap) double, used
 * (T,) the next free slot; 1 + 9 runs slots always suffice.  draws (T, runs, D) int32 in [0, 9): iteration i of tree t reads row (t, i)
 * from column 0 on.  One iteration replays its path from the root state: Descend takes the first-index argmax of Qsa + sqrt(log Ns /
 * (1 + Nsa)) fresh at every level and steps; Expand (a node without children, key length < D) takes A fresh slots with Qsa = -1, Nsa =
 * 0, steps with column 0 and rolls out D - length more steps with the following columns, value = minus the collisions counted;
 * Terminal (key length D - 1, expanded) takes no step, value = Qsa of the edge drawn with column 0, counts edge 0 and leaves its Qsa
 * alone.  Ns and Nsa are raised and Qsa averaged from there up to the root.  All `runs` iterations of all trees in one launch, then
 * action[e] = first-index argmax of the root's Nsa summed over environment e's R trees (0 for an empty search).
 * min_gap (T,) in/out: lowered to the smallest u_best - u_a over the Descend levels walked, among a whose (Qsa, Nsa) differ from the
 * best's.  Qsa equals the host forest's bit for bit (no contraction; log is the only library call).
 * status (T,) in/out: 0 searched; 1 out of slots (an expansion with used + 9 > cap); 2 a draw outside [0, 9) or a failed index check.
 * A tree with non-zero status is frozen as it stood at the start of the offending iteration, the other trees unaffected; nothing is
 * read or written out of bounds.  On `stream`, no synchronisation (the call can be captured), no atomics.  A NULL array, M < 0, R < 1,
 * N outside 1 .. 6, D < 2, runs < 0, cap < 10, granularity < 1: hipErrorInvalidValue, nothing launched.  M == 0 is a valid empty call;
 * with runs == 0 only `action` is written (draws may then be NULL). */
int stove_env_search(const double* x, const double* v, const double* r, const double* m, const int* draws, int* first, int* parent,
                     int* depth, int* Ns, int* Nsa, double* Qsa, int* used, double* min_gap, int* status, int* action, int M, int R,
                     int N, int D, int runs, int cap, int granularity, int drift, double hw, double t, double friction,
                     double action_force, void* stream);

/* ---- The model-free PPO arm on states: S steps of B of those environments under a policy, next_value and the discounted returns in
 * one launch (csrc/ppo_collect.hip, csrc/ppo_policy.h; the host forest PolicyForest of stove_amd/rl/collect.py is the specification).
 * The policy is Policy(base='control') of stove_amd/rl/rl_model.py: Linear(4N, 128), ReLU, Linear(128, 32), ReLU, Linear(32, H), ReLU
 * [with `deep`: Linear(H, H), ReLU, Linear(H, H), ReLU], then the value (H -> 1) and nine logits (H -> 9); 1 <= N <= 6, 1 <= H <= 128.
 * params: stove_ppo_param_floats(N, H, deep) floats (0 for an N or H outside its range), the layers in that order, each as its
 * TRANSPOSED weight wT[k * out + j] = weight[j][k] followed by its bias (out); the last layer is the two heads side by side, out = 10,
 * column 0 the value head, columns 1 .. 9 the actor head (Policy.flat_params() writes it).
 * Step s of environment b: obs[b][s] = (x[i][0], x[i][1], v[i][0], v[i][1])_i rounded to float32; every neuron is one float32 sum
 * that starts at its bias and adds w[k] * in[k] for k ascending, uncontracted; values[b][s] the value; the action is drawn from the
 * logits with the caller's uniform u[b][s] in [0, 1): d_a = l_a - max l in float32, c_a the running double sum of exp(d_a), the first a
 * with c_a > u c_8 (else 8), logp = d_a - log c_8 rounded to float32; then stove_env_step's step with that action, rewards[b][s] =
 * -collisions.  After step S - 1: obs[b][S], next_value[b] the value there, returns[b][s] = returns[b][s + 1] * discount + rewards[b][s]
 * in float32 (discount rounded to float32 once).  x, v (B, N, 2) double in/out; r, m (B, N) double; u, rewards, values, logp, returns
 * (B, S) float; actions (B, S) int32; obs (B, S + 1, 4N) float; next_value (B,) float.  Everything but logp (exp, log) equals the host
 * forest bit for bit wherever the uniform is not within a last-bit error of exp of a boundary.
 * status (B,): 0 collected; 3 a value or logit was not finite at some step: nothing of that step or after it is written (no obs row, no
 * next_value, no returns), x and v stand as the steps before left them, the other environments are unaffected.  One launch on `stream`,
 * no synchronisation (the call can be captured), no atomics.  A NULL array, B < 0, S < 0, N outside 1 .. 6, H outside 1 .. 128,
 * granularity < 1: hipErrorInvalidValue, nothing launched.  B == 0 is a valid empty call; with S == 0 only obs (B, 1, 4N), next_value
 * and status are written (the (B, S) arrays may then be NULL). */
size_t stove_ppo_param_floats(int N, int H, int deep);
int stove_ppo_collect(double* x, double* v, const double* r, const double* m, const float* params, const float* u, float* obs,
                      int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status, int B,
                      int S, int N, int H, int deep, int granularity, int drift, double hw, double t, double friction,
                      double action_force, double discount, void* stream);

/* ---- The model-based PPO arm: S imagined steps of B trajectories on the learned, action-conditioned cl = 32 model under that policy,
 * next_value and the discounted returns in one launch (csrc/ppo_model.hip; reference runners.py: run_pretrained_batch).  One workgroup
 * per trajectory, laid out as the small-graph rollout (one object: as the general rollout, which is what stove_rollout_fwd runs there);
 * 1 <= N <= 6, 1 <= H <= 128, nine actions, 20 + app_dim <= 32.
 * z0 (B, N, 18) the start states [sx, sy, x, y, vx, vy, latent]; app (B, N, app_dim) the appearance rows (NULL with app_dim == 0);
 * policy_params the image of stove_ppo_param_floats(N, H, deep); emb_w (4N, 9), emb_b (4N) the action embedding Linear; gnn_params the
 * stove_gnn_param_floats() image, rh_params the stove_reward_head_param_floats() one; u (B, S) uniforms in [0, 1).
 * Step s of trajectory b, from the state z (z0 at s == 0, else z_pred[b][s - 1]):
 *   obs[b][s][4i + c] = (z[i][2 + c] + 1.0f) / 2.0f * hw for c < 2 (positions), z[i][2 + c] / 2.0f * hw for c = 2, 3 (velocities), every
 *   operation rounded to float32 on its own, hw rounded to float32 once;
 *   values[b][s], actions[b][s], logp[b][s] from the policy on that row exactly as stove_ppo_collect computes them;
 *   the model's extra inputs [embedding column of the action + bias (the bits of stove_small_linear on a one-hot row) | app];
 *   z_pred[b][s], pred[b][s] (optional, NULL to skip): the bits of stove_rollout_fwd with num = A = S on those inputs;
 *   rewards[b][s] = r - 1.0f with r the bits of stove_reward_head_fwd on pred[b][s].
 * After step S - 1: obs[b][S], next_value[b], returns[b][s] = returns[b][s + 1] * discount + rewards[b][s] in float32 (no episode ends).
 * pos_var, vel_std, lat_std are the model's scales; this rollout puts out no deviations and does not read them.
 * status (B,): 0 collected; 3 a value or logit was not finite at some step (a NaN in z0, say): nothing of that step or after it is
 * written (no obs row, no z_pred, no next_value, no returns), the other trajectories are unaffected.  One launch on `stream`, no
 * synchronisation (the call can be captured), no atomics, deterministic.  A NULL required array, B < 0, S < 0, N outside 1 .. 6, H
 * outside 1 .. 128, app_dim outside 0 .. 12, lim_enc outside 0 .. 32: hipErrorInvalidValue, nothing launched.  B == 0 is a valid empty
 * call; with S == 0 only obs (B, 1, 4N), next_value and status are written (the (B, S) arrays and z_pred may then be NULL). */
int stove_ppo_collect_model(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                            const float* gnn_params, const float* rh_params, const float* u, float* z_pred, float* pred, float* obs,
                            int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status, int B,
                            int S, int N, int H, int deep, int app_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                            float hw, float discount, void* stream);

/* ---- The model-free PPO arm on images: `warm` warm-up steps and S steps of B of those environments under the image policy, next_value
 * and the discounted returns in one launch (csrc/ppo_image.hip, csrc/ppo_image.h; the host forest ImageForest of
 * stove_amd/rl/collect.py is the specification).  The policy is Policy((32, 32, 3F), 9) of stove_amd/rl/rl_model.py: frame / 255.0f,
 * Conv2d(3F, 32, 4, stride 2), ReLU, Conv2d(32, 32, 3, stride 2), ReLU, flatten, Linear(1568, H), ReLU [with `deep`: Linear(H, H), ReLU,
 * Linear(H, H), ReLU], then the value and nine logits; 1 <= F <= 4, 1 <= H <= 512, 1 <= N <= 6; frames are 32 x 32.
 * params: stove_ppo_image_param_floats(F, H, deep) floats (0 for an F or H outside its range), the layers in that order, each as its
 * TRANSPOSED weight wT[k * out + j] followed by its bias (out): conv1 (48F -> 32) with k = (c * 4 + ky) * 4 + kx and input channel
 * c = f * 3 + ch, f counted from the oldest frame of the window; conv2 (288 -> 32) with k = (c * 3 + ky) * 3 + kx; head.main
 * (1568 -> H) with k = c * 49 + y * 7 + x; the deep layers; the two heads side by side as for stove_ppo_collect
 * (Policy.flat_image_params() writes it).
 * frames (B, F + S, 3, 32, 32) float, each row in the layout stove_env_step writes.  Before step 0 the environment takes `warm` >= 1 steps
 * with action 0 whose rewards are dropped; rows 0 .. F - 1, the first window, are the last min(warm, F) frames rendered after them, zeros
 * before those.  Step s of environment b reads rows s .. s + F - 1 (the stacked observation is never stored): every convolution output
 * and neuron is one float32 sum that starts at its bias and adds w[k] * in[k] for k ascending, uncontracted; values[b][s] the value;
 * the action drawn with u[b][s] and logp as stove_ppo_collect does; then stove_env_step's step, rewards[b][s] = -collisions, and the new
 * frame, row F + s.  After step S - 1: next_value[b] the value on rows S .. S + F - 1, returns as for stove_ppo_collect.
 * x, v (B, N, 2) double in/out; r, m (B, N) double; u, rewards, values, logp, returns (B, S) float; actions (B, S) int32; next_value
 * (B,) float.
 * status (B,): 0 collected; 3 a value or logit was not finite at some step s: nothing of that step or after it is written (with s == 0
 * not even the first window), x and v stand as the steps before -- the warm-up included -- left them, the other environments are
 * unaffected.  One launch on `stream`, one workgroup per environment, no synchronisation (the call can be captured), no atomics.  A NULL
 * array, B < 0, S < 0, N outside 1 .. 6, F outside 1 .. 4, H outside 1 .. 512, warm < 1, granularity < 1: hipErrorInvalidValue, nothing
 * launched.  B == 0 is a valid empty call; with S == 0 only the first window (frames (B, F, 3, 32, 32)), next_value and status are written
 * (the (B, S) arrays may then be NULL). */
size_t stove_ppo_image_param_floats(int F, int H, int deep);
int stove_ppo_collect_images(double* x, double* v, const double* r, const double* m, const float* params, const float* u, float* frames,
                             int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status,
                             int B, int S, int N, int F, int H, int deep, int warm, int granularity, int drift, int use_colors, double hw,
                             double t, double friction, double action_force, double discount, void* stream);

/* ---- The PPO arm's update: every epoch and mini-batch of PPOAgent.update (stove_amd/rl/agents.py, the specification), E x M
 * dependent optimiser steps, in ONE launch of one workgroup (csrc/ppo_update.hip, csrc/ppo_update.h).  params: the image above, in/out;
 * m, v: Adam's moments in the image's layout, in/out; step (1,) in/out: the optimiser's step count.  obs (n, 4N) float; actions (n,)
 * int32 in 0 .. 8; returns, values, logp, adv (n,) float; perm (E, n) int32: epoch e's permutation of 0 .. n - 1.  Step e M + i works on
 * the mb = n / M rows perm[e][i mb .. (i + 1) mb - 1] (the trailing n - M mb indices of an epoch are never read): the forward of each
 * row, log-softmax and entropy in float64, ratio = exp(new_logp - logp), the surrogate -min(ratio adv, clamp(ratio, 1 - clip, 1 + clip)
 * adv), the value loss 0.5 max((v - R)^2, (v_old + clamp(v - v_old, -clip, clip) - R)^2) (0.5 (v - R)^2 with clipped_value_loss == 0),
 * their means over the rows, the loss value_loss * value_coef + action_loss - entropy * entropy_coef and its gradient as torch's
 * autograd gives it (equal arguments of min / max share the gradient, a clamp passes it on its closed range); every weight and bias
 * gradient is one float32 sum over the rows in order; the norm in float64, the factor min(1, max_grad_norm / (norm + 1e-6)), then
 * torch.optim.Adam with betas (0.9, 0.999), no weight decay and eps outside the root.  losses (E M, 3): value loss, action loss,
 * entropy of each step; gnorm (E M,): its gradient norm before clipping.  max_steps stops after that many steps (E M runs them all).
 * status (2,): [0] 0 completed; 2 an index of perm outside 0 .. n - 1 or an action outside 0 .. 8 among a step's rows (device memory:
 * the kernel checks it, as everywhere in this interface); 3 a loss or the gradient norm of a step was not finite.  With 2 or 3 that step
 * and everything after it change nothing: params, m, v and step stand as the step before left them and the later rows of losses and
 * gnorm are not written.  [1] the number of steps completed.  Deterministic: the same inputs give the same bits.  One launch on `stream`,
 * no synchronisation (the call can be captured), no atomics.  A NULL array, n < M, M < 1, E < 0, max_steps outside 0 .. E M, N outside
 * 1 .. 6, H outside 1 .. 128: hipErrorInvalidValue, nothing launched.  E == 0 and max_steps == 0 are valid empty calls. */
int stove_ppo_update(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns,
                     const float* values, const float* logp, const float* adv, const int* perm, float* losses, float* gnorm, int* status,
                     int n, int E, int M, int max_steps, int N, int H, int deep, float clip, float value_coef, float entropy_coef, float lr,
                     float eps, float max_grad_norm, int clipped_value_loss, void* stream);

/* ---- The update of the PPO arm on images: every epoch and mini-batch of PPOAgent.update for the image policy above, E x M dependent
 * optimiser steps, as one call that enqueues a fixed chain of launches per step on `stream` (csrc/ppo_image_update.hip): nothing is
 * synchronised or allocated inside, so the call can be captured as a linear chain.  params, m, v: stove_ppo_image_param_floats(F, H, deep)
 * floats in the layout of stove_ppo_collect_images, in/out; step (1,) in/out.  Row r of the n rows has its observation, the window of
 * 3072 F floats (3F, 32, 32) with pixels in the frames' scale (the division by 255 happens on the way in), at
 * obs + (r / S) env_stride + (r % S) 3072 floats: frames (B, F + S, 3, 32, 32) as stove_ppo_collect_images wrote them with
 * env_stride = (F + S) 3072 and n = B S, or a dense (n, 3F, 32, 32) tensor with S = 1, env_stride = 3072 F.  actions (n,) int32; returns,
 * values, logp, adv (n,) float; perm (E, n) int32.  Steps, mini-batches, losses, the gradient as autograd gives it, the norm, the clip
 * factor and Adam are those of stove_ppo_update; losses (E M, 3), gnorm (E M,), max_steps and status (2,) mean what they mean there
 * (status 2: an index or action out of range; 3: a loss or norm not finite; that step and all after it change nothing; [1] the steps
 * completed).  The three wide products of each layer run on the float32 matrix instructions; every sum has a fixed order (no atomics),
 * so equal inputs give equal bits.  grad: NULL, or stove_ppo_image_param_floats floats that receive the unclipped gradient image of the
 * last step completed, in the parameters' layout.  ws: stove_ppo_update_images_ws_bytes(n, M, F, H, deep) bytes of device memory, 16-byte
 * aligned (0 for a shape that is not served).  A NULL array, n < M, M < 1, S < 1, E < 0, max_steps outside 0 .. E M, F outside 1 .. 4,
 * H outside 1 .. 512: hipErrorInvalidValue, nothing launched.  E M == 0 and max_steps == 0 are valid empty calls: one launch that writes
 * status; the other arrays and ws may then be NULL. */
size_t stove_ppo_update_images_ws_bytes(int n, int M, int F, int H, int deep);
int stove_ppo_update_images(float* params, float* m, float* v, int* step, const float* obs, const int* actions, const float* returns,
                            const float* values, const float* logp, const float* adv, const int* perm, float* losses, float* gnorm,
                            float* grad, int* status, void* ws, int n, int S, int env_stride, int E, int M, int max_steps, int F, int H,
                            int deep, float clip, float value_coef, float entropy_coef, float lr, float eps, float max_grad_norm,
                            int clipped_value_loss, void* stream);

/* ---- The GNN step, the inference recursion and the rollout at state-code lengths other than 32 (csrc/gnn_cl.hip): cl = 16 or 64,
 * 1 <= N <= 6, cl/2 <= sin_dim <= cl.  Same conventions as their cl = 32 siblings above with every width derived from cl:
 * params is the image [W | W^T | vectors] of stove_gnn_param_floats_cl(cl) floats (no packed sections), result / pred (B,N,cl),
 * states cl/2 + 2 wide, dyn means / stds cl/2, extra (B,Ts,N,sin_dim - cl/2).  Any other cl, N or sin_dim: hipErrorInvalidValue.
 * The recursion runs all Ts steps in one launch each way (the backward recomputes each step's forward, so there is no `act` buffer)
 * plus one fixed-order reduction launch for the weight gradients; ws: stove_gnn_bwd_ws_bytes_cl(cl, B, N) bytes.
 * An empty batch (B == 0, or Ts == 0 for the recursion) is a valid call everywhere; the backwards then zero g_params. */
size_t stove_gnn_param_floats_cl(int cl);
size_t stove_gnn_grad_floats_cl(int cl);
size_t stove_gnn_bwd_ws_bytes_cl(int cl, int B, int N);
int stove_gnn_fwd_cl(const float* s_in, const float* params, float* result, float* pred, int cl, int B, int N, int sin_dim,
                     int lim_enc, int elu, void* stream);
int stove_gnn_bwd_cl(const float* s_in, const float* params, const float* d_result, const float* d_pred, float* d_s_in,
                     float* g_params, void* ws, int cl, int B, int N, int sin_dim, int lim_enc, int elu, void* stream);
int stove_dynloop_fwd_cl(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                         const float* params, float* z, float* zdyn, float* zdstd, float* mean, float* std_, float* pred,
                         int cl, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std, float lat_std,
                         void* stream);
int stove_dynloop_bwd_cl(const float* z1, const float* zsup, const float* zsstd, const float* eps, const float* extra,
                         const float* params, const float* z, const float* dz, const float* dzdyn, const float* dmean,
                         const float* dstd, const float* dpred, float* dz1, float* dzsup, float* dzsstd, float* dextra,
                         float* g_params, void* ws, int cl, int B, int Ts, int N, int sin_dim, int lim_enc, int elu, float pos_var,
                         float vel_std, float lat_std, void* stream);
int stove_rollout_fwd_cl(const float* z_last, const float* extra, const float* params, float* z_pred, float* zstd, float* pred,
                         int cl, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu, float pos_var, float vel_std,
                         float lat_std, void* stream);
int stove_rollout_sample_fwd_cl(const float* z_last, const float* extra, const float* params, const float* eps, float* z_pred,
                                float* log_q, float* zstd, float* pred, int cl, int B, int num, int A, int N, int sin_dim, int lim_enc,
                                int elu, float pos_var, float vel_std, float lat_std, void* stream);
size_t stove_rollout_bwd_ws_bytes_cl(int cl, int B, int N);
int stove_rollout_bwd_cl(const float* z_last, const float* extra, const float* params, const float* eps, const float* z_pred,
                         const float* d_z_pred, const float* d_log_q, const float* d_pred, float* d_z_last, float* d_extra,
                         float* g_params, void* ws, int cl, int B, int num, int A, int N, int sin_dim, int lim_enc, int elu,
                         float pos_var, float vel_std, float lat_std, void* stream);

/* ---- The state-supervised baseline (csrc/gnn_sup.hip; reference model/supairvised): the interaction network on given object states
 * (x, y, vx, vy) at cl = 16 or 64, 1 <= N <= 6, V >= 1 observed frames, R >= 1 predicted ones.  With core = the GNN step on a cl-wide
 * code (sin_dim = cl, lim_enc = 4; params: the stove_gnn_param_floats_cl(cl) image that stove_rollout_fwd_cl takes):
 *   code_0 = [x[:, 0] | latent0];   warm-up i = 1..V-1: code_i = [x[:, i] | core(code_{i-1})[..., 4:]];
 *   rollout k = 0..R-1: res = core(cur), cur = [res[..., :2] + cur[..., :2] | res[..., 2:]], pred[:, k] = cur[..., :4].
 * stove_sup_rollout_fwd: x (B,V,N,4), latent0 (B,N,cl-4) -> pred (B,R,N,4) in one launch; codes (B,V-1+R,N,cl), optional, receives
 * the input code of every step, which is what the backward recomputes from.
 * stove_sup_rollout_bwd: d_pred (B,R,N,4) -> g_params (stove_gnn_grad_floats_cl(cl) floats) and d_latent0 (B,N,cl-4) (optional),
 * every element overwritten; x gets no gradient.  One launch over the steps in reverse plus the fixed-order reduction of the
 * per-workgroup weight gradients (no atomics: two calls agree bit for bit); ws: stove_sup_rollout_bwd_ws_bytes(cl, B, N) bytes, 0 for
 * what the call rejects.
 * stove_sup_loss: pred, future (B,R,N,4) -> losses[3] = (total, pred, delta) with, over the columns < end (2 or 4) and M = B N end,
 * pred = sum_t discount^(t+1) sum (pred_t - future_t)^2 / M and, with_delta != 0, delta = sum_{t<R-1} 6 discount^(t+1)
 * sum ((pred_{t+1} - pred_t) - (future_{t+1} - future_t))^2 / M; d_pred (B,R,N,4) = d total / d pred, zeros in the columns >= end.
 * One launch in one workgroup, summed in a fixed order; B, R >= 1.
 * B == 0 is a valid empty rollout call (the backward then zeroes g_params).  A NULL required pointer, any other cl, N, V, R or end, or
 * a NULL ws: hipErrorInvalidValue, nothing launched. */
int stove_sup_rollout_fwd(const float* x, const float* latent0, const float* params, float* pred, float* codes, int cl, int B, int V,
                          int R, int N, int elu, void* stream);
size_t stove_sup_rollout_bwd_ws_bytes(int cl, int B, int N);
int stove_sup_rollout_bwd(const float* x, const float* params, const float* codes, const float* d_pred, float* d_latent0,
                          float* g_params, void* ws, int cl, int B, int V, int R, int N, int elu, void* stream);
int stove_sup_loss(const float* pred, const float* future, float* losses, float* d_pred, int B, int R, int N, int end, int with_delta,
                   double discount, void* stream);

/* ---- Planning at state-code lengths other than 32 (csrc/plan.hip, csrc/plan_tree.hip): stove_plan_expand and stove_plan_search with
 * every width derived from cl = 16 or 64 -- z_pool (M, cap, N, cl/2 + 2); gnn_params the stove_gnn_param_floats_cl(cl) image that
 * stove_rollout_fwd_cl takes, which is the rollout behind these calls (child states bit for bit its z_pred); a node's input row is
 * [state cl/2 | action embedding 4 | appearance], so 1 <= N <= 6 and app_dim <= cl/2 - 4 (4 at cl = 16, 28 at cl = 64).
 * rh_params: the reward head at that width, head0 = Linear(cl,cl) ReLU Linear(cl,cl) summed over the objects, head1 =
 * Linear(cl,cl/2) ReLU Linear(cl/2,cl/4) ReLU Linear(cl/4,1), the ten tensors in module order, nn.Linear layout:
 * stove_reward_head_param_floats_cl(cl) = 2 cl^2 + 2 cl + cl^2/2 + cl/2 + cl^2/8 + cl/4 + cl/4 + 1 floats (721 / 10945; 0 for any
 * other cl).  Launch counts, outputs, the value formula, status and the treatment of bad device indices are those of the cl = 32
 * calls; forward only.  Any other cl (32 included: it has its own entry points), and what those calls reject at this width's limits:
 * hipErrorInvalidValue, nothing launched; the workspace queries then return 0. */
size_t stove_reward_head_param_floats_cl(int cl);
size_t stove_plan_expand_ws_bytes_cl(int cl, int M, int A, int L, int N, int app_dim);
int stove_plan_expand_cl(float* z_pool, const int* leaf, const int* child, const int* len_s, const float* app,
                         const int* acts, const float* emb_w, const float* emb_b, const float* gnn_params,
                         const float* rh_params, float* q, float* r_first, float* r_roll, void* ws,
                         int cl, int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                         float pos_var, float vel_std, float lat_std, float gamma, void* stream);
size_t stove_plan_search_ws_bytes_cl(int cl, int M, int A, int L, int N, int app_dim);
int stove_plan_search_cl(float* z_pool, int* first, int* parent, int* depth, int* Ns, int* Nsa, double* Qsa, int* used,
                         double* min_gap, int* status, int* action, int* sel_trace, const float* app, const int* acts,
                         const float* emb_w, const float* emb_b, const float* gnn_params, const float* rh_params, void* ws,
                         int cl, int M, int cap, int A, int L, int D, int N, int app_dim, int lim_enc, int elu,
                         float pos_var, float vel_std, float lat_std, float gamma, int R, void* stream);

/* ---- The model-based PPO arm at state-code lengths other than 32 (csrc/ppo_model_cl.hip): stove_ppo_collect_model with every width
 * derived from cl = 16 or 64 -- z0 (B, N, cl/2 + 2), z_pred (B, S, N, cl/2 + 2), pred (B, S, N, cl) (optional); gnn_params the
 * stove_gnn_param_floats_cl(cl) image, rh_params the stove_reward_head_param_floats_cl(cl) block; everything else as there.  One
 * workgroup of 256 threads per trajectory, laid out as the rollout of stove_rollout_fwd_cl with one sequence per workgroup, every
 * object count 1 <= N <= 6 in the same kernel; a node's input row is [state cl/2 | action embedding 4 | appearance], so
 * app_dim <= cl/2 - 4 (4 at cl = 16, 28 at cl = 64).  Per step: obs, values, actions, logp exactly as stove_ppo_collect_model computes
 * them (the policy reads columns 2 .. 5 of a state row at every width); z_pred[b][s], pred[b][s]: the bits of stove_rollout_fwd_cl with
 * num = A = S on the extra rows [embedding column of the action + bias | app]; rewards[b][s] = r - 1.0f with r the bits of
 * stove_plan_expand_cl's r_first for that state and action.  next_value, returns, status (0 / 3) and what a trajectory that stops
 * leaves unwritten: as there.  One launch on `stream`, no synchronisation (the call can be captured), no atomics, deterministic.
 * cl other than 16 or 64 (32 included: it has its own entry point), a NULL required array, B < 0, S < 0, N outside 1 .. 6, H outside
 * 1 .. 128, app_dim outside 0 .. cl/2 - 4, lim_enc outside 0 .. cl, B (S + 1) N cl beyond an int: hipErrorInvalidValue, nothing
 * launched.  B == 0 is a valid empty call; with S == 0 only obs (B, 1, 4N), next_value and status are written (the (B, S) arrays and
 * z_pred may then be NULL). */
int stove_ppo_collect_model_cl(const float* z0, const float* app, const float* policy_params, const float* emb_w, const float* emb_b,
                               const float* gnn_params, const float* rh_params, const float* u, float* z_pred, float* pred, float* obs,
                               int* actions, float* rewards, float* values, float* logp, float* next_value, float* returns, int* status,
                               int cl, int B, int S, int N, int H, int deep, int app_dim, int lim_enc, int elu, float pos_var,
                               float vel_std, float lat_std, float hw, float discount, void* stream);

/* ---- Stove._3_only_match_objects / _greedy_match_objects / _volatile_match_objects
 * (stove.py:200-329, 432-514, 331-430): the T-serial nearest-neighbour re-ordering of objects.
 * feat (B,T,N,F) matching features in [-1,1] (positions [, appearance]); mode 0 = '3_only',
 * 1 = 'greedy', 2 = 'volatile', 3 = '3_only' forced through the frame-by-frame walk (the three-object '3_only' case
 * normally runs as a composition of per-frame transition tables, same indices).  idx (B,T,N) int64: current object assigned to slot a.
 * perm (B,T,N,N) f32, pre-zeroed, only written in mode 2 (may be NULL otherwise). */
int stove_match_objects(const float* feat, long long* idx, float* perm, int B, int T, int N, int F, int mode, void* stream);

/* ---- SuPAIR state pipeline and ELBO assembly (elementwise / short stencils in t; replaces ~180 ATen launches per step).
 * stove_supair_state_fwd: raw codes (n*T*o, 8) of the recognition LSTM ->
 *     zc (n,T,o,8) = constrain_zp (supair.py:112-149; span_low = 8 spans then 8 lows, HOST floats),
 *     idx (n,T,o) = object matching on the positions (mode as stove_match_objects; pos (n,T,o,2) is scratch),
 *     zfix (n,T,o,8) = gathered + fix_supair-smoothed [mean 4 | std 4] (stove.py:516-563; hits (n,T,o) u8 = its mask),
 *     zl / sl (n,T-skip,o,6) = z_sup_full / z_sup_std_full[:, skip:] with finite-difference velocities
 *     (stove.py:172-198), init6 (n,o,6) = z_sup_full[:, skip-1] (1 <= skip < T; at skip = 1 that is the zero row in front of
 *     frame 1, written like any other: no output element is left unwritten).
 *     codes == NULL: zc and idx are INPUTS (states already constrained, a matching already chosen) and only the gather /
 *     fix_supair / velocity stage runs -- what the reference's fix_supair fixtures exercise.
 * stove_supair_state_bwd: gradients of zfix / zl / sl / init6 (any may be NULL) -> g_codes; gfix_ws: n*T*o*8 floats.
 * stove_zall_fwd/bwd: z of the scene likelihood, frames 1..T-1: SuPAIR means before `skip`, sampled states after,
 *     [sx, sy/sx, x, y] -> [sx, sy, x, y] (stove.py:731-736); bwd writes every element of g_zfix and g_zs (n,T-skip,o,18).
 * stove_elbo_fwd: out3 = { mean_t,b(trans_lik + img_lik - log_q) + mean(img_lik_sup), mean trans_lik, mean log_q }
 *     (stove.py:738-748); lik (n,T-1); trans_std16 HOST floats; part_ws n*4 floats.  stove_elbo_bwd: g_out = device
 *     scalar dL/d out3[0]. */
int stove_supair_state_fwd(const float* codes, const float* span_low, float* zc, float* pos, long long* idx, float* zfix,
                           unsigned char* hits, float* zl, float* sl, float* init6, int n, int T, int o, int skip, int fix,
                           int mode, void* stream);
int stove_supair_state_bwd(const float* zc, const long long* idx, const unsigned char* hits, const float* zfix, const float* g_zfix,
                           const float* g_zl, const float* g_sl, const float* g_init6, const float* span_low, float* gfix_ws,
                           float* g_codes, int n, int T, int o, int skip, void* stream);
/* The same with the recursion's whole initial state as output: init (n, o, init_ld) gets the six SuPAIR values in columns 0..5 and,
 * with lat_noise (n, o, lat_dim) standard-normal draws, 0.01 x lat_noise in columns 6.. (stove.py:663-668); the backward reads
 * g_init with the same row stride. */
int stove_supair_state_fwd2(const float* codes, const float* span_low, float* zc, float* pos, long long* idx, float* zfix,
                            unsigned char* hits, float* zl, float* sl, float* init, int init_ld, const float* lat_noise, int lat_dim,
                            int n, int T, int o, int skip, int fix, int mode, void* stream);
int stove_supair_state_bwd2(const float* zc, const long long* idx, const unsigned char* hits, const float* zfix, const float* g_zfix,
                            const float* g_zl, const float* g_sl, const float* g_init6, int init_ld, const float* span_low, float* gfix_ws,
                            float* g_codes, int n, int T, int o, int skip, void* stream);
int stove_zall_fwd(const float* zfix, const float* zs, float* zall, int n, int T, int o, int skip, void* stream);
/* dz_in (NULL = none): the gradient zs receives from its other consumers (the ELBO's log q and transition terms; layout of zs): g_zs = the
 * likelihood's part + dz_in, so that the caller needs no separate accumulation pass. */
int stove_zall_bwd(const float* zfix, const float* zs, const float* g_zall, const float* dz_in, float* g_zfix, float* g_zs, int n, int T, int o,
                   int skip, void* stream);
int stove_elbo_fwd(const float* zs, const float* mean, const float* std_, const float* zdyn, const float* lik, const float* trans_std16,
                   float* part_ws, float* out3, int n, int T, int o, int skip, void* stream);
int stove_elbo_bwd(const float* zs, const float* mean, const float* std_, const float* zdyn, const float* trans_std16, const float* g_out,
                   float* g_zs, float* g_mean, float* g_std, float* g_zdyn, float* g_lik, int n, int T, int o, int skip, void* stream);

/* debug aid of the measurement tools: device buffer of 64 int64 cycle stamps ([4 waves][16 phases]) written by
 * workgroup 0 of the small-graph time loops in their last step; NULL (default) switches it off. */
void stove_debug_set_stamps(long long* device_buffer);
/* debug aid of the tests: the small-graph recursion (2 <= N <= 6) of the following stove_dynloop_fwd / _bwd calls runs the steps
 * [ts0, ts1) only, all tensors keeping their (B, Ts, ...) layout.  Forward: a piece with ts0 > 0 starts from the state the previous
 * piece left in z.  Backward: pieces from the last to the first over the same act and ws; `carry` (B, N, 18 floats on the device)
 * takes the gradient from step ts0 into the state before it (written when ts0 > 0, read when ts1 < Ts); the piece with ts0 == 0
 * writes dz1 and g_params.  ts1 <= 0 (default) = the whole range; a piece outside [0, Ts) makes the calls fail. */
void stove_debug_set_piece(int ts0, int ts1, float* carry);

/* ---- flat parameter arena.  When all model parameters are views into ONE fp32 buffer (and their gradients
 * into one gradient buffer, which is also the data-parallel all-reduce bucket), the SPN tables and the GNN
 * parameter image are baked from / their gradients pushed into those buffers directly:
 *   stove_spn_bake      leaf (a,b,c) from means / sigma_params (rat_torch.py:85-99), softmax of the sum
 *                       weights (rat_torch.py:210), permuted into the kernel order
 *   stove_spn_bake_bwd  the chain rule of the same, ACCUMULATED into grad_arena
 *   stove_arena_gather / _scatter_add   image[i] = arena[src[i]] (src < 0: zero padding) and its adjoint.
 * Offsets are float offsets into the arena; obj_* follow the kernel's leaf / sum order. */
typedef struct StoveSpnArenaPlan {
  const int32_t* obj_mu;    /* [24] */
  const int32_t* obj_rho;   /* [24] */
  const int32_t* obj_sum;   /* [12] */
  const int32_t* bg_mu;     /* [6]  */
  const int32_t* bg_rho;    /* [6]  */
  const int32_t* bg_gidx;   /* [3*1024] leaf*512 + row of pixel p in replica r */
  int32_t obj_root, bg_root;
  float obj_vmin, obj_vmax, bg_vmin, bg_vmax;
} StoveSpnArenaPlan;
int stove_spn_bake(const float* arena, const StoveSpnArenaPlan* plan, float* obj_coef, float* obj_wsum, float* obj_wroot,
                   float* bg_coef, float* bg_wroot, void* stream);
int stove_spn_bake_bwd(const float* arena, const StoveSpnArenaPlan* plan, const StoveSpnTableGrads* g, float* grad_arena, void* stream);
int stove_arena_gather(const float* arena, const int32_t* src, float* image, int n, void* stream);
int stove_arena_scatter_add(const float* gimage, const int32_t* src, float* grad_arena, int n, void* stream);

/* out[j] = sum_c parts[c][j] in chunk order (n a multiple of 4): the split-K partials of the weight-gradient GEMMs. */
int stove_sum_chunks(const float* parts, float* out, size_t n, int chunks, void* stream);

/* ---- auxiliary streams.  Every entry point only enqueues on the stream(s) it is given -- with ONE exception: the scene calls
 * (stove_scene_fwd / _bwd and their variants) run their background-SPN chain next to the object-SPN chain on a per-device FORK stream
 * that the library creates on first use (hipStreamNonBlocking), forks from the call's stream and joins back before the call's last
 * kernel, so the caller sees single-stream semantics (stove_set_overlap(0): no fork at all).  A caller that wants to
 * own that stream -- several models per device, its own capture discipline -- hands it over here: stream != NULL = use this one,
 * NULL = run the chain on the call's stream; restore_default != 0 = back to the library-owned stream.  Thread-safe; takes effect for
 * calls enqueued afterwards.
 * ---- process state.  Everything the library keeps between calls: the fork streams above; the switch below (a measurement
 * aid; the Python binding sets it once from STOVE_NO_OVERLAP, the library itself never reads the environment); the open event list (stove_event_list_*); the profiler at the end of this header. */
int stove_set_fork_stream(int device, void* stream, int restore_default);
/* on = 0: no internal fork stream, every chain of a scene call on the call's stream (default 1). */
int stove_set_overlap(int on);
/* process state, test / measurement switch: which glimpse-tile kernel the scene forward runs -- 1 (default): one lane per glimpse PIXEL with
 * the tile transposed through LDS for up to three objects, one lane per glimpse (the round-5 kernel) beyond; 0: lane per glimpse always;
 * 2: lane per pixel always.  Same numbers bit for bit. */
int stove_set_tile_lds(int mode);
/* ---- stream ordering and graph replay (no reference counterpart: the reference enqueues ~6000 ATen launches per step from Python,
 * train.py:443-473; here a step is ~70 launches that a trainer replays as captured hipGraphs, stove_amd/graphed.py).
 * stove_stream_after: everything enqueued on `to` from now on runs after everything enqueued on `from` so far.  Plain streams: an
 * event record + wait.  Both streams capturing in the SAME capture: the usual fork / join edge.  Capturing in two DIFFERENT captures:
 * an event-record node in `from`'s graph and an event-wait node in `to`'s graph on a persistent event -- the graphs then order
 * against each other at replay, provided the recording graph is launched first.  The *_overlap entry points order their streams
 * with exactly this call, so they may be captured either way.
 * stove_capture_begin / _end: capture what is enqueued on `stream` (relaxed mode) into a graph (n_nodes optional);
 * stove_graph_instantiate: graph -> executable graph (consumes the graph; exec_out NULL-valued for an empty graph);
 * stove_graph_launch / _destroy: replay / free it.
 * stove_event_list_begin / _end / _destroy: who owns the events of the two-capture case.  begin opens a list (one at a time per
 * process) that every such event created from now on is appended to, end closes it (returns the number of events), destroy
 * frees the events -- call it when the graphs that hold their nodes are gone.  Without an open list the events are leaked. */
void* stove_event_list_begin(void);
int stove_event_list_end(void* list);
int stove_event_list_destroy(void* list);
int stove_stream_after(void* to, void* from);
int stove_capture_begin(void* stream);
int stove_capture_end(void* stream, void** graph_out, int* n_nodes);
int stove_graph_instantiate(void* graph, void** exec_out);
int stove_graph_launch(void* exec, void* stream);
int stove_graph_destroy(void* exec);

/* ---- reparameterisation noise (stove.py:667, 679, 146/167): out[0..n) <- standard normal draws, Philox-4x32-10 + Box-Muller, a pure
 * function of (state[0] = seed, state[1] = call number, element index); state: two 64-bit words in DEVICE memory, state[1] is advanced by
 * one behind the draw (a captured launch therefore replays with fresh noise; no host-side generator state).  out 16-byte aligned. */
int stove_noise_normal(float* out, size_t n, unsigned long long* state, void* stream);

/* bw_transform (reference utils.py): x (n_frames, channels, pixels) -> out (n_frames, pixels) = clamp(sum over channels, 0, 1). */
int stove_bw_transform(const float* x, float* out, int n_frames, int channels, int pixels, void* stream);
/* the same from an 8-bit frame store (load_data.py:60-113 keeps float frames on the host; here the training
 * set may live on the device as uint8 = round(255 v)): out = clamp(sum_c (x_c / 255), 0, 1), fp32. */
int stove_bw_transform_u8(const unsigned char* x, float* out, int n_frames, int channels, int pixels, void* stream);

/* out[c] = sum_r a[r][c] of a row-major (rows, cols) matrix, cols a multiple of 4 or <= 64 (bias gradients of the
 * recognition network: 25 600 x 1024, 76 800 x 50, 76 800 x 8); ws: stove_colsum_ws_floats(rows, cols) floats.  Fixed summation order. */
size_t stove_colsum_ws_floats(int rows, int cols);
int stove_colsum(const float* a, float* out, float* ws, int rows, int cols, void* stream);
/* out (M, N) = a^T b over the rows of a (rows, M), b (rows, N), M * N <= 256 (weight gradient of a narrow linear layer over
 * many rows); ws: stove_small_tn_ws_floats floats; fixed summation order. */
size_t stove_small_tn_ws_floats(int rows, int M, int N);
int stove_small_tn(const float* a, const float* b, float* out, float* ws, int rows, int M, int N, void* stream);
/* the same with a second output receiving the same sums (b_ih and b_hh of an LSTM) and accumulate != 0: added to the outputs */
int stove_colsum2(const float* a, float* out, float* out2, int accumulate, float* ws, int rows, int cols, void* stream);

/* One Adam / AMSGrad step of torch.optim.Adam (weight_decay 0; reference train.py:46-49, 431-473) over the flat arena,
 * with clip_grad_norm_(max_norm) folded in (clip != 0: gradients are scaled by min(1, max_norm / (||grads|| + 1e-6)) on the
 * fly; the norm is computed here, in a fixed order, and stored to grad_norm_out if that is not NULL).
 * torch's per-parameter semantics are kept: a SEGMENT is one parameter tensor (each starts on a float4 boundary);
 * seg_of4[i] = segment of floats 4i..4i+3 (numel/4 ints); seg_trainable[s] = requires_grad; seg_steps[s] = steps taken so
 * far (float, advanced here).  A segment steps only if it is trainable and its gradient slice has a non-zero element (what
 * `p.grad is None` means in a flat buffer) and uses ITS step count for the bias corrections; other segments are untouched.
 * ws: stove_flat_adam_ws_bytes(nseg) bytes, zeroed once by the caller before the first call.  max_exp_avg_sq NULL = plain
 * Adam.  hyper_dev != NULL: f32[5] = lr, beta1, beta2, eps, max_norm in device memory override the by-value arguments
 * (captured hipGraphs: kernel arguments are frozen at capture, the learning-rate schedule is not). */
/* clip: bit 0 = clip the gradient to max_norm; bit 1 = "strict zero gradients": a tensor that has once received a gradient keeps
 * stepping while its gradient is all zero (torch.optim.Adam on zero-FILLED .grad tensors, the zero_grad() of the torch 1.0.1 the
 * reference pins); default (bit clear): an all-zero gradient slice means `grad is None` (current torch's zero_grad(set_to_none=True)). */
size_t stove_flat_adam_ws_bytes(int nseg);
int stove_flat_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t numel,
                    const int* seg_of4, const unsigned char* seg_trainable, float* seg_steps, int nseg, void* ws, float* grad_norm_out,
                    const float* hyper_dev, float lr, float beta1, float beta2, float eps, float max_norm, int clip, void* stream);

/* ---- the dense products of RnnStates (encoder.py:43-57: nn.LSTM's x W_ih^T, h W_hh^T, fc1, and their gradients) as fp32
 * GEMMs on the bf16 matrix cores:  C[m][n] = sum_k a(m,k) b(n,k) (+ bias[n]) (+ add[m*ldc + n]),  a(m,k) = A[m*lda + k], or A[k*lda + m] when
 * a_kmajor (the operand is stored K-major, as dg / x are in the weight-gradient products dW = dg^T x); b likewise.
 * nsplit = 2: every fp32 operand element is split on the fly into bf16 hi + lo and the product is three bf16 MFMAs with fp32
 * accumulation (~2^-18 relative per product); nsplit = 3: the same with IEEE-half pieces (~2^-22: an fp32-grade product) for
 * operands inside half's range -- an element keeps max(2^-22 |x|, 2^-25) and must stay below 65504; B, the weights of the forward
 * products, is cut as 2^8 B (floor 2^-33, ceiling 256) and the epilogue shifts back -- K-contiguous, float4-addressable operands
 * only; nsplit = 1: plain bf16 operands (2^-8), fp32 accumulate.  A, B, bias, C stay fp32.
 * splitk > 1: K is cut into `splitk` slices computed by different workgroups into ws (stove_gemm_bf16_ws_floats floats), then
 * summed in slice order into C (needs ldc == N, bias and add NULL): fills the chip when M x N is small and K huge (weight gradients).
 * tile: workgroup tile, 0 = chosen by the library, 1 = 256 x 128 (8 waves), 2 = 128 x 128 (4 waves), 3 = 256 x 256 (8 waves of
 * 64 x 128; needs 136 KB of LDS: one workgroup per CU).
 * Operands / outputs whose leading dimension, contiguous extent or base address is not a multiple of 4 floats (fc1 of the
 * recognition network: 50 columns) are handled element-wise (slow path, meant for small operands); split-K needs an aligned C and
 * takes no add, except add == C (the product is accumulated into C, a gradient view) or, with 2..15 slices, a dense 16-byte aligned
 * M x N add term (added by the slice sum); a bias is allowed with 2..15 slices (added by
 * the slice sum). */
size_t stove_gemm_bf16_ws_floats(int M, int N, int splitk);
int stove_gemm_bf16(const float* A, const float* B, const float* bias, const float* add, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                    int a_kmajor, int b_kmajor, int nsplit, int splitk, int tile, float* ws, void* stream);

/* ---- gate math of RnnStates' LSTM (encoder.py:43-51, torch.nn.LSTM cell, gate order i,f,g,o); the GEMMs
 * around it are stove_gemm_bf16 (or library GEMMs).  gx (n,4H): gate pre-activations -- x W_ih^T + b_ih + b_hh, or already
 * the full sum with the recurrent term (the recurrent GEMM adds gx in its epilogue) and then gh NULL; gh (n,4H): h_prev W_hh^T
 * or NULL; c_prev (n,H) or NULL (zero state).  bwd: dh, dc_in (NULL = 0) -> dg (n,4H) (NULL: not stored), dc_out (n,H);
 * dgx_sum (n,4H) or NULL = dg of this step + the n_more gate gradients dg_more[m][n][4H] of other steps: the gradient of the
 * input projection shared by all steps, formed once (by the last backward step) and feeding dW_ih.
 * fast != 0: sigmoid / tanh on v_exp_f32 / v_rcp_f32 (absolute error ~1e-7) instead of an IEEE division and ocml's tanhf. */
int stove_lstm_cell_fwd(const float* gx, const float* gh, const float* c_prev, float* c, float* h, int n, int H, int fast, void* stream);
int stove_lstm_cell_bwd(const float* gx, const float* gh, const float* c_prev, const float* c, const float* dh,
                        const float* dc_in, float* dg, float* dc_out, float* dgx_sum, const float* dg_more, int n_more, int n, int H,
                        int fast, void* stream);
/* ---- the whole output head of RnnStates in one kernel each way (encoder.py:53-56), csrc/head_fused.hip: fc1, sigmoid and fc2 on the
 * matrix cores; H must be 256, HID <= 64, OUT 8.  fc1_split != 0 (the default path): fc1's forward products as three MFMAs on IEEE-half
 * hi / lo pieces (2^-22 of the value per product, as stove_gemm_bf16 nsplit = 3); 0: on the fp32 MFMA like everything else of the head.
 * fwd: h (rows, H) -> h1 = sigmoid(h W1^T + b1) (rows, HID) and codes (rows, OUT) = h1 W2^T + b2; W1 (HID, H), W2 (OUT, HID).
 * bwd: dcodes (rows, OUT), h1, h -> gh (rows, H) = dL/dh and the parameter gradients gW1 (HID, H), gb1 (HID), gW2 (OUT, HID),
 * gb2 (OUT); accumulate != 0: added to what the four tensors hold (gradient views of a flat arena).  ws:
 * stove_enc_head_bwd_ws_floats floats.  Fixed summation order.  frames > 0: h, h1, gh are step-major (row = step * frames + frame,
 * as the LSTM writes them) while codes / dcodes are frame-major (row = frame * steps + step, encoder.py:57); 0: same row order. */
int stove_enc_head_fwd(const float* h, const float* W1, const float* b1, const float* W2, const float* b2, float* h1, float* codes, int rows,
                       int H, int HID, int OUT, int frames, int fc1_split, void* stream);
size_t stove_enc_head_bwd_ws_floats(int rows, int HID);
int stove_enc_head_bwd(const float* dcodes, const float* h1, const float* h, const float* W1, const float* W2, float* gh, float* gW1,
                       float* gb1, float* gW2, float* gb2, int accumulate, float* ws, int rows, int H, int HID, int OUT, int frames, void* stream);

/* ---- measurement hooks (bench.py): when enabled, every kernel launch of this library is bracketed by
 * two HIP events recorded on the launch stream.  stove_profile_report() synchronises them, writes
 * "kernel\ttotal_ms\tcount\twall_ms\n" lines into buf (wall_ms: the time the kernel's launches cover -- less than their sum
 * where launches on two streams overlap) and clears the records; returns the bytes needed.
 * This is the only process-global state of the library and it is off by default. */
void stove_profile_enable(int on);
size_t stove_profile_report(char* buf, size_t cap);

/* test / debugging utility: n_words 32-bit words at p <- value (tests poison a captured step's memory between replays) */
int stove_fill_words(void* p, uint32_t value, size_t n_words, void* stream);

/* self-test hooks used by tests/ (wave reduction) */
int stove_selftest_wave_sum(const float* in, float* out, int n_waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STOVE_HIP_H */
