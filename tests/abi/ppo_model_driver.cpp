// Host-only driver of the model-based PPO arm's policy half (stove_amd/csrc/ppo_policy.h: observe_model, forward, draw -- the text the
// kernel of ppo_model.hip runs between two steps of the model) and of stove_ppo_collect_model's argument check
// (stove_amd/csrc/validate.h: ppo_collect_model), built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_ppo_model_cpu.py.
//   ppo_model_driver validate      every documented bad argument; one line per failure, exit status = number of failures
//   ppo_model_driver run IN OUT    IN:  int32 K, N, H, deep; float hw; float z[K][N][18]; float params[param_floats]; float u[K]
//                                  OUT: float obs[K][4N]; float values[K]; int32 actions[K]; float logp[K]; double margin[K]
// Every state, the image and every observation row live in a heap block of exactly their length, so the sanitizer sees any index
// past them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../stove_amd/csrc/ppo_policy.h"
#include "driver.h"

static void validate() {
  const float* f = dev<const float>(2);
  const int* i = dev<const int>(3);
  const float* nf = nullptr;
  const int* ni = nullptr;
  // (z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, obs, actions, rewards, values, logp, next_value, returns,
  //  status, B, S, N, H, app_dim, lim_enc)
  auto call = [&](int B, int S, int N, int H, int app_dim, int lim_enc) {
    return stove_validate::ppo_collect_model(f, f, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, B, S, N, H, app_dim, lim_enc);
  };
  expect("ok", call(32, 128, 3, 64, 3, 2), 0);
  expect("ok at N = 1, H = 1, no appearance", stove_validate::ppo_collect_model(f, nf, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, 1, 1, 1, 1, 0, 0), 0);
  expect("ok at N = 6, H = 128, the widest appearance", call(256, 128, 6, 128, 12, 32), 0);
  expect("B = 0 (an empty batch has no arrays)",
         stove_validate::ppo_collect_model(nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 128, 3, 64, 3, 2), 0);
  expect("S = 0 (no table, no step rows)",
         stove_validate::ppo_collect_model(f, f, f, f, f, f, f, nf, nf, f, ni, nf, nf, nf, f, nf, i, 4, 0, 3, 64, 3, 2), 0);
  for (int k = 0; k < 17; ++k) {
    // z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, obs, rewards, values, logp, next_value, returns
    const float* ff[15] = {f, f, f, f, f, f, f, f, f, f, f, f, f, f, f};
    const int* ii[2] = {i, i};                            // actions, status
    if (k < 15) ff[k] = nf;
    else ii[k - 15] = ni;
    expect("a NULL array", stove_validate::ppo_collect_model(ff[0], ff[1], ff[2], ff[3], ff[4], ff[5], ff[6], ff[7], ff[8], ff[9], ii[0], ff[10],
                                                             ff[11], ff[12], ff[13], ff[14], ii[1], 3, 5, 3, 64, 3, 2), 1);
  }
  expect("B = -1", call(-1, 5, 3, 64, 3, 2), 1);
  expect("S = -1", call(3, -1, 3, 64, 3, 2), 1);
  expect("N = 0", call(3, 5, 0, 64, 3, 2), 1);
  expect("N = 7", call(3, 5, 7, 64, 3, 2), 1);
  expect("H = 0", call(3, 5, 3, 0, 3, 2), 1);
  expect("H = 129", call(3, 5, 3, 129, 3, 2), 1);
  expect("app_dim = -1", call(3, 5, 3, 64, -1, 2), 1);
  expect("app_dim = 13 (20 + app_dim past 32)", call(3, 5, 3, 64, 13, 2), 1);
  expect("lim_enc = -1", call(3, 5, 3, 64, 3, -1), 1);
  expect("lim_enc = 33", call(3, 5, 3, 64, 3, 33), 1);
  expect("N = 7 at B = 0", stove_validate::ppo_collect_model(nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 5, 7, 64, 3, 2), 1);
  expect("B (S + 1) N 32 past int", call(1 << 20, 1 << 10, 6, 64, 3, 2), 1);
}

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head;
  std::vector<float> scal, params;
  bool ok = read_n(in, head, 4) && read_n(in, scal, 1);
  const int K = ok ? head[0] : 0, N = ok ? head[1] : 0, H = ok ? head[2] : 0;
  ok = ok && K >= 1 && N >= 1 && N <= env_step::kMaxObjects && H >= 1 && H <= ppo_policy::kMaxHidden;
  if (!ok) {
    std::fclose(in);
    return 2;
  }
  const ppo_policy::Shape sh{N, H, head[3] != 0 ? 1 : 0};
  const float hw = scal[0];
  std::vector<std::vector<float>> z((size_t)K), obs((size_t)K);
  for (auto& row : z) ok = ok && read_n(in, row, (size_t)N * 18);
  ok = ok && read_n(in, params, ppo_policy::param_floats(sh));
  std::vector<float> u;
  ok = ok && read_n(in, u, (size_t)K);
  std::fclose(in);
  if (!ok) return 2;
  std::vector<float> values((size_t)K), logp((size_t)K);
  std::vector<int32_t> actions((size_t)K);
  std::vector<double> margin((size_t)K);
  for (int k = 0; k < K; ++k) {
    std::vector<float> a(ppo_policy::kMaxWidth), b(ppo_policy::kMaxWidth), heads(ppo_policy::kHeads);
    obs[k].resize((size_t)4 * N);
    for (int i = 0; i < N; ++i)
      for (int c = 0; c < 4; ++c) obs[k][4 * i + c] = ppo_policy::observe_model(z[k][(size_t)i * 18 + 2 + c], c, hw);
    ppo_policy::forward(params.data(), sh, obs[k].data(), a.data(), b.data(), heads.data());
    values[k] = heads[0];
    actions[k] = ppo_policy::draw(heads.data() + 1, u[k], &logp[k], &margin[k]);
  }
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  for (const auto& row : obs) ok = ok && write_v(out, row);
  ok = ok && write_v(out, values) && write_v(out, actions) && write_v(out, logp) && write_v(out, margin);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}, run); }
