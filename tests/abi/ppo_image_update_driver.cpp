// Host-only driver of stove_ppo_update_images' argument check (stove_amd/csrc/validate.h: ppo_update_images) and of the rule by which
// the kernels of csrc/ppo_image_update.hip address a row's observation, built with -fsanitize=address,undefined by
// tests/test_ppo_image_update_cpu.py.
//   ppo_image_update_driver validate     every documented bad argument and the empty calls; one line per failure, exit status = failures
//   ppo_image_update_driver windows      row r's 3072 F floats at obs + (r / S) env_stride + (r % S) 3072, read under the sanitizer from a
//                                        frames array of exactly B (F + S) 3072 floats and from a dense one of n 3072 F: the window
//                                        frames[b, s : s + F] of row b S + s, the last row ending on the array's last float
#include "driver.h"

static void validate() {
  const float* f = dev<const float>(2);
  const int* i = dev<const int>(3);
  const void* ws = dev<const void>(4);
  // (params, m, v, step, obs, actions, returns, values, logp, adv, perm, losses, gnorm, status, ws, n, S, env_stride, E, M, max_steps, F, H)
  auto call = [&](int n, int S, int env_stride, int E, int M, int max_steps, int F, int H) {
    return stove_validate::ppo_update_images(f, f, f, i, f, i, f, f, f, f, i, f, f, i, ws, n, S, env_stride, E, M, max_steps, F, H);
  };
  expect("ok", call(4096, 128, 132 * 3072, 4, 32, 128, 4, 512), 0);
  expect("ok, dense", call(70, 1, 3072 * 4, 1, 2, 2, 4, 16), 0);
  expect("ok, one row per step", call(12, 4, 5 * 3072, 1, 12, 12, 1, 1), 0);
  expect("ok, partial", call(64, 1, 3072, 2, 4, 3, 1, 8), 0);
  expect("n < M", call(3, 1, 3072, 2, 4, 8, 1, 8), 1);
  expect("M < 1", call(64, 1, 3072, 2, 0, 0, 1, 8), 1);
  expect("S < 1", call(64, 0, 3072, 2, 4, 8, 1, 8), 1);
  expect("F = 0", call(64, 1, 3072, 2, 4, 8, 0, 8), 1);
  expect("F = 5", call(64, 1, 3072, 2, 4, 8, 5, 8), 1);
  expect("H = 0", call(64, 1, 3072, 2, 4, 8, 1, 0), 1);
  expect("H = 513", call(64, 1, 3072, 2, 4, 8, 1, 513), 1);
  expect("E < 0", call(64, 1, 3072, -1, 4, 0, 1, 8), 1);
  expect("max_steps < 0", call(64, 1, 3072, 2, 4, -1, 1, 8), 1);
  expect("max_steps > E M", call(64, 1, 3072, 2, 4, 9, 1, 8), 1);
  expect("env_stride < 0", call(64, 1, -3072, 2, 4, 8, 1, 8), 1);
  expect("E n overflows", call(1 << 20, 1, 3072, 1 << 12, 4, 8, 1, 8), 1);
  const float* ff[10] = {f, f, f, f, f, f, f, f, f, f};
  const int* ii[4] = {i, i, i, i};
  for (int k = 0; k < 15; ++k) {
    const float* a[10];
    const int* b[4];
    for (int q = 0; q < 10; ++q) a[q] = ff[q];
    for (int q = 0; q < 4; ++q) b[q] = ii[q];
    const void* w = ws;
    if (k < 10) a[k] = nullptr;
    else if (k < 14) b[k - 10] = nullptr;
    else w = nullptr;
    expect("a NULL array", stove_validate::ppo_update_images(a[0], a[1], a[2], b[0], a[3], b[1], a[4], a[5], a[6], a[7], b[2], a[8], a[9], b[3], w,
                                                             64, 1, 3072, 2, 4, 8, 1, 8), 1);
  }
  // the empty calls: only status is needed
  const float* nf = nullptr;
  const int* ni = nullptr;
  expect("E = 0", stove_validate::ppo_update_images(nf, nf, nf, ni, nf, ni, nf, nf, nf, nf, ni, nf, nf, i, nullptr, 64, 1, 3072, 0, 4, 0, 1, 8), 0);
  expect("max_steps = 0", stove_validate::ppo_update_images(nf, nf, nf, ni, nf, ni, nf, nf, nf, nf, ni, nf, nf, i, nullptr, 64, 1, 3072, 2, 4, 0, 1, 8),
         0);
  expect("an empty call without status", stove_validate::ppo_update_images(nf, nf, nf, ni, nf, ni, nf, nf, nf, nf, ni, nf, nf, ni, nullptr, 64, 1, 3072,
                                                                           0, 4, 0, 1, 8), 1);
}

static const float* window(const float* obs, int r, int S, int env_stride) {
  return obs + (size_t)(r / S) * (size_t)env_stride + (size_t)(r % S) * 3072;
}

static void windows() {
  for (int F = 1; F <= 4; ++F) {
    const int B = 3, S = 5, R = F + S;
    std::vector<float> frames((size_t)B * R * 3072);          // (exactly: a read past the last window is a sanitizer report)
    for (size_t k = 0; k < frames.size(); ++k) frames[k] = (float)(k % 8191) + 0.5f * (float)(k / 8191);
    std::vector<float> dense((size_t)B * S * F * 3072);
    bool same = true;
    for (int r = 0; r < B * S; ++r) {
      const int b = r / S, s = r % S;
      const float* w = window(frames.data(), r, S, R * 3072);
      for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3072; ++k) {
          same = same && w[f * 3072 + k] == frames[((size_t)b * R + s + f) * 3072 + k];
          dense[((size_t)r * F + f) * 3072 + k] = w[f * 3072 + k];
        }
    }
    check("a row's window is frames[b, s : s + F]", same);
    bool again = true;
    for (int r = 0; r < B * S; ++r) {
      const float* w = window(dense.data(), r, 1, F * 3072);
      for (int k = 0; k < F * 3072; ++k) again = again && w[k] == window(frames.data(), r, S, R * 3072)[k];
    }
    check("the dense layout is S = 1, env_stride = 3072 F", again);
  }
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"windows", windows}}); }
