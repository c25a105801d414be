// Host-only driver of the PPO arm's collection on images (stove_amd/csrc/ppo_image.h, the text the kernel of ppo_image.hip runs) and of
// stove_ppo_collect_images' argument check (stove_amd/csrc/validate.h: ppo_collect_images), built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_ppo_image_cpu.py.
//   ppo_image_driver validate      every documented bad argument; one line per failure, exit status = number of failures
//   ppo_image_driver run IN OUT    IN:  int32 B, S, N, F, H, deep, warm, granularity, drift, use_colors; double hw, t, friction,
//                                       action_force, discount; double x[B][N][2], v[B][N][2], r[B][N], m[B][N]; float params[param_floats];
//                                       float u[B][S]
//                                  OUT: float frames[B][F+S][3][32][32]; int32 actions[B][S]; float rewards, values, logp [B][S]; float
//                                       next_value[B]; float returns[B][S]; int32 status[B]; double x, v [B][N][2]; double margin[B]
// Every environment's rows, the image, the working room and every row of the table live in a heap block of their own, so the sanitizer
// sees any index past them; every output row is filled with NaN / -77 before the call and sits between kGuard elements of that fill,
// which must still hold it afterwards (exit status 3 otherwise).  What a stopped environment leaves unwritten reaches OUT as that fill.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../stove_amd/csrc/ppo_image.h"
#include "driver.h"

static void validate() {
  const double* d = dev<const double>(1);
  const float* f = dev<const float>(2);
  const int* i = dev<const int>(3);
  const double* nd = nullptr;
  const float* nf = nullptr;
  const int* ni = nullptr;
  // (x, v, r, m, params, u, frames, actions, rewards, values, logp, next_value, returns, status, B, S, N, F, H, warm, granularity)
  auto call = [&](int B, int S, int N, int F, int H, int warm, int gran) {
    return stove_validate::ppo_collect_images(d, d, d, d, f, f, f, i, f, f, f, f, f, i, B, S, N, F, H, warm, gran);
  };
  expect("ok", call(32, 128, 3, 4, 512, 4, 2), 0);
  expect("ok at N = 1, F = 1, H = 1, warm = 1", call(1, 1, 1, 1, 1, 1, 1), 0);
  expect("ok at N = 6, F = 4, H = 512", call(256, 128, 6, 4, 512, 9, 50), 0);
  expect("B = 0 (an empty batch has no arrays)",
         stove_validate::ppo_collect_images(nd, nd, nd, nd, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 128, 3, 4, 64, 4, 5), 0);
  expect("S = 0 (no table, no step rows)",
         stove_validate::ppo_collect_images(d, d, d, d, f, nf, f, ni, nf, nf, nf, f, nf, i, 4, 0, 3, 4, 64, 4, 5), 0);
  for (int k = 0; k < 14; ++k) {
    const double* dd[4] = {d, d, d, d};
    const float* ff[8] = {f, f, f, f, f, f, f, f};        // params, u, frames, rewards, values, logp, next_value, returns
    const int* ii[2] = {i, i};                            // actions, status
    if (k < 4) dd[k] = nd;
    else if (k < 12) ff[k - 4] = nf;
    else ii[k - 12] = ni;
    expect("a NULL array", stove_validate::ppo_collect_images(dd[0], dd[1], dd[2], dd[3], ff[0], ff[1], ff[2], ii[0], ff[3], ff[4], ff[5], ff[6],
                                                              ff[7], ii[1], 3, 5, 3, 4, 64, 4, 5), 1);
  }
  expect("B = -1", call(-1, 5, 3, 4, 64, 4, 5), 1);
  expect("S = -1", call(3, -1, 3, 4, 64, 4, 5), 1);
  expect("N = 0", call(3, 5, 0, 4, 64, 4, 5), 1);
  expect("N = 7", call(3, 5, 7, 4, 64, 4, 5), 1);
  expect("F = 0", call(3, 5, 3, 0, 64, 4, 5), 1);
  expect("F = 5", call(3, 5, 3, 5, 64, 4, 5), 1);
  expect("H = 0", call(3, 5, 3, 4, 0, 4, 5), 1);
  expect("H = 513", call(3, 5, 3, 4, 513, 4, 5), 1);
  expect("warm = 0", call(3, 5, 3, 4, 64, 0, 5), 1);
  expect("granularity = 0", call(3, 5, 3, 4, 64, 4, 0), 1);
  expect("F = 5 at B = 0", stove_validate::ppo_collect_images(nd, nd, nd, nd, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 5, 3, 5, 64, 4, 5), 1);
  expect("B (F + S) past int", call(1 << 20, 1 << 12, 3, 4, 64, 4, 5), 1);
  check("the image's length", ppo_image::param_floats(ppo_image::Shape{4, 512, 0}) == (size_t)(193 * 32 + 289 * 32 + 1569 * 512 + 513 * 10));
  check("the ranges", !ppo_image::served(ppo_image::Shape{0, 64, 0}) && !ppo_image::served(ppo_image::Shape{5, 64, 0}) &&
                          !ppo_image::served(ppo_image::Shape{4, 0, 0}) && !ppo_image::served(ppo_image::Shape{4, 513, 0}) &&
                          ppo_image::served(ppo_image::Shape{1, 1, 1}) && ppo_image::served(ppo_image::Shape{4, 512, 1}));
}

constexpr size_t kGuard = 16;
constexpr int32_t kIntFill = -77;

// an output row between two guards, everything filled alike
template <typename T>
struct Guarded {
  std::vector<T> all;
  size_t n = 0;
  T fill() const {
    if constexpr (std::is_integral<T>::value) return (T)kIntFill;
    else return (T)NAN;
  }
  void room(size_t count) {
    n = count;
    all.assign(count + 2 * kGuard, fill());
  }
  T* data() { return all.data() + kGuard; }
  bool intact() const {
    const T f = fill();
    for (size_t k = 0; k < kGuard; ++k)
      if (std::memcmp(&all[k], &f, sizeof(T)) != 0 || std::memcmp(&all[kGuard + n + k], &f, sizeof(T)) != 0) return false;
    return true;
  }
  bool write(std::FILE* out) const { return n == 0 || std::fwrite(all.data() + kGuard, sizeof(T), n, out) == n; }
};

struct OneEnv {
  std::vector<double> x, v, r, m;
  std::vector<float> u;
  Guarded<float> frames, rewards, values, logp, returns, next_value;
  Guarded<int32_t> actions;
  int32_t status = 0;
  double margin = INFINITY;
  void room(int F, int S) {
    frames.room((size_t)(F + S) * ppo_image::kFrameFloats);
    for (auto* a : {&rewards, &values, &logp, &returns}) a->room((size_t)S);
    next_value.room(1);
    actions.room((size_t)S);
  }
  bool intact() const {
    return frames.intact() && rewards.intact() && values.intact() && logp.intact() && returns.intact() && next_value.intact() && actions.intact();
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head;
  std::vector<double> scal;
  bool ok = read_n(in, head, 10) && read_n(in, scal, 5);
  const int B = ok ? head[0] : 0, S = ok ? head[1] : 0, N = ok ? head[2] : 0, F = ok ? head[3] : 0, H = ok ? head[4] : 0;
  const int warm = ok ? head[6] : 0;
  const ppo_image::Shape sh{F, H, ok && head[5] != 0 ? 1 : 0};
  ok = ok && B >= 1 && S >= 0 && N >= 1 && N <= env_step::kMaxObjects && ppo_image::served(sh) && warm >= 1 && head[7] >= 1;
  std::vector<OneEnv> envs;
  std::vector<float> params;
  env_step::Params p{};
  if (ok) {
    p = env_step::Params{N, head[7], head[8] != 0 ? 1 : 0, scal[0], scal[1], scal[2], scal[3]};
    envs.resize((size_t)B);
    for (OneEnv& e : envs) ok = ok && read_n(in, e.x, 2 * (size_t)N);
    for (OneEnv& e : envs) ok = ok && read_n(in, e.v, 2 * (size_t)N);
    for (OneEnv& e : envs) ok = ok && read_n(in, e.r, (size_t)N);
    for (OneEnv& e : envs) ok = ok && read_n(in, e.m, (size_t)N);
    ok = ok && read_n(in, params, ppo_image::param_floats(sh));
    for (OneEnv& e : envs) {
      ok = ok && read_n(in, e.u, (size_t)S);
      e.room(F, S);
    }
  }
  std::fclose(in);
  if (!ok) return 2;
  {
    // working room of exactly the lengths ppo_image.h names
    std::vector<float> ring((size_t)F * ppo_image::kFrameFloats), c1(ppo_image::kConv1Floats), c2(ppo_image::kFlat), a(ppo_image::kMaxHidden),
        b(ppo_image::kMaxHidden);
    for (OneEnv& e : envs)
      e.status = ppo_image::collect(e.x.data(), e.v.data(), e.r.data(), e.m.data(), p, head[9] != 0 ? 1 : 0, params.data(), sh, e.u.data(),
                                    (float)scal[4], S, warm, ring.data(), c1.data(), c2.data(), a.data(), b.data(), e.frames.data(),
                                    e.actions.data(), e.rewards.data(), e.values.data(), e.logp.data(), e.next_value.data(), e.returns.data(),
                                    &e.margin);
  }
  for (const OneEnv& e : envs)
    if (!e.intact()) {
      std::printf("a guard around an output row was overwritten\n");
      return 3;
    }
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  for (const OneEnv& e : envs) ok = ok && e.frames.write(out);
  for (const OneEnv& e : envs) ok = ok && e.actions.write(out);
  for (const OneEnv& e : envs) ok = ok && e.rewards.write(out);
  for (const OneEnv& e : envs) ok = ok && e.values.write(out);
  for (const OneEnv& e : envs) ok = ok && e.logp.write(out);
  for (const OneEnv& e : envs) ok = ok && e.next_value.write(out);
  for (const OneEnv& e : envs) ok = ok && e.returns.write(out);
  std::vector<int32_t> status;
  std::vector<double> margins;
  for (const OneEnv& e : envs) {
    status.push_back(e.status);
    margins.push_back(e.margin);
  }
  ok = ok && write_v(out, status);
  for (const OneEnv& e : envs) ok = ok && write_v(out, e.x);
  for (const OneEnv& e : envs) ok = ok && write_v(out, e.v);
  ok = ok && write_v(out, margins);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}, run); }
