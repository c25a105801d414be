// Host-only driver of the PPO update (stove_amd/csrc/ppo_update.h, the text the kernel of ppo_update.hip runs) and of
// stove_ppo_update's argument check (stove_amd/csrc/validate.h: ppo_update), built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_ppo_update_cpu.py.
//   ppo_update_driver validate      every documented bad argument; one line per failure, exit status = number of failures
//   ppo_update_driver status        a NaN advantage in a row of step k: status (3, k) and everything as a clean run of max_steps = k left
//                                   it; an index of perm or an action out of range: status (2, k) likewise; empty calls
//   ppo_update_driver run IN OUT    IN:  int32 n, E, M, max_steps, N, H, deep, clipped_value_loss, step; float clip, value_coef,
//                                        entropy_coef, lr, eps, max_grad_norm; float params, m, v [param_floats]; float obs[n][4N];
//                                        int32 actions[n]; float returns, values, logp, adv [n]; int32 perm[E][n]
//                                   OUT: float params, m, v [param_floats]; int32 step, status, done; float losses[E M][3], gnorm[E M]
//                                        (rows of steps not taken keep the poison -77)
// Every array lives in a heap block of exactly its length, so the sanitizer sees any index past it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/ppo_update.h"
#include "driver.h"

static void validate() {
  const float* f = dev<const float>(2);
  const int* i = dev<const int>(3);
  // (params, m, v, step, obs, actions, returns, values, logp, adv, perm, losses, gnorm, status, n, E, M, max_steps, N, H)
  auto call = [&](int n, int E, int M, int max_steps, int N, int H) {
    return stove_validate::ppo_update(f, f, f, i, f, i, f, f, f, f, i, f, f, i, n, E, M, max_steps, N, H);
  };
  expect("ok", call(4096, 4, 32, 128, 3, 64), 0);
  expect("ok at N = 1, H = 1, one row", call(1, 1, 1, 1, 1, 1), 0);
  expect("ok at N = 6, H = 128", call(32768, 4, 32, 128, 6, 128), 0);
  expect("E = 0 is an empty call", call(64, 0, 4, 0, 3, 64), 0);
  expect("max_steps = 0 is an empty call", call(64, 2, 4, 0, 3, 64), 0);
  expect("max_steps below E M", call(64, 2, 4, 5, 3, 64), 0);
  for (int k = 0; k < 14; ++k) {
    const float* ff[10] = {f, f, f, f, f, f, f, f, f, f};        // params, m, v, obs, returns, values, logp, adv, losses, gnorm
    const int* ii[4] = {i, i, i, i};                             // step, actions, perm, status
    if (k < 10) ff[k] = nullptr;
    else ii[k - 10] = nullptr;
    expect("a NULL array", stove_validate::ppo_update(ff[0], ff[1], ff[2], ii[0], ff[3], ii[1], ff[4], ff[5], ff[6], ff[7], ii[2], ff[8], ff[9],
                                                      ii[3], 64, 2, 4, 8, 3, 64), 1);
  }
  expect("n < M", call(3, 2, 4, 8, 3, 64), 1);
  expect("M = 0", call(64, 2, 0, 0, 3, 64), 1);
  expect("E = -1", call(64, -1, 4, 0, 3, 64), 1);
  expect("max_steps = -1", call(64, 2, 4, -1, 3, 64), 1);
  expect("max_steps above E M", call(64, 2, 4, 9, 3, 64), 1);
  expect("N = 0", call(64, 2, 4, 8, 0, 64), 1);
  expect("N = 7", call(64, 2, 4, 8, 7, 64), 1);
  expect("H = 0", call(64, 2, 4, 8, 3, 0), 1);
  expect("H = 129", call(64, 2, 4, 8, 3, 129), 1);
  expect("E n past int", call(1 << 20, 1 << 12, 4, 8, 3, 64), 1);
}

struct Problem {
  int n = 0, E = 0, M = 0, max_steps = 0, step = 0, status = 0, done = 0;
  ppo_policy::Shape sh{1, 1, 0};
  ppo_update::Hyper hy{};
  std::vector<float> params, m, v, obs, returns, values, logp, adv, losses, gnorm;
  std::vector<int32_t> actions, perm;
  void room() {
    losses.assign((size_t)E * M * 3, -77.0f);
    gnorm.assign((size_t)E * M, -77.0f);
  }
  void update() {
    std::vector<float> grad(ppo_policy::param_floats(sh)), row((size_t)ppo_update::row_floats(sh));
    status = ppo_update::update(params.data(), m.data(), v.data(), &step, obs.data(), actions.data(), returns.data(), values.data(), logp.data(),
                                adv.data(), perm.data(), losses.data(), gnorm.data(), n, E, M, max_steps, sh, hy, grad.data(), row.data(), &done);
  }
  bool state_equals(const Problem& o) const {
    auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
      return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
    };
    return same(params, o.params) && same(m, o.m) && same(v, o.v) && step == o.step && same(losses, o.losses) && same(gnorm, o.gnorm);
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head;
  std::vector<float> scal;
  bool ok = read_n(in, head, 9) && read_n(in, scal, 6);
  Problem p;
  if (ok) {
    p.n = head[0], p.E = head[1], p.M = head[2], p.max_steps = head[3], p.step = head[8];
    p.sh = ppo_policy::Shape{head[4], head[5], head[6] != 0 ? 1 : 0};
    p.hy = ppo_update::Hyper{scal[0], scal[1], scal[2], scal[3], scal[4], scal[5], head[7] != 0 ? 1 : 0};
    const float* nf = dev<const float>(2);
    const int* ni = dev<const int>(3);
    ok = stove_validate::ppo_update(nf, nf, nf, ni, nf, ni, nf, nf, nf, nf, ni, nf, nf, ni, p.n, p.E, p.M, p.max_steps, p.sh.N, p.sh.H) == 0;
  }
  if (ok) {
    const size_t P = ppo_policy::param_floats(p.sh), n = (size_t)p.n;
    ok = read_n(in, p.params, P) && read_n(in, p.m, P) && read_n(in, p.v, P) && read_n(in, p.obs, n * 4 * p.sh.N) && read_n(in, p.actions, n) &&
         read_n(in, p.returns, n) && read_n(in, p.values, n) && read_n(in, p.logp, n) && read_n(in, p.adv, n) && read_n(in, p.perm, (size_t)p.E * n);
  }
  std::fclose(in);
  if (!ok) return 2;
  p.room();
  p.update();
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  const std::vector<int32_t> tail = {p.step, p.status, p.done};
  ok = write_v(out, p.params) && write_v(out, p.m) && write_v(out, p.v) && write_v(out, tail) && write_v(out, p.losses) && write_v(out, p.gnorm);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// 22 rows of three balls under a small seeded policy (a linear congruential generator), E = 2, M = 4: mb = 5, two rows dropped
static Problem small(int H, int deep) {
  Problem p;
  p.n = 22, p.E = 2, p.M = 4, p.max_steps = 8;
  p.sh = ppo_policy::Shape{3, H, deep};
  p.hy = ppo_update::Hyper{0.1f, 0.5f, 0.01f, 2e-4f, 1e-5f, 40.0f, 1};
  uint32_t s = 77u;
  auto next = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) / 16777216.0f;          // [0, 1)
  };
  const size_t P = ppo_policy::param_floats(p.sh);
  p.params.resize(P);
  for (size_t k = 0; k < P; ++k) p.params[k] = (next() - 0.5f) * 0.25f;
  p.m.assign(P, 0.0f);
  p.v.assign(P, 0.0f);
  for (int r = 0; r < p.n; ++r) {
    for (int k = 0; k < 12; ++k) p.obs.push_back(next() * 10.0f - (k % 4 >= 2 ? 5.0f : 0.0f));
    p.actions.push_back((int32_t)(next() * 9.0f) % 9);
    p.returns.push_back(next() - 1.0f);
    p.values.push_back(next() * 0.2f - 0.1f);
    p.logp.push_back(-2.2f + 0.1f * (next() - 0.5f));
    p.adv.push_back(p.returns.back() - p.values.back());
  }
  for (int e = 0; e < p.E; ++e)
    for (int r = 0; r < p.n; ++r) p.perm.push_back((r * 7 + 3 + 5 * e) % p.n);          // (7 and 22 are coprime: a permutation)
  p.room();
  return p;
}

static void status() {
  for (int deep = 0; deep < 2; ++deep) {
    const Problem start = small(deep ? 40 : 64, deep);
    Problem clean = start;
    clean.update();
    expect("premise: the clean run completes", clean.status, 0);
    check("premise: all steps taken", clean.done == 8 && clean.step == 8);
    check("premise: the update moves the parameters", std::memcmp(clean.params.data(), start.params.data(), start.params.size() * sizeof(float)) != 0);
    for (int k = 0; k < 8; k += 3) {          // steps 0, 3, 6
      Problem part = start;
      part.max_steps = k;
      part.update();
      check("max_steps = k: status 0, k steps", part.status == 0 && part.done == k && part.step == k);
      for (int at = 0; at < 8; ++at)
        check("max_steps = k: later rows keep the poison", (part.gnorm[at] == -77.0f) == (at >= k) && (part.losses[3 * at] == -77.0f) == (at >= k));
      const int row = start.perm[(size_t)(k / 4) * start.n + (size_t)(k % 4) * 5 + 2];          // a row of step k
      // ---- a NaN advantage: the earliest step holding the row stops the update
      {
        Problem bad = start;
        bad.adv[row] = NAN;
        bad.update();
        int first = 8;
        for (int at = 7; at >= 0; --at)
          for (int r = 0; r < 5; ++r)
            if (start.perm[(size_t)(at / 4) * start.n + (size_t)(at % 4) * 5 + r] == row) first = at;
        Problem want = start;
        want.max_steps = first;
        want.update();
        check("a NaN advantage: status 3 at its step", bad.status == ppo_update::kNonFinite && bad.done == first);
        check("a NaN advantage: everything as the steps before left it", bad.state_equals(want));
      }
      // ---- an index of perm out of range in step k, an action out of range in a row of step k
      for (int which = 0; which < 3; ++which) {
        Problem bad = start;
        if (which == 0) bad.perm[(size_t)(k / 4) * start.n + (size_t)(k % 4) * 5 + 4] = start.n;
        if (which == 1) bad.perm[(size_t)(k / 4) * start.n + (size_t)(k % 4) * 5] = -1;
        if (which == 2 && k >= 4) continue;          // (the row would stop an earlier step too)
        if (which == 2) bad.actions[row] = 9;
        bad.update();
        Problem want = start;
        want.max_steps = k;
        want.update();
        check("an index out of range: status 2 at its step", bad.status == ppo_update::kBadIndex && bad.done == k);
        check("an index out of range: everything as the steps before left it", bad.state_equals(want));
      }
    }
    // ---- the chunked sums are ppo_policy's: the forward with its activations kept puts out what ppo_policy::forward does, bit for bit
    {
      std::vector<float> row((size_t)ppo_update::row_floats(start.sh)), a(ppo_policy::kMaxWidth), b(ppo_policy::kMaxWidth), heads(ppo_policy::kHeads);
      bool same = true;
      for (int r = 0; r < start.n; ++r) {
        ppo_update::forward_keep(start.params.data(), start.sh, start.obs.data() + (size_t)r * 12, row.data());
        ppo_policy::forward(start.params.data(), start.sh, start.obs.data() + (size_t)r * 12, a.data(), b.data(), heads.data());
        same = same && std::memcmp(heads.data(), row.data() + ppo_update::delta_offset(start.sh, ppo_policy::layers(start.sh) - 1),
                                   ppo_policy::kHeads * sizeof(float)) == 0;
      }
      check("forward_keep equals ppo_policy::forward bit for bit", same);
    }
    // ---- the indices an epoch drops are never read
    {
      Problem odd = start;
      odd.perm[20] = 1 << 30;
      odd.perm[21] = -5;
      odd.update();
      check("the trailing n - M mb indices are never read", odd.status == 0 && odd.state_equals(clean));
    }
    // ---- E = 0
    {
      Problem none = start;
      none.E = 0, none.max_steps = 0;
      none.perm.clear();
      none.room();
      none.update();
      check("E = 0: nothing happens", none.status == 0 && none.done == 0 && none.step == 0);
    }
    // ---- the unclipped value loss differs, and both leave finite parameters
    {
      Problem plain = start;
      plain.hy.clipped_value_loss = 0;
      plain.update();
      bool fin = true;
      for (float f : plain.params) fin = fin && std::isfinite(f);
      check("the unclipped value loss runs", plain.status == 0 && fin);
    }
  }
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"status", status}}, run); }
