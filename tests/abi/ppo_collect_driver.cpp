// Host-only driver of the PPO arm's collection (stove_amd/csrc/ppo_policy.h, the text the kernel of ppo_collect.hip runs) and of
// stove_ppo_collect's argument check (stove_amd/csrc/validate.h: ppo_collect), built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_ppo_cpu.py.
//   ppo_collect_driver validate      every documented bad argument; one line per failure, exit status = number of failures
//   ppo_collect_driver status        a NaN weight: every environment status 3 and nothing written; an infinite velocity in one environment
//                                    of three: that one status 3 and untouched, its neighbours as in a clean run; as above
//   ppo_collect_driver run IN OUT    IN:  int32 B, S, N, H, deep, granularity, drift; double hw, t, friction, action_force, discount;
//                                         double x[B][N][2], v[B][N][2], r[B][N], m[B][N]; float params[param_floats]; float u[B][S]
//                                    OUT: float obs[B][S+1][4N]; int32 actions[B][S]; float rewards, values, logp [B][S]; float
//                                         next_value[B]; float returns[B][S]; int32 status[B]; double x, v [B][N][2]; double margin[B]
// Every environment's rows, the image and every row of the table live in a heap block of exactly their length, so the sanitizer sees
// any index past them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/ppo_policy.h"
#include "driver.h"

static void validate() {
  const double* d = dev<const double>(1);
  const float* f = dev<const float>(2);
  const int* i = dev<const int>(3);
  const double* nd = nullptr;
  const float* nf = nullptr;
  const int* ni = nullptr;
  // (x, v, r, m, params, u, obs, actions, rewards, values, logp, next_value, returns, status, B, S, N, H, granularity)
  auto call = [&](int B, int S, int N, int H, int gran) {
    return stove_validate::ppo_collect(d, d, d, d, f, f, f, i, f, f, f, f, f, i, B, S, N, H, gran);
  };
  expect("ok", call(32, 128, 3, 64, 2), 0);
  expect("ok at N = 1, H = 1", call(1, 1, 1, 1, 1), 0);
  expect("ok at N = 6, H = 128", call(256, 128, 6, 128, 50), 0);
  expect("B = 0 (an empty batch has no arrays)",
         stove_validate::ppo_collect(nd, nd, nd, nd, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 128, 3, 64, 5), 0);
  expect("S = 0 (no table, no step rows)", stove_validate::ppo_collect(d, d, d, d, f, nf, f, ni, nf, nf, nf, f, nf, i, 4, 0, 3, 64, 5), 0);
  for (int k = 0; k < 14; ++k) {
    const double* dd[4] = {d, d, d, d};
    const float* ff[8] = {f, f, f, f, f, f, f, f};        // params, u, obs, rewards, values, logp, next_value, returns
    const int* ii[2] = {i, i};                            // actions, status
    if (k < 4) dd[k] = nd;
    else if (k < 12) ff[k - 4] = nf;
    else ii[k - 12] = ni;
    expect("a NULL array", stove_validate::ppo_collect(dd[0], dd[1], dd[2], dd[3], ff[0], ff[1], ff[2], ii[0], ff[3], ff[4], ff[5], ff[6], ff[7],
                                                       ii[1], 3, 5, 3, 64, 5), 1);
  }
  expect("B = -1", call(-1, 5, 3, 64, 5), 1);
  expect("S = -1", call(3, -1, 3, 64, 5), 1);
  expect("N = 0", call(3, 5, 0, 64, 5), 1);
  expect("N = 7", call(3, 5, 7, 64, 5), 1);
  expect("H = 0", call(3, 5, 3, 0, 5), 1);
  expect("H = 129", call(3, 5, 3, 129, 5), 1);
  expect("granularity = 0", call(3, 5, 3, 64, 0), 1);
  expect("N = 7 at B = 0", stove_validate::ppo_collect(nd, nd, nd, nd, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 5, 7, 64, 5), 1);
  expect("B (S + 1) 4N past int", call(1 << 20, 1 << 10, 6, 64, 5), 1);
}

// one environment's rows, each vector of exactly its length
struct OneEnv {
  std::vector<double> x, v, r, m;
  std::vector<float> u, obs, rewards, values, logp, returns;
  std::vector<int32_t> actions;
  float next_value = 0.0f;
  int32_t status = 0;
  double margin = INFINITY;
  void room(int N, int S) {
    obs.assign((size_t)(S + 1) * 4 * N, 0.0f);
    for (auto* a : {&rewards, &values, &logp, &returns}) a->assign((size_t)S, 0.0f);
    actions.assign((size_t)S, 0);
  }
  bool rows_equal(const OneEnv& o) const {
    auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
      return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
    };
    auto samed = [](const std::vector<double>& a, const std::vector<double>& b) {
      return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
    };
    return same(obs, o.obs) && same(rewards, o.rewards) && same(values, o.values) && same(logp, o.logp) && same(returns, o.returns) &&
           actions == o.actions && std::memcmp(&next_value, &o.next_value, sizeof(float)) == 0 && status == o.status && samed(x, o.x) &&
           samed(v, o.v);
  }
};

struct Batch {
  env_step::Params p;
  ppo_policy::Shape sh;
  int S;
  float discount;
  std::vector<float> params;
  std::vector<OneEnv> envs;
  void collect() {
    for (OneEnv& e : envs)
      e.status = ppo_policy::collect(e.x.data(), e.v.data(), e.r.data(), e.m.data(), p, params.data(), sh, e.u.data(), discount, S, e.obs.data(),
                                     e.actions.data(), e.rewards.data(), e.values.data(), e.logp.data(), &e.next_value, e.returns.data(),
                                     &e.margin);
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head;
  std::vector<double> scal;
  bool ok = read_n(in, head, 7) && read_n(in, scal, 5);
  const int B = ok ? head[0] : 0, S = ok ? head[1] : 0, N = ok ? head[2] : 0, H = ok ? head[3] : 0;
  ok = ok && B >= 1 && S >= 0 && N >= 1 && N <= env_step::kMaxObjects && H >= 1 && H <= ppo_policy::kMaxHidden && head[5] >= 1;
  Batch b;
  if (ok) {
    b.p = env_step::Params{N, head[5], head[6] != 0 ? 1 : 0, scal[0], scal[1], scal[2], scal[3]};
    b.sh = ppo_policy::Shape{N, H, head[4] != 0 ? 1 : 0};
    b.S = S;
    b.discount = (float)scal[4];
    b.envs.resize((size_t)B);
    for (OneEnv& e : b.envs) ok = ok && read_n(in, e.x, 2 * (size_t)N);
    for (OneEnv& e : b.envs) ok = ok && read_n(in, e.v, 2 * (size_t)N);
    for (OneEnv& e : b.envs) ok = ok && read_n(in, e.r, (size_t)N);
    for (OneEnv& e : b.envs) ok = ok && read_n(in, e.m, (size_t)N);
    ok = ok && read_n(in, b.params, ppo_policy::param_floats(b.sh));
    for (OneEnv& e : b.envs) {
      ok = ok && read_n(in, e.u, (size_t)S);
      e.room(N, S);
    }
  }
  std::fclose(in);
  if (!ok) return 2;
  b.collect();
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.obs);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.actions);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.rewards);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.values);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.logp);
  std::vector<float> nv;
  std::vector<int32_t> status;
  std::vector<double> margins;
  for (const OneEnv& e : b.envs) {
    nv.push_back(e.next_value);
    status.push_back(e.status);
    margins.push_back(e.margin);
  }
  ok = ok && write_v(out, nv);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.returns);
  ok = ok && write_v(out, status);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.x);
  for (const OneEnv& e : b.envs) ok = ok && write_v(out, e.v);
  ok = ok && write_v(out, margins);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// three environments of three balls under a small seeded policy (a linear congruential generator; the actor head larger)
static Batch three(int H, int deep, int S) {
  const int N = 3;
  Batch b;
  b.p = env_step::Params{N, 5, 0, 10.0, 1.0, 0.0, 0.6};
  b.sh = ppo_policy::Shape{N, H, deep};
  b.S = S;
  b.discount = 0.95f;
  uint32_t s = 2024u;
  auto next = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) / 16777216.0f;          // [0, 1)
  };
  b.params.resize(ppo_policy::param_floats(b.sh));
  const size_t heads = ppo_policy::offset(b.sh, ppo_policy::layers(b.sh) - 1);
  for (size_t k = 0; k < b.params.size(); ++k) b.params[k] = (next() - 0.5f) * (k >= heads ? 1.5f : 0.25f);
  for (int e = 0; e < 3; ++e) {
    OneEnv env;
    env.x = {3.0, 3.0, 4.5 + 0.3 * e, 3.2, 7.0, 7.5 - 0.4 * e};
    env.v = {0.0, 0.0, -0.4, 0.1, 0.3, -0.2};
    env.r = {1.0, 1.0, 1.0};
    env.m = {10000.0, 1.0, 1.0};
    for (int t = 0; t < S; ++t) env.u.push_back(next());
    env.room(N, S);
    b.envs.push_back(env);
  }
  return b;
}

static void status() {
  for (int deep = 0; deep < 2; ++deep) {
    const int S = 12, H = deep ? 40 : 64;
    const Batch start = three(H, deep, S);
    Batch clean = start;
    clean.collect();
    bool acted = false;
    for (const OneEnv& e : clean.envs) {
      expect("premise: the clean run collects", e.status, 0);
      for (int a : e.actions) acted = acted || a != e.actions[0];
    }
    expect("premise: the draw matters (more than one action drawn)", !acted, 0);
    expect("premise: the environments differ", clean.envs[0].rows_equal(clean.envs[1]), 0);
    // ---- a NaN weight (in the first layer, then in the heads' bias): every environment status 3, nothing written
    for (int where = 0; where < 2; ++where) {
      Batch bad = start;
      bad.params[where == 0 ? 5 : bad.params.size() - 1] = NAN;
      bad.collect();
      for (size_t e = 0; e < 3; ++e) {
        OneEnv want = start.envs[e];
        want.status = ppo_policy::kNonFinite;
        expect("a NaN weight: status 3 and nothing written", !bad.envs[e].rows_equal(want), 0);
      }
    }
    // ---- an infinite velocity of ball 1 in environment 1: status 3 at step 0, untouched; the neighbours as in the clean run
    {
      Batch bad = start;
      bad.envs[1].v[2] = INFINITY;
      bad.collect();
      OneEnv want = start.envs[1];
      want.v[2] = INFINITY;
      want.status = ppo_policy::kNonFinite;
      expect("an infinite observation: status 3 and nothing written", !bad.envs[1].rows_equal(want), 0);
      expect("its neighbours equal the clean run", !bad.envs[0].rows_equal(clean.envs[0]) || !bad.envs[2].rows_equal(clean.envs[2]), 0);
    }
    // ---- S = 0: the observation, next_value and status only
    {
      Batch none = three(H, deep, 0);
      none.collect();
      float o[12], a[ppo_policy::kMaxWidth], b2[ppo_policy::kMaxWidth], heads[ppo_policy::kHeads];
      for (int k = 0; k < 12; ++k) o[k] = ppo_policy::observe(none.envs[0].x.data(), none.envs[0].v.data(), k);
      ppo_policy::forward(none.params.data(), none.sh, o, a, b2, heads);
      expect("S = 0 collects", none.envs[0].status, 0);
      expect("S = 0: next_value is the value at the start", std::memcmp(&none.envs[0].next_value, &heads[0], sizeof(float)) != 0, 0);
      expect("S = 0: obs[0] is written", std::memcmp(none.envs[0].obs.data(), o, sizeof(o)) != 0, 0);
    }
  }
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"status", status}}, run); }
