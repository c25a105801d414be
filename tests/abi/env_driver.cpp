// Host-only driver of the environment step (stove_amd/csrc/env_step.h, the text the kernel of env.hip runs) and of stove_env_step's
// argument check (stove_amd/csrc/validate.h: env_step), built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_env_batched_cpu.py.
//   env_driver validate          every documented bad argument; one line per failure, exit status = number of failures
//   env_driver status            an action index outside [0, 9): status 2, the environment untouched, its neighbours stepped; as above
//   env_driver run IN OUT        IN:  int32 M, N, granularity, drift, acting, steps, res, use_colors; double hw, t, friction, action_force;
//                                     double x[M][N][2], v[M][N][2], r[M][N], m[M][N]; int32 action[steps][M] (if acting)
//                                OUT: double x[steps][M][N][2], v[steps][M][N][2]; int32 collisions[steps][M], status[steps][M];
//                                     float frame[M][3][res][res] of the final state
// `run` steps every environment `steps` times as the kernel does: rows copied out, stepped, written back unless the status is 2.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/env_step.h"
#include "driver.h"

static void validate() {
  using stove_validate::env_step;
  const double* d = dev<const double>(1);
  const int* i = dev<const int>(2);
  const double* nd = nullptr;
  const int* ni = nullptr;
  // (x, v, r, m, collisions, status, M, N, granularity, res)
  expect("ok", env_step(d, d, d, d, i, i, 100, 3, 5, 32), 0);
  expect("ok at N = 1, granularity 1, res 1", env_step(d, d, d, d, i, i, 1, 1, 1, 1), 0);
  expect("ok at N = 6, res 50", env_step(d, d, d, d, i, i, 65, 6, 50, 50), 0);
  expect("M = 0 (an empty batch has no arrays)", env_step(nd, nd, nd, nd, ni, ni, 0, 3, 5, 32), 0);
  expect("NULL x", env_step(nd, d, d, d, i, i, 3, 3, 5, 32), 1);
  expect("NULL v", env_step(d, nd, d, d, i, i, 3, 3, 5, 32), 1);
  expect("NULL r", env_step(d, d, nd, d, i, i, 3, 3, 5, 32), 1);
  expect("NULL m", env_step(d, d, d, nd, i, i, 3, 3, 5, 32), 1);
  expect("NULL collisions", env_step(d, d, d, d, ni, i, 3, 3, 5, 32), 1);
  expect("NULL status", env_step(d, d, d, d, i, ni, 3, 3, 5, 32), 1);
  expect("M = -1", env_step(d, d, d, d, i, i, -1, 3, 5, 32), 1);
  expect("N = 0", env_step(d, d, d, d, i, i, 3, 0, 5, 32), 1);
  expect("N = 7", env_step(d, d, d, d, i, i, 3, 7, 5, 32), 1);
  expect("N = 0 at M = 0", env_step(nd, nd, nd, nd, ni, ni, 0, 0, 5, 32), 1);
  expect("granularity = 0", env_step(d, d, d, d, i, i, 3, 3, 0, 32), 1);
  expect("granularity = -5", env_step(d, d, d, d, i, i, 3, 3, -5, 32), 1);
  expect("res = 0", env_step(d, d, d, d, i, i, 3, 3, 5, 0), 1);
  expect("res = -32", env_step(d, d, d, d, i, i, 3, 3, 5, -32), 1);
}

// M environments' rows and the per-environment body of env_step_k
struct Batch {
  int M;
  env_step::Params p;
  std::vector<double> x, v, r, m;
  std::vector<int32_t> collisions, status;
  // action (M,) or NULL
  void step(const int32_t* action) {
    const int N = p.N;
    for (int e = 0; e < M; ++e) {
      std::vector<double> sx(x.begin() + (size_t)e * 2 * N, x.begin() + (size_t)(e + 1) * 2 * N);      // exactly 2 N long: the sanitizer
      std::vector<double> sv(v.begin() + (size_t)e * 2 * N, v.begin() + (size_t)(e + 1) * 2 * N);      // sees any index past the rows
      std::vector<double> sr(r.begin() + (size_t)e * N, r.begin() + (size_t)(e + 1) * N);
      std::vector<double> sm(m.begin() + (size_t)e * N, m.begin() + (size_t)(e + 1) * N);
      int hit = 0;
      const int s = env_step::step(sx.data(), sv.data(), sr.data(), sm.data(), p, action != nullptr ? action + e : nullptr, &hit);
      if (s == env_step::kOk) {
        std::copy(sx.begin(), sx.end(), x.begin() + (size_t)e * 2 * N);
        std::copy(sv.begin(), sv.end(), v.begin() + (size_t)e * 2 * N);
        collisions[e] = hit;
      }
      status[e] = s;
    }
  }
  std::vector<float> frames(int res, int use_colors) const {
    const int N = p.N;
    const size_t plane = (size_t)res * res;
    std::vector<float> out((size_t)M * 3 * plane);
    for (int e = 0; e < M; ++e)
      for (size_t px = 0; px < plane; ++px) {
        const int a = (int)(px / res), b = (int)(px % res);
        float rgb[3];
        env_step::pixel(x.data() + (size_t)e * 2 * N, r.data() + (size_t)e * N, N, use_colors, env_step::centre(b, res, p.hw),
                        env_step::centre(a, res, p.hw), rgb);
        for (int ch = 0; ch < 3; ++ch) out[((size_t)e * 3 + ch) * plane + px] = rgb[ch];
      }
    return out;
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head, action;
  std::vector<double> scal;
  Batch b;
  bool ok = read_n(in, head, 8) && read_n(in, scal, 4);
  const int M = ok ? head[0] : 0, N = ok ? head[1] : 0, gran = ok ? head[2] : 0, acting = ok ? head[4] : 0, steps = ok ? head[5] : 0;
  const int res = ok ? head[6] : 0, use_colors = ok ? head[7] : 0;
  ok = ok && M >= 1 && N >= 1 && N <= env_step::kMaxObjects && gran >= 1 && steps >= 0 && res >= 1 && res <= 256;
  if (ok) {
    b.M = M;
    b.p = env_step::Params{N, gran, head[3] != 0 ? 1 : 0, scal[0], scal[1], scal[2], scal[3]};
    ok = read_n(in, b.x, (size_t)M * N * 2) && read_n(in, b.v, (size_t)M * N * 2) && read_n(in, b.r, (size_t)M * N) &&
         read_n(in, b.m, (size_t)M * N) && (!acting || read_n(in, action, (size_t)steps * M));
  }
  std::fclose(in);
  if (!ok) return 2;
  b.collisions.assign((size_t)M, 0);
  b.status.assign((size_t)M, 0);
  std::vector<double> xs, vs;
  std::vector<int32_t> cs, ss;
  for (int s = 0; s < steps; ++s) {
    b.step(acting ? action.data() + (size_t)s * M : nullptr);
    xs.insert(xs.end(), b.x.begin(), b.x.end());
    vs.insert(vs.end(), b.v.begin(), b.v.end());
    cs.insert(cs.end(), b.collisions.begin(), b.collisions.end());
    ss.insert(ss.end(), b.status.begin(), b.status.end());
  }
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  ok = write_v(out, xs) && write_v(out, vs) && write_v(out, cs) && write_v(out, ss) && write_v(out, b.frames(res, use_colors));
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// Three environments, the same state in 0 and 2; environment 1 gets an action index of 9, then of -1: status [0, 2, 0], environment 1
// exactly as handed over (x, v, and its collisions entry), 0 and 2 as in a run where all three actions were fine.
static void status() {
  const int M = 3, N = 3;
  Batch b;
  b.M = M;
  b.p = env_step::Params{N, 5, 0, 10.0, 1.0, 0.0, 0.6};
  const double x0[N * 2] = {3.0, 3.0, 4.5, 3.2, 7.0, 7.5}, v0[N * 2] = {0.0, 0.0, -0.4, 0.1, 0.3, -0.2};
  for (int e = 0; e < M; ++e) {
    b.x.insert(b.x.end(), x0, x0 + N * 2);
    b.v.insert(b.v.end(), v0, v0 + N * 2);
    for (int i = 0; i < N; ++i) {
      b.r.push_back(1.0);
      b.m.push_back(i == 0 ? 10000.0 : 1.0);
    }
  }
  b.x[2 * N] = 6.0;                                 // environment 1 is another one
  b.collisions.assign((size_t)M, -7);
  b.status.assign((size_t)M, -7);
  Batch clean = b;
  const int32_t good[M] = {1, 3, 1};
  clean.step(good);
  for (int32_t bad : {9, -1, 1 << 30}) {
    Batch t = b;
    const int32_t acts[M] = {1, bad, 1};
    t.step(acts);
    expect("status of environment 0", t.status[0], 0);
    expect("status 2", t.status[1] != env_step::kBadAction, 0);
    expect("status of environment 2", t.status[2], 0);
    expect("collisions entry of the refused environment is not written", t.collisions[1] != -7, 0);
    expect("the refused environment is left as handed over",
           std::memcmp(t.x.data() + 2 * N, b.x.data() + 2 * N, 2 * N * sizeof(double)) != 0 ||
               std::memcmp(t.v.data() + 2 * N, b.v.data() + 2 * N, 2 * N * sizeof(double)) != 0, 0);
    for (int e : {0, 2}) {
      expect("the neighbours equal a clean run",
             std::memcmp(t.x.data() + (size_t)e * 2 * N, clean.x.data() + (size_t)e * 2 * N, 2 * N * sizeof(double)) != 0 ||
                 std::memcmp(t.v.data() + (size_t)e * 2 * N, clean.v.data() + (size_t)e * 2 * N, 2 * N * sizeof(double)) != 0 ||
                 t.collisions[e] != clean.collisions[e], 0);
    }
    expect("the twins agree", std::memcmp(t.x.data(), t.x.data() + 4 * N, 2 * N * sizeof(double)) != 0, 0);
  }
  expect("premise: the clean step moved environment 0", std::memcmp(clean.x.data(), b.x.data(), 2 * N * sizeof(double)) == 0, 0);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"status", status}}, run); }
