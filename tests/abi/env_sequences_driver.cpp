// Host-only driver of whole sequences (stove_amd/csrc/env_step.h and stove_amd/csrc/env_gravity.h, the text the kernel of
// env_sequences.hip runs) and of stove_env_sequences' argument check (stove_amd/csrc/validate.h: env_sequences), built with
// -fsanitize=address,undefined and -ffp-contract=off by tests/test_env_sequences_cpu.py.
//   env_sequences_driver validate     every documented bad argument; one line per failure, exit status = number of failures
//   env_sequences_driver status       an action index outside [0, 9) anywhere in a row: status 2, the sequence's rows untouched, its
//                                     neighbours as in a clean run; as above
//   env_sequences_driver run IN OUT   IN:  int32 B, N, T, granularity, drift, acting, kind, res, use_colors; double hw, t, friction,
//                                          action_force; double x0[B][N][2], v0[B][N][2], r[B][N], m[B][N]; int32 actions[B][T] (if acting)
//                                     OUT: double y[B][T][N][4]; int32 collisions[B][T], in_bounds[B], status[B];
//                                          float frames[B][T][3][res][res]
// A sequence runs as the kernel runs it: the action row scanned first, then T times step, record, count, paint.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/env_gravity.h"
#include "../../stove_amd/csrc/env_step.h"
#include "driver.h"

static void validate() {
  using stove_validate::env_sequences;
  const double* d = dev<const double>(1);
  const int* i = dev<const int>(2);
  const double* nd = nullptr;
  const int* ni = nullptr;
  // (x0, v0, r, m, actions, y, collisions, in_bounds, status, B, N, T, granularity, res, kind)
  expect("ok", env_sequences(d, d, d, d, i, d, i, i, i, 1000, 3, 100, 10, 32, 0), 0);
  expect("ok without actions", env_sequences(d, d, d, d, ni, d, i, i, i, 4, 3, 12, 10, 32, 0), 0);
  expect("ok gravity", env_sequences(d, d, d, d, ni, d, i, i, i, 4, 3, 12, 50, 50, 1), 0);
  expect("ok at N = 1, T = 1, granularity 1, res 1", env_sequences(d, d, d, d, ni, d, i, i, i, 1, 1, 1, 1, 1, 0), 0);
  expect("ok at N = 6", env_sequences(d, d, d, d, i, d, i, i, i, 65, 6, 3, 50, 50, 0), 0);
  expect("B = 0 (an empty batch has no arrays)", env_sequences(nd, nd, nd, nd, ni, nd, ni, ni, ni, 0, 3, 12, 10, 32, 0), 0);
  expect("NULL x0", env_sequences(nd, d, d, d, i, d, i, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL v0", env_sequences(d, nd, d, d, i, d, i, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL r", env_sequences(d, d, nd, d, i, d, i, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL m", env_sequences(d, d, d, nd, i, d, i, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL y", env_sequences(d, d, d, d, i, nd, i, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL collisions", env_sequences(d, d, d, d, i, d, ni, i, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL in_bounds", env_sequences(d, d, d, d, i, d, i, ni, i, 3, 3, 12, 10, 32, 0), 1);
  expect("NULL status", env_sequences(d, d, d, d, i, d, i, i, ni, 3, 3, 12, 10, 32, 0), 1);
  expect("B = -1", env_sequences(d, d, d, d, i, d, i, i, i, -1, 3, 12, 10, 32, 0), 1);
  expect("N = 0", env_sequences(d, d, d, d, i, d, i, i, i, 3, 0, 12, 10, 32, 0), 1);
  expect("N = 7", env_sequences(d, d, d, d, i, d, i, i, i, 3, 7, 12, 10, 32, 0), 1);
  expect("N = 0 at B = 0", env_sequences(nd, nd, nd, nd, ni, nd, ni, ni, ni, 0, 0, 12, 10, 32, 0), 1);
  expect("T = 0", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 0, 10, 32, 0), 1);
  expect("T = -1", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, -1, 10, 32, 0), 1);
  expect("granularity = 0", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, 0, 32, 0), 1);
  expect("granularity = -5", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, -5, 32, 0), 1);
  expect("res = 0", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, 10, 0, 0), 1);
  expect("res = -32", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, 10, -32, 0), 1);
  expect("res = 20000 (a frame's pixels are counted in int)", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, 10, 20000, 0), 1);
  expect("kind = 2", env_sequences(d, d, d, d, ni, d, i, i, i, 3, 3, 12, 10, 32, 2), 1);
  expect("kind = -1", env_sequences(d, d, d, d, ni, d, i, i, i, 3, 3, 12, 10, 32, -1), 1);
  expect("gravity with actions", env_sequences(d, d, d, d, i, d, i, i, i, 3, 3, 12, 50, 32, 1), 1);
  expect("gravity with actions at B = 0", env_sequences(nd, nd, nd, nd, i, nd, ni, ni, ni, 0, 3, 12, 50, 32, 1), 1);
}

// B sequences' arrays and the per-sequence body of env_sequences_k
struct Batch {
  int B, T, kind, res, use_colors;
  env_step::Params p;
  std::vector<double> x0, v0, r, m, y;
  std::vector<int32_t> collisions, in_bounds, status;
  std::vector<float> frames;
  void shape(int32_t ifill, double dfill, float ffill) {
    y.assign((size_t)B * T * p.N * 4, dfill);
    collisions.assign((size_t)B * T, ifill);
    in_bounds.assign((size_t)B, ifill);
    status.assign((size_t)B, ifill);
    frames.assign((size_t)B * T * 3 * res * res, ffill);
  }
  // actions (B, T) or NULL
  void run(const int32_t* actions) {
    const int N = p.N;
    const size_t plane = (size_t)res * res;
    for (int e = 0; e < B; ++e) {
      bool bad = false;
      if (actions != nullptr)
        for (int s = 0; s < T; ++s) bad = bad || actions[(size_t)e * T + s] < 0 || actions[(size_t)e * T + s] >= env_step::kActions;
      if (bad) {
        status[e] = env_step::kBadAction;
        continue;
      }
      std::vector<double> sx(x0.begin() + (size_t)e * 2 * N, x0.begin() + (size_t)(e + 1) * 2 * N);      // exactly 2 N long: the sanitizer
      std::vector<double> sv(v0.begin() + (size_t)e * 2 * N, v0.begin() + (size_t)(e + 1) * 2 * N);      // sees any index past the rows
      std::vector<double> sr(r.begin() + (size_t)e * N, r.begin() + (size_t)(e + 1) * N);
      std::vector<double> sm(m.begin() + (size_t)e * N, m.begin() + (size_t)(e + 1) * N);
      int count = 0;
      for (int s = 0; s < T; ++s) {
        int hit = 0;
        if (kind == 1)
          env_gravity::step(sx.data(), sv.data(), sm.data(), p);
        else
          env_step::step(sx.data(), sv.data(), sr.data(), sm.data(), p, actions != nullptr ? actions + (size_t)e * T + s : nullptr, &hit);
        double* row = y.data() + ((size_t)e * T + s) * 4 * N;
        for (int i = 0; i < N; ++i) {
          row[4 * i] = sx[2 * i];
          row[4 * i + 1] = sx[2 * i + 1];
          row[4 * i + 2] = sv[2 * i];
          row[4 * i + 3] = sv[2 * i + 1];
        }
        collisions[(size_t)e * T + s] = hit;
        count += env_gravity::inside(sx.data(), N, p.hw);
        float* out = frames.data() + ((size_t)e * T + s) * 3 * plane;
        for (size_t px = 0; px < plane; ++px) {
          const int a = (int)(px / res), b = (int)(px % res);
          float rgb[3];
          env_step::pixel(sx.data(), sr.data(), N, use_colors, env_step::centre(b, res, p.hw), env_step::centre(a, res, p.hw), rgb);
          for (int ch = 0; ch < 3; ++ch) out[ch * plane + px] = rgb[ch];
        }
      }
      in_bounds[e] = count;
      status[e] = env_step::kOk;
    }
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head, actions;
  std::vector<double> scal;
  Batch b;
  bool ok = read_n(in, head, 9) && read_n(in, scal, 4);
  const int B = ok ? head[0] : 0, N = ok ? head[1] : 0, T = ok ? head[2] : 0, gran = ok ? head[3] : 0, acting = ok ? head[5] : 0;
  const int kind = ok ? head[6] : 0, res = ok ? head[7] : 0;
  ok = ok && B >= 1 && N >= 1 && N <= env_step::kMaxObjects && T >= 1 && gran >= 1 && res >= 1 && res <= 256 && (kind == 0 || kind == 1) &&
       !(kind == 1 && acting);
  if (ok) {
    b.B = B;
    b.T = T;
    b.kind = kind;
    b.res = res;
    b.use_colors = head[8] != 0 ? 1 : 0;
    b.p = env_step::Params{N, gran, head[4] != 0 ? 1 : 0, scal[0], scal[1], scal[2], scal[3]};
    ok = read_n(in, b.x0, (size_t)B * N * 2) && read_n(in, b.v0, (size_t)B * N * 2) && read_n(in, b.r, (size_t)B * N) &&
         read_n(in, b.m, (size_t)B * N) && (!acting || read_n(in, actions, (size_t)B * T));
  }
  std::fclose(in);
  if (!ok) return 2;
  b.shape(0, 0.0, 0.0f);
  b.run(acting ? actions.data() : nullptr);
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  ok = write_v(out, b.y) && write_v(out, b.collisions) && write_v(out, b.in_bounds) && write_v(out, b.status) && write_v(out, b.frames);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// Three sequences of T = 5 steps, the same start in 0 and 2; sequence 1 gets an action index of 9, -1 or 2^30 at step 0, in the middle
// or at step T - 1: status [0, 2, 0], sequence 1's output rows keep their poison pattern, 0 and 2 as in a run where all actions were fine.
static void status() {
  const int B = 3, N = 3, T = 5, res = 8;
  Batch b;
  b.B = B;
  b.T = T;
  b.kind = 0;
  b.res = res;
  b.use_colors = 1;
  b.p = env_step::Params{N, 5, 0, 10.0, 1.0, 0.0, 0.6};
  const double x0[N * 2] = {3.0, 3.0, 4.5, 3.2, 7.0, 7.5}, v0[N * 2] = {0.0, 0.0, -0.4, 0.1, 0.3, -0.2};
  for (int e = 0; e < B; ++e) {
    b.x0.insert(b.x0.end(), x0, x0 + N * 2);
    b.v0.insert(b.v0.end(), v0, v0 + N * 2);
    for (int i = 0; i < N; ++i) {
      b.r.push_back(1.0);
      b.m.push_back(i == 0 ? 10000.0 : 1.0);
    }
  }
  b.x0[2 * N] = 6.0;                                // sequence 1 is another one
  const double poison = -7.5;
  b.shape(-7, poison, -7.5f);
  Batch clean = b;
  std::vector<int32_t> good((size_t)B * T, 1);
  for (int s = 0; s < T; ++s) good[(size_t)T + s] = 3;
  clean.run(good.data());
  const size_t ny = (size_t)T * N * 4, nf = (size_t)T * 3 * res * res;
  for (int32_t bad : {9, -1, 1 << 30})
    for (int at : {0, T / 2, T - 1}) {
      Batch t = b;
      std::vector<int32_t> acts = good;
      acts[(size_t)T + at] = bad;
      t.run(acts.data());
      expect("status of sequence 0", t.status[0], 0);
      expect("status 2", t.status[1] != env_step::kBadAction, 0);
      expect("status of sequence 2", t.status[2], 0);
      bool kept = t.in_bounds[1] == -7;
      for (size_t k = 0; k < ny; ++k) kept = kept && t.y[ny + k] == poison;
      for (size_t k = 0; k < nf; ++k) kept = kept && t.frames[nf + k] == -7.5f;
      for (int s = 0; s < T; ++s) kept = kept && t.collisions[(size_t)T + s] == -7;
      check("the refused sequence's rows keep the poison pattern", kept);
      for (int e : {0, 2})
        check("the neighbours equal a clean run",
              std::memcmp(t.y.data() + e * ny, clean.y.data() + e * ny, ny * sizeof(double)) == 0 &&
                  std::memcmp(t.frames.data() + e * nf, clean.frames.data() + e * nf, nf * sizeof(float)) == 0 &&
                  std::memcmp(t.collisions.data() + (size_t)e * T, clean.collisions.data() + (size_t)e * T, T * sizeof(int32_t)) == 0 &&
                  t.in_bounds[e] == clean.in_bounds[e]);
      check("the twins agree", std::memcmp(t.y.data(), t.y.data() + 2 * ny, ny * sizeof(double)) == 0);
    }
  check("premise: the clean run moved sequence 0", clean.y[4] != x0[2] && clean.status[1] == 0 && clean.in_bounds[0] == 2 * N * T);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"status", status}}, run); }
