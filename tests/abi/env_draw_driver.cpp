// Host-only driver of the counter-based random stream of data synthesis (stove_amd/csrc/env_draw.h, the text the kernel of
// env_draw.hip runs) and of stove_env_draw_starts' argument check (stove_amd/csrc/validate.h: env_draw_starts), built with
// -fsanitize=address,undefined and -ffp-contract=off by tests/test_env_draw_cpu.py.
//   env_draw_driver validate     every documented bad argument; one line per failure, exit status = number of failures
//   env_draw_driver philox       the published known-answer vectors of Philox4x32-10; as above
//   env_draw_driver run IN OUT   IN:  int32 B, N, T, acting, kind, max_tries, seed_lo, seed_hi; double hw, v_factor; double r[B][N]
//                                OUT: double x0[B][N][2], v0[B][N][2]; int32 actions[B][T] (if acting), tries[B], status[B]
//                                kind 2: IN's arrays are double x[B] instead, OUT is double log_pos(x)[B]
// A sequence is drawn as the kernel draws it, except that the attempts are walked one by one: the first good one is the lowest.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../stove_amd/csrc/env_draw.h"
#include "driver.h"

static void validate() {
  using stove_validate::env_draw_starts;
  const double* d = dev<const double>(1);
  const int* i = dev<const int>(2);
  const double* nd = nullptr;
  const int* ni = nullptr;
  // (r, x0, v0, tries, status, B, N, T, kind, max_tries)
  expect("ok", env_draw_starts(d, d, d, i, i, 1000, 3, 100, 0, 1 << 20), 0);
  expect("ok gravity", env_draw_starts(d, d, d, i, i, 4, 3, 12, 1, 1), 0);
  expect("ok at N = 1, T = 0, max_tries = 1", env_draw_starts(d, d, d, i, i, 1, 1, 0, 0, 1), 0);
  expect("ok at N = 6", env_draw_starts(d, d, d, i, i, 65, 6, 3, 0, 0x7fffffff), 0);
  expect("B = 0 (an empty batch has no arrays)", env_draw_starts(nd, nd, nd, ni, ni, 0, 3, 12, 0, 64), 0);
  expect("NULL r", env_draw_starts(nd, d, d, i, i, 3, 3, 12, 0, 64), 1);
  expect("NULL x0", env_draw_starts(d, nd, d, i, i, 3, 3, 12, 0, 64), 1);
  expect("NULL v0", env_draw_starts(d, d, nd, i, i, 3, 3, 12, 0, 64), 1);
  expect("NULL tries", env_draw_starts(d, d, d, ni, i, 3, 3, 12, 0, 64), 1);
  expect("NULL status", env_draw_starts(d, d, d, i, ni, 3, 3, 12, 0, 64), 1);
  expect("B = -1", env_draw_starts(d, d, d, i, i, -1, 3, 12, 0, 64), 1);
  expect("N = 0", env_draw_starts(d, d, d, i, i, 3, 0, 12, 0, 64), 1);
  expect("N = 7", env_draw_starts(d, d, d, i, i, 3, 7, 12, 0, 64), 1);
  expect("N = 0 at B = 0", env_draw_starts(nd, nd, nd, ni, ni, 0, 0, 12, 0, 64), 1);
  expect("T = -1", env_draw_starts(d, d, d, i, i, 3, 3, -1, 0, 64), 1);
  expect("max_tries = 0", env_draw_starts(d, d, d, i, i, 3, 3, 12, 0, 0), 1);
  expect("max_tries = -5", env_draw_starts(d, d, d, i, i, 3, 3, 12, 0, -5), 1);
  expect("max_tries = 0 under gravity", env_draw_starts(d, d, d, i, i, 3, 3, 12, 1, 0), 1);
  expect("kind = 2", env_draw_starts(d, d, d, i, i, 3, 3, 12, 2, 64), 1);
  expect("kind = -1", env_draw_starts(d, d, d, i, i, 3, 3, 12, -1, 64), 1);
}

// Random123's kat_vectors, philox4x32 10: counter, key -> output
static void philox() {
  struct Kat {
    uint32_t c[4], k[2], want[4];
  };
  const Kat kats[] = {
      {{0u, 0u, 0u, 0u}, {0u, 0u}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
  };
  for (const Kat& t : kats) {
    const env_draw::Block b = env_draw::philox(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
    check("philox4x32-10 known answer", b.w0 == t.want[0] && b.w1 == t.want[1] && b.w2 == t.want[2] && b.w3 == t.want[3]);
  }
  check("uniform of all ones is the largest double below 1", env_draw::uniform(0xffffffffu, 0xffffffffu) == 1.0 - 1.0 / 9007199254740992.0);
  check("uniform of zeros is 0", env_draw::uniform(31u, 63u) == 0.0);
}

template <int N>
static void draw(uint64_t seed, const double* r, int kind, int max_tries, double hw, double factor, double* x0, double* v0, int32_t* tries,
                 int32_t* status) {
  double x[2 * N], v[2 * N];          // exactly 2 N long: the sanitizer sees any index past the rows
  const uint32_t limit = kind == 1 ? (uint32_t)env_draw::kGravityTries : (uint32_t)max_tries;
  bool good = false;
  uint32_t k = 0;
  for (; k < limit; ++k) {
    good = kind == 1 ? env_draw::gravity_attempt<N>(seed, k, hw, x) : env_draw::billiards_attempt<N>(seed, k, r, hw, x);
    if (good) break;
  }
  if (!good && kind == 1) {          // x holds attempt 999
    good = true;
    k = limit - 1;
  }
  if (!good) {
    for (int c = 0; c < 2 * N; ++c) x0[c] = v0[c] = 0.0;
    *tries = max_tries;
    *status = env_draw::kNoStart;
    return;
  }
  if (kind == 1)
    env_draw::gravity_velocity<N>(seed, x, factor, v);
  else
    env_draw::billiards_velocity<N>(seed, factor, v);
  for (int c = 0; c < 2 * N; ++c) {
    x0[c] = x[c];
    v0[c] = v[c];
  }
  *tries = (int32_t)k + 1;
  *status = env_draw::kOk;
}

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head;
  std::vector<double> scal, r, xs;
  bool ok = read_n(in, head, 8) && read_n(in, scal, 2);
  const int B = ok ? head[0] : 0, N = ok ? head[1] : 0, T = ok ? head[2] : 0, acting = ok ? head[3] : 0, kind = ok ? head[4] : 0;
  const int max_tries = ok ? head[5] : 0;
  ok = ok && B >= 1 && (kind == 2 || (N >= 1 && N <= env_draw::kMaxObjects && T >= 0 && max_tries >= 1 && (kind == 0 || kind == 1)));
  if (ok) ok = kind == 2 ? read_n(in, xs, (size_t)B) : read_n(in, r, (size_t)B * N);
  std::fclose(in);
  if (!ok) return 2;
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  if (kind == 2) {
    std::vector<double> logs((size_t)B);
    for (int e = 0; e < B; ++e) logs[e] = env_draw::log_pos(xs[e]);
    ok = write_v(out, logs);
    return (std::fclose(out) == 0 && ok) ? 0 : 2;
  }
  const uint64_t seed0 = ((uint64_t)(uint32_t)head[7] << 32) | (uint32_t)head[6];
  const double hw = scal[0], factor = scal[1];
  std::vector<double> x0((size_t)B * N * 2), v0((size_t)B * N * 2);
  std::vector<int32_t> actions(acting ? (size_t)B * T : 0), tries((size_t)B), status((size_t)B);
  for (int e = 0; e < B; ++e) {
    const uint64_t seed = seed0 + (uint64_t)e;
    const double* re = r.data() + (size_t)e * N;
    double *xe = x0.data() + (size_t)e * 2 * N, *ve = v0.data() + (size_t)e * 2 * N;
    switch (N) {
      case 1: draw<1>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
      case 2: draw<2>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
      case 3: draw<3>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
      case 4: draw<4>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
      case 5: draw<5>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
      default: draw<6>(seed, re, kind, max_tries, hw, factor, xe, ve, &tries[e], &status[e]); break;
    }
    if (acting) {
      const double p = env_draw::change_prob(seed);
      int cur = env_draw::first_state(seed);
      for (int s = 0; s < T; ++s) {
        cur = env_draw::next_state(cur, p, env_draw::action_uniform(seed, (uint32_t)s));
        actions[(size_t)e * T + s] = cur;
      }
    }
  }
  ok = write_v(out, x0) && write_v(out, v0) && write_v(out, actions) && write_v(out, tries) && write_v(out, status);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"philox", philox}}, run); }
