// Host-only driver of the search on the true environment (stove_amd/csrc/env_search.h, the text the kernel of env_search.hip runs) and
// of stove_env_search's argument check (stove_amd/csrc/validate.h: env_search), built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_env_search_cpu.py.
//   env_search_driver validate      every documented bad argument; one line per failure, exit status = number of failures
//   env_search_driver status        a draw outside [0, 9) in one tree of three, and a cap one expansion short for the largest tree: the tree
//                                   frozen as specified, its neighbours as in a clean run; as above
//   env_search_driver run IN OUT    IN:  int32 T, R, N, D, runs, cap, granularity, drift; double hw, t, friction, action_force;
//                                        double x[M][N][2], v[M][N][2], r[M][N], m[M][N] (M = T / R); int32 draws[T][runs][D]
//                                   OUT: int32 first, parent, depth, Ns, Nsa [T][cap]; double Qsa[T][cap]; int32 used[T], status[T];
//                                        double min_gap[T]; int32 action[M]
// Every tree's rows, every environment's rows and every row of the table live in a heap block of exactly their length, so the sanitizer
// sees any index past them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/env_search.h"
#include "driver.h"

static void validate() {
  const double* d = dev<const double>(1);
  const int* i = dev<const int>(2);
  const double* nd = nullptr;
  const int* ni = nullptr;
  // (x, v, r, m, draws, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, M, R, N, D, runs, cap, granularity)
  auto call = [&](int M, int R, int N, int D, int runs, int cap, int gran) {
    return stove_validate::env_search(d, d, d, d, i, i, i, i, i, i, d, i, d, i, i, M, R, N, D, runs, cap, gran);
  };
  expect("ok", call(100, 1, 3, 10, 100, 901, 5), 0);
  expect("ok at R = 32, N = 6, D = 2, the smallest cap", call(100, 32, 6, 2, 1, 10, 1), 0);
  expect("ok at N = 1", call(1, 1, 1, 2, 1, 10, 50), 0);
  expect("M = 0 (an empty batch has no arrays)",
         stove_validate::env_search(nd, nd, nd, nd, ni, ni, ni, ni, ni, ni, nd, ni, nd, ni, ni, 0, 1, 3, 10, 100, 901, 5), 0);
  expect("runs = 0 (no table)", stove_validate::env_search(d, d, d, d, ni, i, i, i, i, i, d, i, d, i, i, 4, 1, 3, 10, 0, 10, 5), 0);
  for (int k = 0; k < 15; ++k) {
    const double* dd[4] = {d, d, d, d};
    const int* ii[9] = {i, i, i, i, i, i, i, i, i};        // draws, first, parent, depth, Ns, Nsa, used, status, action
    const double *q = d, *g = d;
    if (k < 4) dd[k] = nd;
    else if (k < 13) ii[k - 4] = ni;
    else if (k == 13) q = nd;
    else g = nd;
    expect("a NULL array", stove_validate::env_search(dd[0], dd[1], dd[2], dd[3], ii[0], ii[1], ii[2], ii[3], ii[4], ii[5], q, ii[6], g, ii[7],
                                                      ii[8], 3, 1, 3, 10, 5, 46, 5), 1);
  }
  expect("M = -1", call(-1, 1, 3, 10, 5, 46, 5), 1);
  expect("R = 0", call(3, 0, 3, 10, 5, 46, 5), 1);
  expect("R = -2", call(3, -2, 3, 10, 5, 46, 5), 1);
  expect("N = 0", call(3, 1, 0, 10, 5, 46, 5), 1);
  expect("N = 7", call(3, 1, 7, 10, 5, 46, 5), 1);
  expect("D = 1", call(3, 1, 3, 1, 5, 46, 5), 1);
  expect("D = 0", call(3, 1, 3, 0, 5, 46, 5), 1);
  expect("runs = -1", call(3, 1, 3, 10, -1, 46, 5), 1);
  expect("cap = 9", call(3, 1, 3, 10, 5, 9, 5), 1);
  expect("granularity = 0", call(3, 1, 3, 10, 5, 46, 0), 1);
  expect("R = 0 at M = 0", stove_validate::env_search(nd, nd, nd, nd, ni, ni, ni, ni, ni, ni, nd, ni, nd, ni, ni, 0, 0, 3, 10, 5, 46, 5), 1);
  expect("M R past int", call(1 << 20, 1 << 12, 3, 10, 5, 46, 5), 1);
}

struct OneTree {
  std::vector<int32_t> first, parent, depth, Ns, Nsa;
  std::vector<double> Qsa;
  int used = 1, status = 0;
  double min_gap = INFINITY;
  explicit OneTree(int cap) : first(cap, -1), parent(cap, -1), depth(cap, 0), Ns(cap, 0), Nsa(cap, 0), Qsa(cap, 0.0) {}
  bool operator==(const OneTree& o) const {
    return first == o.first && parent == o.parent && depth == o.depth && Ns == o.Ns && Nsa == o.Nsa && used == o.used &&
           std::memcmp(Qsa.data(), o.Qsa.data(), Qsa.size() * sizeof(double)) == 0 && std::memcmp(&min_gap, &o.min_gap, sizeof(double)) == 0;
  }
};

// T = M R trees and the per-tree body of env_search_k, the reduction of env_search_action_k
struct Search {
  int M, R, D, cap;
  env_step::Params p;
  std::vector<std::vector<double>> x, v, r, m;        // per environment
  std::vector<OneTree> trees;
  void iterate(int t, const int32_t* row) {           // one iteration of tree t on its row of the table (D entries)
    OneTree& tr = trees[(size_t)t];
    if (tr.status != env_search::kOk) return;
    const int e = t / R;
    const std::vector<int32_t> draws(row, row + D);
    std::vector<double> xw(2 * (size_t)p.N), vw(2 * (size_t)p.N);
    const env_search::Tree tree{tr.first.data(), tr.parent.data(), tr.depth.data(), tr.Ns.data(), tr.Nsa.data(), tr.Qsa.data(), cap,
                                env_search::kActions, D};
    tr.status = env_search::iterate(tree, &tr.used, x[(size_t)e].data(), v[(size_t)e].data(), r[(size_t)e].data(), m[(size_t)e].data(), xw.data(),
                                    vw.data(), p, draws.data(), &tr.min_gap);
  }
  std::vector<int32_t> actions() {
    std::vector<int32_t> out((size_t)M);
    for (int e = 0; e < M; ++e) {
      int counts[env_search::kActions] = {0};
      for (int k = 0; k < R; ++k) {
        const OneTree& tr = trees[(size_t)e * R + k];
        env_search::add_root_counts(tr.first.data(), tr.Nsa.data(), cap, counts);
      }
      out[(size_t)e] = env_search::best_of(counts);
    }
    return out;
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head, draws;
  std::vector<double> scal;
  bool ok = read_n(in, head, 8) && read_n(in, scal, 4);
  const int T = ok ? head[0] : 0, R = ok ? head[1] : 0, N = ok ? head[2] : 0, D = ok ? head[3] : 0, runs = ok ? head[4] : 0, cap = ok ? head[5] : 0;
  ok = ok && T >= 1 && R >= 1 && T % R == 0 && N >= 1 && N <= env_step::kMaxObjects && D >= 2 && runs >= 0 && cap >= 1 + env_search::kActions &&
       head[6] >= 1;
  Search s;
  if (ok) {
    s.M = T / R;
    s.R = R;
    s.D = D;
    s.cap = cap;
    s.p = env_step::Params{N, head[6], head[7] != 0 ? 1 : 0, scal[0], scal[1], scal[2], scal[3]};
    for (auto* rows : {&s.x, &s.v}) {
      rows->resize((size_t)s.M);
      for (auto& row : *rows) ok = ok && read_n(in, row, 2 * (size_t)N);
    }
    for (auto* rows : {&s.r, &s.m}) {
      rows->resize((size_t)s.M);
      for (auto& row : *rows) ok = ok && read_n(in, row, (size_t)N);
    }
    ok = ok && read_n(in, draws, (size_t)T * runs * D);
  }
  std::fclose(in);
  if (!ok) return 2;
  s.trees.assign((size_t)T, OneTree(cap));
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < runs; ++i) s.iterate(t, draws.data() + ((size_t)t * runs + i) * D);
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  for (int k = 0; k < 5; ++k)
    for (const OneTree& tr : s.trees) ok = ok && write_v(out, k == 0 ? tr.first : k == 1 ? tr.parent : k == 2 ? tr.depth : k == 3 ? tr.Ns : tr.Nsa);
  for (const OneTree& tr : s.trees) ok = ok && write_v(out, tr.Qsa);
  std::vector<int32_t> used, status;
  std::vector<double> gaps;
  for (const OneTree& tr : s.trees) {
    used.push_back(tr.used);
    status.push_back(tr.status);
    gaps.push_back(tr.min_gap);
  }
  ok = ok && write_v(out, used) && write_v(out, status) && write_v(out, gaps) && write_v(out, s.actions());
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// a deterministic table: a small linear congruential generator, entries in [0, 9)
static std::vector<int32_t> table(int rows, int D, uint32_t seed) {
  std::vector<int32_t> out((size_t)rows * D);
  uint32_t s = seed;
  for (auto& a : out) {
    s = s * 1664525u + 1013904223u;
    a = (int32_t)((s >> 16) % 9u);
  }
  return out;
}

static Search three(int D, int cap) {
  const int N = 3;
  Search s;
  s.M = 3;
  s.R = 1;
  s.D = D;
  s.cap = cap;
  s.p = env_step::Params{N, 5, 0, 10.0, 1.0, 0.0, 0.6};
  for (int e = 0; e < 3; ++e) {
    s.x.push_back({3.0, 3.0, 4.5, 3.2, 7.0, 7.5});
    s.v.push_back({0.0, 0.0, -0.4, 0.1, 0.3, -0.2});
    s.r.push_back({1.0, 1.0, 1.0});
    s.m.push_back({10000.0, 1.0, 1.0});
  }
  s.x[1][2] = 5.4;                                  // environment 1 is another one: ball 1 sits 2.4 to the right of ball 0, so only
  s.x[1][3] = 3.0;                                  // some actions collide and its tree takes another shape than the twins'
  s.v[1][2] = 0.0;
  s.trees.assign(3, OneTree(cap));
  return s;
}

static void status() {
  const int D = 4, runs = 30, cap = 1 + env_search::kActions * runs;
  const std::vector<int32_t> tab = table(runs, D, 12345u);         // the three trees read the same rows
  // the clean run, remembered after every iteration
  std::vector<Search> clean;
  {
    Search s = three(D, cap);
    clean.push_back(s);
    for (int i = 0; i < runs; ++i) {
      for (int t = 0; t < 3; ++t) s.iterate(t, tab.data() + (size_t)i * D);
      clean.push_back(s);
    }
  }
  const Search& end = clean.back();
  expect("premise: the clean run searched", end.trees[1].status != 0 || end.trees[1].used < 1 + 3 * env_search::kActions, 0);
  expect("premise: the twins agree and differ from tree 1", !(end.trees[0] == end.trees[2]) || end.trees[0] == end.trees[1], 0);
  // ---- status 2: a draw of 9, -1, 2^30 in column 0 of iteration 7 (every iteration reads column 0), and in the last rollout column of
  // iteration 0 (the root's expansion reads all D columns)
  for (int32_t bad : {9, -1, 1 << 30})
    for (int where = 0; where < 2; ++where) {
      const int it = where == 0 ? 7 : 0, column = where == 0 ? 0 : D - 1;
      Search s = three(D, cap);
      for (int i = 0; i < runs; ++i)
        for (int t = 0; t < 3; ++t) {
          std::vector<int32_t> row(tab.begin() + (size_t)i * D, tab.begin() + (size_t)(i + 1) * D);
          if (t == 1 && i == it) row[(size_t)column] = bad;
          s.iterate(t, row.data());
        }
      expect("status 2", s.trees[1].status != env_search::kBad, 0);
      expect("the refused tree is as it stood at the start of that iteration", !(s.trees[1] == clean[(size_t)it].trees[1]), 0);
      expect("the neighbours equal a clean run", !(s.trees[0] == end.trees[0]) || !(s.trees[2] == end.trees[2]) || s.trees[0].status != 0 ||
                                                     s.trees[2].status != 0, 0);
      const std::vector<int32_t> a = s.actions(), want = clean[(size_t)it].actions(), all = clean.back().actions();
      expect("the refused tree's action is that of its frozen counts", a[1] != want[1] || a[0] != all[0] || a[2] != all[2], 0);
    }
  // ---- status 1: all three trees under a cap one expansion short of what the largest clean tree used: that tree (or the twins) stops at
  // its last expansion, the smaller trees search on as in the clean run
  {
    // (each tree reads a table of its own here, so that the three trees do not use the same number of slots)
    const std::vector<int32_t> tabs[3] = {table(runs, D, 777u), table(runs, D, 4242u), table(runs, D, 99u)};
    std::vector<Search> clean;
    {
      Search c = three(D, cap);
      clean.push_back(c);
      for (int i = 0; i < runs; ++i) {
        for (int t = 0; t < 3; ++t) c.iterate(t, tabs[t].data() + (size_t)i * D);
        clean.push_back(c);
      }
    }
    const Search& end = clean.back();
    int need = 0;
    for (int t = 0; t < 3; ++t) need = end.trees[(size_t)t].used > need ? end.trees[(size_t)t].used : need;
    const int shortcap = need - 1;                                          // (room for all but the last A slots: used + A > cap there)
    Search s = three(D, shortcap);
    for (int i = 0; i < runs; ++i)
      for (int t = 0; t < 3; ++t) s.iterate(t, tabs[t].data() + (size_t)i * D);
    auto same_rows = [&](const OneTree& got, const OneTree& want) {
      bool same = got.used == want.used && std::memcmp(&got.min_gap, &want.min_gap, sizeof(double)) == 0;
      for (int k = 0; k < shortcap; ++k)
        same = same && got.first[(size_t)k] == want.first[(size_t)k] && got.parent[(size_t)k] == want.parent[(size_t)k] &&
               got.depth[(size_t)k] == want.depth[(size_t)k] && got.Ns[(size_t)k] == want.Ns[(size_t)k] && got.Nsa[(size_t)k] == want.Nsa[(size_t)k] &&
               std::memcmp(&got.Qsa[(size_t)k], &want.Qsa[(size_t)k], sizeof(double)) == 0;
      return same;
    };
    int full = 0, clean_ones = 0;
    for (int t = 0; t < 3; ++t) {
      const OneTree& got = s.trees[(size_t)t];
      if (end.trees[(size_t)t].used == need) {
        int it = 0;
        while (clean[(size_t)it + 1].trees[(size_t)t].used < need) ++it;     // the iteration of the last expansion
        expect("status 1", got.status != env_search::kFull, 0);
        expect("the full tree is as it stood at the start of that iteration", !same_rows(got, clean[(size_t)it].trees[(size_t)t]), 0);
        expect("premise: the last expansion is not the first", it < 1, 0);
        ++full;
      } else {
        expect("a neighbour of the full tree searched on", got.status, 0);
        expect("a neighbour of the full tree equals the clean run", !same_rows(got, end.trees[(size_t)t]), 0);
        ++clean_ones;
      }
    }
    expect("premise: a full tree next to searching neighbours", full < 1 || clean_ones < 1, 0);
  }
  // ---- an empty search: no iteration, action 0
  {
    Search s = three(D, cap);
    const std::vector<int32_t> a = s.actions();
    expect("an empty search returns action 0", a[0] != 0 || a[1] != 0 || a[2] != 0, 0);
  }
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"status", status}}, run); }
