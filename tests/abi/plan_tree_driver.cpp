// Host-only driver of the search-tree arithmetic (stove_amd/csrc/plan_tree.h, the text the kernels of plan_tree.hip run) and of
// stove_plan_search's argument check (stove_amd/csrc/validate.h: plan_search), built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_plan_tree_cpu.py.
//   plan_tree_driver validate            every documented bad argument; one line per failure, exit status = number of failures
//   plan_tree_driver corrupt             trees with damaged arrays: status 2, the tree untouched, its neighbour unaffected; as above
//   plan_tree_driver run IN OUT          IN:  int32 M, A, D, cap, R; int32 used[M]; float32 q[R][M][A]
//                                        OUT: int32 sel[R][M], child[R][M], status[M], used[M], first / parent / depth / Ns / Nsa [M][cap],
//                                             action[M]; double Qsa[M][cap], min_gap[M]
// `run` starts from fresh trees (a root each) and does select -> child_slots -> backpropagate per iteration and tree as
// stove_plan_search does: a tree whose status is not 0 is frozen, its sel / child entries are -1 from there on.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stove_amd/csrc/plan_tree.h"
#include "driver.h"

static void validate() {
  using stove_validate::plan_search;
  const float* f = dev<const float>(1);
  const int* i = dev<const int>(2);
  const double* d = dev<const double>(3);
  void* ws = dev<void>(4);
  const float* nf = nullptr;
  const int* ni = nullptr;
  const double* nd = nullptr;
  // (z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, app, acts, emb_w, emb_b, gnn_params, rh_params, ws,
  //  M, cap, A, L, D, N, app_dim, R)
  expect("ok", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 100, 901, 9, 20, 10, 3, 3, 100), 0);
  expect("R = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 0), 0);
  expect("ok without appearance", plan_search(f, i, i, i, i, i, d, i, d, i, i, nf, i, f, f, f, f, ws, 3, 10, 9, 4, 2, 3, 0, 5), 0);
  expect("NULL z_pool", plan_search(nf, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL first", plan_search(f, ni, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL parent", plan_search(f, i, ni, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL depth", plan_search(f, i, i, ni, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL Ns", plan_search(f, i, i, i, ni, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL Nsa", plan_search(f, i, i, i, i, ni, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL Qsa", plan_search(f, i, i, i, i, i, nd, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL used", plan_search(f, i, i, i, i, i, d, ni, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL min_gap", plan_search(f, i, i, i, i, i, d, i, nd, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL status", plan_search(f, i, i, i, i, i, d, i, d, ni, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL action", plan_search(f, i, i, i, i, i, d, i, d, i, ni, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL action at R = 0", plan_search(f, i, i, i, i, i, d, i, d, i, ni, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 0), 1);
  expect("NULL app with app_dim = 3", plan_search(f, i, i, i, i, i, d, i, d, i, i, nf, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL acts", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, ni, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL acts at R = 0 (there are none)", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, ni, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 0), 0);
  expect("NULL emb_w", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, nf, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL emb_b", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, nf, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL gnn_params", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, nf, f, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL rh_params", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, nf, ws, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("NULL ws", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, nullptr, 3, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("R = -1", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, -1), 1);
  expect("cap = A", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 9, 9, 4, 2, 3, 3, 5), 1);
  expect("cap = 1 + A", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 10, 9, 4, 2, 3, 3, 5), 0);
  // what plan_expand rejects
  expect("M = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 0, 22, 9, 4, 2, 3, 3, 5), 1);
  expect("A = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 0, 4, 2, 3, 3, 5), 1);
  expect("A = 65", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 100, 65, 4, 2, 3, 3, 5), 1);
  expect("L = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 0, 2, 3, 3, 5), 1);
  expect("D = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 0, 3, 3, 5), 1);
  expect("N = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 0, 3, 5), 1);
  expect("N = 9", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 9, 3, 5), 1);
  expect("app_dim = 13", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 13, 5), 1);
  expect("app_dim < 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, -1, 5), 1);
  expect("rows x steps beyond an int's reach", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 1 << 20, 22, 9, 1 << 20, 2, 3, 3, 5), 1);
}

// M trees' arrays and the per-iteration loop of stove_plan_search (a frozen tree is skipped, its sel / child entries stay -1)
struct Forest {
  int M, A, D, cap;
  std::vector<int32_t> first, parent, depth, Ns, Nsa, used, status;
  std::vector<double> Qsa, min_gap;
  Forest(int M_, int A_, int D_, int cap_)
      : M(M_), A(A_), D(D_), cap(cap_), first((size_t)M_ * cap_, -1), parent((size_t)M_ * cap_, -1), depth((size_t)M_ * cap_, 0),
        Ns((size_t)M_ * cap_, 0), Nsa((size_t)M_ * cap_, 0), used((size_t)M_, 1), status((size_t)M_, 0), Qsa((size_t)M_ * cap_, 0.0),
        min_gap((size_t)M_, INFINITY) {}
  plan_tree::Tree tree(int m) {
    const size_t o = (size_t)m * cap;
    return plan_tree::Tree{first.data() + o, parent.data() + o, depth.data() + o, Ns.data() + o, Nsa.data() + o, Qsa.data() + o, cap, A, D};
  }
  // q (R, M, A); sel, child (R, M) or NULL
  void search(const float* q, int R, int32_t* sel, int32_t* child) {
    for (int i = 0; i < R; ++i)
      for (int m = 0; m < M; ++m) {
        if (status[m] != plan_tree::kOk) continue;
        const plan_tree::Tree t = tree(m);
        int leaf = -1, ch = -1, len_s = 0, us = used[m];
        double gap = INFINITY;
        int st = plan_tree::select(t, 1.0, &leaf, &gap);
        if (st == plan_tree::kOk) st = plan_tree::child_slots(t, leaf, &us, &ch, &len_s);
        status[m] = st;
        if (st != plan_tree::kOk) continue;
        used[m] = us;
        if (gap < min_gap[m]) min_gap[m] = gap;
        if (sel != nullptr) sel[(size_t)i * M + m] = leaf;
        if (child != nullptr) child[(size_t)i * M + m] = ch;
        plan_tree::backpropagate(t, leaf, ch, q + ((size_t)i * M + m) * A);
      }
  }
  bool same_tree(const Forest& o, int m) const {
    const size_t a = (size_t)m * cap, n = (size_t)cap;
    return std::equal(first.begin() + a, first.begin() + a + n, o.first.begin() + a) &&
           std::equal(parent.begin() + a, parent.begin() + a + n, o.parent.begin() + a) &&
           std::equal(depth.begin() + a, depth.begin() + a + n, o.depth.begin() + a) &&
           std::equal(Ns.begin() + a, Ns.begin() + a + n, o.Ns.begin() + a) && std::equal(Nsa.begin() + a, Nsa.begin() + a + n, o.Nsa.begin() + a) &&
           std::memcmp(Qsa.data() + a, o.Qsa.data() + a, n * sizeof(double)) == 0 && used[m] == o.used[m];
  }
};

static int run(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (in == nullptr) return 2;
  std::vector<int32_t> head, used;
  std::vector<float> q;
  bool ok = read_n(in, head, 5);
  const int M = ok ? head[0] : 0, A = ok ? head[1] : 0, D = ok ? head[2] : 0, cap = ok ? head[3] : 0, R = ok ? head[4] : 0;
  ok = ok && M >= 1 && A >= 1 && A <= plan_tree::kMaxActions && D >= 1 && cap >= 1 + A && R >= 0;
  ok = ok && read_n(in, used, (size_t)M) && read_n(in, q, (size_t)R * M * A);
  std::fclose(in);
  if (!ok) return 2;
  Forest f(M, A, D, cap);
  f.used = used;
  std::vector<int32_t> sel((size_t)R * M, -1), child((size_t)R * M, -1);
  f.search(q.data(), R, sel.data(), child.data());
  std::vector<int32_t> action((size_t)M);
  for (int m = 0; m < M; ++m) action[m] = plan_tree::best_action(f.tree(m));
  std::FILE* out = std::fopen(out_path, "wb");
  if (out == nullptr) return 2;
  ok = write_v(out, sel) && write_v(out, child) && write_v(out, f.status) && write_v(out, f.used) && write_v(out, f.first) &&
       write_v(out, f.parent) && write_v(out, f.depth) && write_v(out, f.Ns) && write_v(out, f.Nsa) && write_v(out, action) &&
       write_v(out, f.Qsa) && write_v(out, f.min_gap);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}

// Trees with corrupt arrays (status 2).  Six trees grow for R0 iterations on made-up values (D = 8 > R0: every leaf is fresh), then
// five of them are damaged, each in its own way, and all go on for R1 more.  A damaged tree must end with status 2 and exactly the
// arrays it was handed (nothing written, and -- under the address sanitizer -- nothing read outside them); tree 0 must end as in a
// forest nobody damaged.
static void corrupt() {
  const int M = 6, A = 3, D = 8, cap = 1 + A * 12, R0 = 6, R1 = 4;
  std::vector<float> q((size_t)(R0 + R1) * M * A);
  for (size_t k = 0; k < q.size(); ++k) q[k] = -1.0f - 0.37f * (float)((k * 2654435761u >> 7) % 1000) / 1000.0f;
  Forest clean(M, A, D, cap), f(M, A, D, cap);
  clean.search(q.data(), R0 + R1, nullptr, nullptr);
  f.search(q.data(), R0, nullptr, nullptr);
  for (int m = 0; m < M; ++m) {
    expect("premise: a clean tree stays fine", clean.status[m], 0);
    expect("premise: every leaf was fresh", clean.used[m] != 1 + A * (R0 + R1), 0);
  }
  const size_t c = (size_t)cap;
  f.first[1 * c + 0] = cap + 100;                                  // 1: the root's children far outside the arrays
  f.first[2 * c + 0] = cap - A + 1;                                // 2: ... one slot outside
  for (int s = 1; s < f.used[3]; ++s) f.parent[3 * c + s] = s;     // 3: a parent chain that never reaches depth 0
  for (int s = 0; s < f.used[4]; ++s) {                            // 4: a descent that never ends (every leaf points back at the root's
    f.depth[4 * c + s] = 0;                                        //    children, no node is ever at the depth limit)
    if (f.first[4 * c + s] < 0) f.first[4 * c + s] = f.first[4 * c + 0];
  }
  f.used[5] = cap + 5;                                             // 5: the slot cursor outside the arrays
  const Forest handed = f;
  std::vector<int32_t> sel((size_t)R1 * M, -7);
  f.search(q.data() + (size_t)R0 * M * A, R1, sel.data(), nullptr);
  expect("tree 0 stays fine", f.status[0], 0);
  expect("tree 0 as in a forest nobody damaged", !f.same_tree(clean, 0), 0);
  for (int m = 1; m < M; ++m) {
    expect("status 2", f.status[m] != plan_tree::kBad, 0);
    expect("a damaged tree is left as handed over", !f.same_tree(handed, m), 0);
    for (int i = 0; i < R1; ++i) expect("no leaf recorded for a damaged tree", sel[(size_t)i * M + m] != -7, 0);
    expect("no action read outside the arrays", plan_tree::best_action(f.tree(m)) < 0 || plan_tree::best_action(f.tree(m)) >= A, 0);
  }
  // a slot cursor below 1, and a parent index outside the arrays
  Forest g = handed;
  g.status.assign((size_t)M, 0);
  g.used[5] = 0;
  for (int s = 1; s < g.used[3]; ++s) g.parent[3 * c + s] = cap + 100;
  const Forest handed2 = g;
  g.search(q.data() + (size_t)R0 * M * A, 1, nullptr, nullptr);
  for (int m : {3, 5}) {
    expect("status 2 (second set)", g.status[m] != plan_tree::kBad, 0);
    expect("left as handed over (second set)", !g.same_tree(handed2, m), 0);
  }
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}, {"corrupt", corrupt}}, run); }
