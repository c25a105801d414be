// Host-only driver of the argument checks of stove_plan_expand_cl / stove_plan_search_cl (stove_amd/csrc/validate.h: plan_dims_bad,
// plan_expand, plan_search run with gnn_limits_cl(cl)), built with -fsanitize=address,undefined by tests/test_plan_cl_cpu.py, in the
// manner of plan_validate_driver.cpp: fake, never-mapped "device" pointers that the layer must not dereference.  Where plan_dims_bad
// holds the workspace queries return 0 (csrc/capi.hip); the CPU test asks the library for that.
// `plan_cl_validate_driver validate`: one line per failure, exit status = number of failures.
#include <cstdio>
#include <cstdint>

#include "driver.h"

using namespace stove_validate;

static const float* f = dev<const float>(1);
static const int* i = dev<const int>(2);
static const double* d = dev<const double>(3);
static void* ws = dev<void>(4);

// (cl, M, cap, A, L, D, N, app_dim) with every pointer given
static int expand(int cl, int M, int cap, int A, int L, int D, int N, int app_dim) {
  return plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, M, cap, A, L, D, N, app_dim, gnn_limits_cl(cl));
}
static int search(int cl, int M, int cap, int A, int L, int D, int N, int app_dim, int R) {
  return plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, M, cap, A, L, D, N, app_dim, R, gnn_limits_cl(cl));
}
// both checks refuse, and the dimensions alone are what the workspace queries answer 0 to
static void refused(const char* what, int cl, int M, int cap, int A, int L, int D, int N, int app_dim, bool dims = true) {
  expect(what, expand(cl, M, cap, A, L, D, N, app_dim), 1);
  expect(what, search(cl, M, cap, A, L, D, N, app_dim, 4), 1);
  check(what, plan_dims_bad(M, A, L, N, app_dim, gnn_limits_cl(cl)) == dims);
}

static void validate() {
  for (int cl : {16, 64}) {
    const int app_max = cl / 2 - 4;
    expect("ok", expand(cl, 100, 901, 9, 20, 10, 3, 3), 0);
    expect("ok", search(cl, 100, 901, 9, 20, 10, 3, 3, 100), 0);
    expect("ok at the limits", expand(cl, 1, 65, 64, 1, 1, 6, app_max), 0);
    expect("ok at the limits", search(cl, 1, 65, 64, 1, 1, 6, app_max, 0), 0);
    expect("ok with one object", expand(cl, 3, 10, 9, 4, 2, 1, 0), 0);
    check("dimensions in range", !plan_dims_bad(3, 9, 4, 6, app_max, gnn_limits_cl(cl)));
    refused("N = 7", cl, 3, 22, 9, 4, 2, 7, 3);
    refused("N = 0", cl, 3, 22, 9, 4, 2, 0, 3);
    refused("app_dim one past the limit", cl, 3, 22, 9, 4, 2, 3, app_max + 1);
    refused("app_dim < 0", cl, 3, 22, 9, 4, 2, 3, -1);
    refused("A = 65", cl, 3, 100, 65, 4, 2, 3, 3);
    refused("M = 0", cl, 0, 22, 9, 4, 2, 3, 3);
    refused("L = 0", cl, 3, 22, 9, 0, 2, 3, 3);
    refused("rows x steps beyond an int's reach", cl, 1 << 20, 22, 9, 1 << 20, 2, 3, 3);
    refused("cap = A", cl, 3, 9, 9, 4, 2, 3, 3, false);
    refused("D = 0", cl, 3, 22, 9, 4, 0, 3, 3, false);
    expect("R < 0", search(cl, 3, 22, 9, 4, 2, 3, 3, -1), 1);
    // NULL pointers: (z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, ws, ...)
    const GnnLimits k = gnn_limits_cl(cl);
    expect("NULL z_pool", plan_expand(nullptr, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL leaf", plan_expand(f, nullptr, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL child", plan_expand(f, i, nullptr, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL len_s", plan_expand(f, i, i, nullptr, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL app with app_dim = 3", plan_expand(f, i, i, i, nullptr, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL app with app_dim = 0", plan_expand(f, i, i, i, nullptr, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 0, k), 0);
    expect("NULL acts", plan_expand(f, i, i, i, f, nullptr, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL emb_w", plan_expand(f, i, i, i, f, i, nullptr, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL emb_b", plan_expand(f, i, i, i, f, i, f, nullptr, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL gnn_params", plan_expand(f, i, i, i, f, i, f, f, nullptr, f, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL rh_params", plan_expand(f, i, i, i, f, i, f, f, f, nullptr, f, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL q", plan_expand(f, i, i, i, f, i, f, f, f, f, nullptr, ws, 3, 22, 9, 4, 2, 3, 3, k), 1);
    expect("NULL ws", plan_expand(f, i, i, i, f, i, f, f, f, f, f, nullptr, 3, 22, 9, 4, 2, 3, 3, k), 1);
    // (z_pool, first, parent, depth, Ns, Nsa, Qsa, used, min_gap, status, action, app, acts, emb_w, emb_b, gnn_params, rh_params, ws, ...)
    expect("search: NULL first", plan_search(f, nullptr, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL Qsa", plan_search(f, i, i, i, i, i, nullptr, i, d, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL min_gap", plan_search(f, i, i, i, i, i, d, i, nullptr, i, i, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL action", plan_search(f, i, i, i, i, i, d, i, d, i, nullptr, f, i, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL rh_params", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, nullptr, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL ws", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, i, f, f, f, f, nullptr, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL acts with R = 4", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, nullptr, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 4, k), 1);
    expect("search: NULL acts with R = 0", plan_search(f, i, i, i, i, i, d, i, d, i, i, f, nullptr, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3, 0, k), 0);
  }
  // the widths the `_cl` entry points do not serve: 32 has entry points of its own, 48 has no kernels
  for (int cl : {32, 48, 0, -16}) {
    refused("a width that is not served", cl, 3, 22, 9, 4, 2, 3, 3);
    expect("a width that is not served, R = 0", search(cl, 3, 22, 9, 4, 2, 3, 0, 0), 1);
  }
  // the cl = 32 calls keep their limits: eight objects, twelve appearance columns
  expect("cl = 32: N = 8, app_dim = 12", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 1, 65, 64, 1, 1, 8, 12), 0);
  expect("cl = 32: app_dim = 13", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 13), 1);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}); }
