// Host-only driver of stove_plan_expand's argument check (stove_amd/csrc/validate.h: plan_expand, plan_dims_bad), built with
// -fsanitize=address,undefined by tests/test_mcts_cpu.py, in the manner of validate_driver.cpp: fake, never-mapped "device"
// pointers that the layer must not dereference.  `plan_validate_driver validate`: one line per failure, exit status = number of failures.
#include <cstdio>
#include <cstdint>

#include "driver.h"

using namespace stove_validate;

static void validate() {
  const float* f = dev<const float>(1);
  const int* i = dev<const int>(2);
  void* ws = dev<void>(3);
  // (z_pool, leaf, child, len_s, app, acts, emb_w, emb_b, gnn_params, rh_params, q, ws, M, cap, A, L, D, N, app_dim)
  expect("ok", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 100, 901, 9, 20, 10, 3, 3), 0);
  expect("ok without appearance", plan_expand(f, i, i, i, nullptr, i, f, f, f, f, f, ws, 3, 10, 9, 4, 2, 3, 0), 0);
  expect("ok at the limits", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 1, 65, 64, 1, 1, 8, 12), 0);
  expect("NULL z_pool", plan_expand(nullptr, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL leaf", plan_expand(f, nullptr, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL child", plan_expand(f, i, nullptr, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL len_s", plan_expand(f, i, i, nullptr, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL app with app_dim = 3", plan_expand(f, i, i, i, nullptr, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL acts", plan_expand(f, i, i, i, f, nullptr, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL emb_w", plan_expand(f, i, i, i, f, i, nullptr, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL emb_b", plan_expand(f, i, i, i, f, i, f, nullptr, f, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL gnn_params", plan_expand(f, i, i, i, f, i, f, f, nullptr, f, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL rh_params", plan_expand(f, i, i, i, f, i, f, f, f, nullptr, f, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL q", plan_expand(f, i, i, i, f, i, f, f, f, f, nullptr, ws, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("NULL ws", plan_expand(f, i, i, i, f, i, f, f, f, f, f, nullptr, 3, 22, 9, 4, 2, 3, 3), 1);
  expect("M = 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 0, 22, 9, 4, 2, 3, 3), 1);
  expect("A = 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 0, 4, 2, 3, 3), 1);
  expect("A = 65", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 100, 65, 4, 2, 3, 3), 1);
  expect("L = 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 0, 2, 3, 3), 1);
  expect("D = 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 0, 3, 3), 1);
  expect("N = 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 0, 3), 1);
  expect("N = 9", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 9, 3), 1);
  expect("app_dim = 13 (more than 32 inputs per node)", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, 13), 1);
  expect("app_dim < 0", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 22, 9, 4, 2, 3, -1), 1);
  expect("cap = A", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 3, 9, 9, 4, 2, 3, 3), 1);
  expect("rows x steps beyond an int's reach", plan_expand(f, i, i, i, f, i, f, f, f, f, f, ws, 1 << 20, 22, 9, 1 << 20, 2, 3, 3), 1);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}); }
