// Host-only driver of the argument checks of stove_ppo_collect_model_cl (stove_amd/csrc/validate.h: ppo_collect_model_cl run with
// gnn_limits_cl(cl)), built with -fsanitize=address,undefined by tests/test_ppo_model_cl_cpu.py, in the manner of
// plan_cl_validate_driver.cpp: fake, never-mapped "device" pointers that the layer must not dereference.
// `ppo_model_cl_validate_driver validate`: one line per failure, exit status = number of failures.
#include <cstdio>
#include <cstdint>

#include "driver.h"

using namespace stove_validate;

static const float* f = dev<const float>(1);
static const int* i = dev<const int>(2);
static const float* nf = nullptr;
static const int* ni = nullptr;

// (cl, B, S, N, H, app_dim, lim_enc) with every pointer given
static int call(int cl, int B, int S, int N, int H, int app_dim, int lim_enc) {
  return ppo_collect_model_cl(f, f, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, B, S, N, H, app_dim, lim_enc, gnn_limits_cl(cl));
}

static void validate() {
  for (int cl : {16, 64}) {
    const int app_max = cl / 2 - 4;
    const GnnLimits k = gnn_limits_cl(cl);
    expect("ok", call(cl, 32, 128, 3, 64, 3, 2), 0);
    expect("ok at N = 1, H = 1, no appearance", ppo_collect_model_cl(f, nf, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, 1, 1, 1, 1, 0, 0, k), 0);
    expect("ok at N = 6, H = 128, the widest appearance, lim_enc = cl", call(cl, 256, 128, 6, 128, app_max, cl), 0);
    // the two empty-call forms
    expect("B = 0 (an empty batch has no arrays)",
           ppo_collect_model_cl(nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 128, 3, 64, 3, 2, k), 0);
    expect("S = 0 (no table, no step rows)", ppo_collect_model_cl(f, f, f, f, f, f, f, nf, nf, f, ni, nf, nf, nf, f, nf, i, 4, 0, 3, 64, 3, 2, k), 0);
    // a NULL required array: (z0, app, policy_params, emb_w, emb_b, gnn_params, rh_params, u, z_pred, obs | actions | rewards, values,
    // logp, next_value, returns | status)
    for (int drop = 0; drop < 17; ++drop) {
      const float* ff[15];
      const int* ii[2] = {i, i};
      for (int q = 0; q < 15; ++q) ff[q] = f;
      if (drop < 10) ff[drop] = nullptr;
      else if (drop == 10) ii[0] = nullptr;
      else if (drop < 16) ff[drop - 1] = nullptr;
      else ii[1] = nullptr;
      expect("a NULL array", ppo_collect_model_cl(ff[0], ff[1], ff[2], ff[3], ff[4], ff[5], ff[6], ff[7], ff[8], ff[9], ii[0], ff[10], ff[11], ff[12],
                                                  ff[13], ff[14], ii[1], 3, 5, 3, 64, 3, 2, k), 1);
    }
    expect("NULL app with app_dim = 0", ppo_collect_model_cl(f, nf, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, 3, 5, 3, 64, 0, 2, k), 0);
    expect("B = -1", call(cl, -1, 5, 3, 64, 3, 2), 1);
    expect("S = -1", call(cl, 3, -1, 3, 64, 3, 2), 1);
    expect("N = 0", call(cl, 3, 5, 0, 64, 3, 2), 1);
    expect("N = 7", call(cl, 3, 5, 7, 64, 3, 2), 1);
    expect("H = 0", call(cl, 3, 5, 3, 0, 3, 2), 1);
    expect("H = 129", call(cl, 3, 5, 3, 129, 3, 2), 1);
    expect("app_dim = -1", call(cl, 3, 5, 3, 64, -1, 2), 1);
    expect("app_dim one past cl/2 - 4", call(cl, 3, 5, 3, 64, app_max + 1, 2), 1);
    expect("app_dim = INT32_MAX", call(cl, 3, 5, 3, 64, INT32_MAX, 2), 1);
    expect("lim_enc = -1", call(cl, 3, 5, 3, 64, 3, -1), 1);
    expect("lim_enc = cl + 1", call(cl, 3, 5, 3, 64, 3, cl + 1), 1);
    expect("N = 7 at B = 0", ppo_collect_model_cl(nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, ni, nf, nf, nf, nf, nf, ni, 0, 5, 7, 64, 3, 2, k), 1);
    // the 32-bit size guard: B (S + 1) N cl has to stay an int
    expect("B (S + 1) N cl past int", call(cl, 1 << 20, 1 << 10, 6, 64, 3, 2), 1);
    expect("B (S + 1) N cl just within int", call(cl, 0x7fffffff / (129 * 6 * cl), 128, 6, 64, 3, 2), 0);
    expect("B (S + 1) N cl just past int", call(cl, 0x7fffffff / (129 * 6 * cl) + 1, 128, 6, 64, 3, 2), 1);
  }
  // the widths this entry point does not serve: 32 has an entry point of its own, 48 has no kernels
  for (int cl : {32, 48, 0, -16}) {
    expect("a width that is not served", call(cl, 3, 5, 3, 64, 3, 2), 1);
    expect("a width that is not served, B = 0", call(cl, 0, 5, 3, 64, 0, 0), 1);
  }
  // the cl = 32 call keeps its limits: twelve appearance columns, lim_enc up to 32
  expect("cl = 32: app_dim = 12", ppo_collect_model(f, f, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, 3, 5, 3, 64, 12, 32), 0);
  expect("cl = 32: app_dim = 13", ppo_collect_model(f, f, f, f, f, f, f, f, f, f, i, f, f, f, f, f, i, 3, 5, 3, 64, 13, 2), 1);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}); }
