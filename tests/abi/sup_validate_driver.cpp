// Host-only driver of the argument checks of stove_sup_rollout_fwd / stove_sup_rollout_bwd / stove_sup_loss (stove_amd/csrc/validate.h:
// sup_dims_bad, sup_rollout_fwd, sup_rollout_bwd, sup_loss), built with -fsanitize=address,undefined by tests/test_sup_cpu.py, in the
// manner of plan_cl_validate_driver.cpp: fake, never-mapped "device" pointers that the layer must not dereference.  Where sup_dims_bad
// holds the workspace query returns 0 (csrc/capi.hip); the CPU test asks the library for that.
// `sup_validate_driver validate`: one line per failure, exit status = number of failures.
#include <cstdio>
#include <cstdint>

#include "driver.h"

using namespace stove_validate;

static const float* f = dev<const float>(1);
static void* ws = dev<void>(2);

// (cl, B, V, R, N) with every pointer given
static int fwd(int cl, int B, int V, int R, int N) { return sup_rollout_fwd(f, f, f, f, cl, B, V, R, N); }
static int bwd(int cl, int B, int V, int R, int N) { return sup_rollout_bwd(f, f, f, f, f, ws, cl, B, V, R, N); }
static void refused(const char* what, int cl, int B, int V, int R, int N) {
  expect(what, fwd(cl, B, V, R, N), 1);
  expect(what, bwd(cl, B, V, R, N), 1);
  check(what, sup_dims_bad(cl, B, V, R, N));
}

static void validate() {
  for (int cl : {16, 64}) {
    expect("ok", fwd(cl, 256, 6, 8, 3), 0);
    expect("ok", bwd(cl, 256, 6, 8, 3), 0);
    expect("ok at the limits", fwd(cl, 1, 1, 1, 6), 0);
    expect("ok at the limits", bwd(cl, 1, 1, 1, 1), 0);
    expect("a long rollout", fwd(cl, 10, 6, 500, 3), 0);
    check("dimensions in range", !sup_dims_bad(cl, 11, 3, 4, 6));
    refused("N = 7", cl, 4, 3, 4, 7);
    refused("N = 0", cl, 4, 3, 4, 0);
    refused("V = 0", cl, 4, 0, 4, 3);
    refused("R = 0", cl, 4, 3, 0, 3);
    refused("B < 0", cl, -1, 3, 4, 3);
    refused("more steps than an int counts", cl, 4, 0x7fffffff, 2, 3);
    // B == 0: a valid empty call; the forward needs no pointer, the backward g_params alone (it is zeroed)
    expect("empty forward", sup_rollout_fwd(nullptr, nullptr, nullptr, nullptr, cl, 0, 3, 4, 3), 0);
    expect("empty backward", sup_rollout_bwd(nullptr, nullptr, nullptr, nullptr, f, nullptr, cl, 0, 3, 4, 3), 0);
    expect("empty backward: NULL g_params", sup_rollout_bwd(f, f, f, f, nullptr, ws, cl, 0, 3, 4, 3), 1);
    // NULL pointers: (x, latent0, params, pred, ...) -- codes is optional and not part of the check
    expect("NULL x", sup_rollout_fwd(nullptr, f, f, f, cl, 4, 3, 4, 3), 1);
    expect("NULL latent0", sup_rollout_fwd(f, nullptr, f, f, cl, 4, 3, 4, 3), 1);
    expect("NULL params", sup_rollout_fwd(f, f, nullptr, f, cl, 4, 3, 4, 3), 1);
    expect("NULL pred", sup_rollout_fwd(f, f, f, nullptr, cl, 4, 3, 4, 3), 1);
    // (x, params, codes, d_pred, g_params, ws, ...) -- d_latent0 is optional and not part of the check
    expect("bwd: NULL x", sup_rollout_bwd(nullptr, f, f, f, f, ws, cl, 4, 3, 4, 3), 1);
    expect("bwd: NULL params", sup_rollout_bwd(f, nullptr, f, f, f, ws, cl, 4, 3, 4, 3), 1);
    expect("bwd: NULL codes", sup_rollout_bwd(f, f, nullptr, f, f, ws, cl, 4, 3, 4, 3), 1);
    expect("bwd: NULL d_pred", sup_rollout_bwd(f, f, f, nullptr, f, ws, cl, 4, 3, 4, 3), 1);
    expect("bwd: NULL g_params", sup_rollout_bwd(f, f, f, f, nullptr, ws, cl, 4, 3, 4, 3), 1);
    expect("bwd: NULL ws", sup_rollout_bwd(f, f, f, f, f, nullptr, cl, 4, 3, 4, 3), 1);
  }
  // the widths these entry points do not serve: 32 has no width-generic instantiation, 48 has no kernels
  for (int cl : {32, 48, 0, -16}) refused("a width that is not served", cl, 4, 3, 4, 3);
  // the loss: (pred, future, losses, d_pred, B, R, N, end)
  expect("loss ok", sup_loss(f, f, f, f, 256, 8, 3, 4), 0);
  expect("loss ok, positions only, one step", sup_loss(f, f, f, f, 1, 1, 6, 2), 0);
  expect("loss: end = 3", sup_loss(f, f, f, f, 4, 4, 3, 3), 1);
  expect("loss: end = 0", sup_loss(f, f, f, f, 4, 4, 3, 0), 1);
  expect("loss: B = 0", sup_loss(f, f, f, f, 0, 4, 3, 4), 1);
  expect("loss: R = 0", sup_loss(f, f, f, f, 4, 0, 3, 4), 1);
  expect("loss: N = 0", sup_loss(f, f, f, f, 4, 4, 0, 4), 1);
  expect("loss: N = 7", sup_loss(f, f, f, f, 4, 4, 7, 4), 1);
  expect("loss: more entries than an int counts", sup_loss(f, f, f, f, 1 << 20, 1 << 10, 3, 4), 1);
  expect("loss: NULL pred", sup_loss(nullptr, f, f, f, 4, 4, 3, 4), 1);
  expect("loss: NULL future", sup_loss(f, nullptr, f, f, 4, 4, 3, 4), 1);
  expect("loss: NULL losses", sup_loss(f, f, nullptr, f, 4, 4, 3, 4), 1);
  expect("loss: NULL d_pred", sup_loss(f, f, f, nullptr, 4, 4, 3, 4), 1);
}

int main(int argc, char** argv) { return driver_main(argc, argv, {{"validate", validate}}); }
