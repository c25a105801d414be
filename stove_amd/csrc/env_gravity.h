// One gravity environment's step (stove_amd/envs/envs.py: PhysicsEnv.step with mass_center_obs + GravityEnv.simulate_physics -- that
// file is the specification) on ONE environment's rows, in float64, in the manner of env_step.h: __host__ __device__ under hipcc (the
// kernel of env_sequences.hip calls these functions), unmarked under a host compiler (tests/abi/env_sequences_driver.cpp runs the same
// text on the CPU under sanitizers).  The state must equal stove_amd/envs/synth.py's numpy arithmetic bit for bit: every operation is
// an IEEE double add, multiply, divide or sqrt in the order written here, and none may be contracted.  Two restatements of envs.py
// are deliberate: norms are sqrt(a a + b b) where envs.py calls BLAS, and cubes are d * d * d where numpy's `** 3` calls pow, whose
// last bit a device cannot be made to reproduce.
// A substep is written as pieces per ball (moved, mass_sums, shift, shifted, slowed, attract, to_middle, clipped, pushed), so that the serial form below and a
// kernel that holds one ball per lane run the same text.
#pragma once
#include "env_step.h"

namespace env_gravity {

constexpr int kMaxObjects = env_step::kMaxObjects;
constexpr double kG = 0.5, kSoftening = 1e-5, kPull = 0.001;

// x += t eps v
ENV_STEP_FN double moved(double x, double v, double te) {
  ENV_STEP_NO_CONTRACT
  return x + te * v;
}

// sum(m x) per axis and sum(m), taken in ball order
ENV_STEP_FN void mass_sums(const double* x, const double* m, int N, double* s0, double* s1, double* sm) {
  ENV_STEP_NO_CONTRACT
  double a0 = m[0] * x[0], a1 = m[0] * x[1], am = m[0];
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 1; i < kMaxObjects; ++i)          // (a constant trip count: rows held in registers stay there)
    if (i < N) {
      a0 = a0 + m[i] * x[2 * i];
      a1 = a1 + m[i] * x[2 * i + 1];
      am = am + m[i];
    }
  *s0 = a0;
  *s1 = a1;
  *sm = am;
}

// the centre-of-mass shift of one axis, hw / 2 - sum(m x) / sum(m), and x += shift
ENV_STEP_FN double shift(double hw, double smx, double sm) {
  ENV_STEP_NO_CONTRACT
  return hw / 2.0 - smx / sm;
}
ENV_STEP_FN double shifted(double x, double d) {
  ENV_STEP_NO_CONTRACT
  return x + d;
}

// v -= fric m v t eps
ENV_STEP_FN double slowed(double v, double m, double fric, double t, double eps) {
  ENV_STEP_NO_CONTRACT
  return v - fric * m * v * t * eps;
}

// force -= G m_j m_i (x_i - x_j) / (|x_j - x_i| + 1e-5)^3
ENV_STEP_FN void attract(double* f, double xi0, double xi1, double xj0, double xj1, double mi, double mj) {
  ENV_STEP_NO_CONTRACT
  const double a0 = xj0 - xi0, a1 = xj1 - xi1;
  const double d = sqrt(a0 * a0 + a1 * a1) + kSoftening;
  const double cube = d * d * d;
  const double g = kG * mj * mi;
  f[0] = f[0] - g * (xi0 - xj0) / cube;
  f[1] = f[1] - g * (xi1 - xj1) / cube;
}

// force += 0.001 (mid - x_i)^3 / |mid - x_i|
ENV_STEP_FN void to_middle(double* f, double xi0, double xi1, double hw) {
  ENV_STEP_NO_CONTRACT
  const double mid = hw / 2.0;
  const double c0 = mid - xi0, c1 = mid - xi1;
  const double n = sqrt(c0 * c0 + c1 * c1);
  f[0] = f[0] + kPull * (c0 * c0 * c0) / n;
  f[1] = f[1] + kPull * (c1 * c1 * c1) / n;
}

ENV_STEP_FN double clipped(double f) { return f < -1.0 ? -1.0 : (f > 1.0 ? 1.0 : f); }

// v_i + (force / m_i) t eps
ENV_STEP_FN double pushed(double v, double f, double m, double t, double eps) {
  ENV_STEP_NO_CONTRACT
  return v + (f / m) * t * eps;
}

// One substep of all N balls, in place
ENV_STEP_FN void substep(double* x, double* v, const double* m, const env_step::Params& p, double eps) {
  ENV_STEP_NO_CONTRACT
  const int N = p.N;
  const double te = p.t * eps;
  for (int k = 0; k < 2 * N; ++k) x[k] = moved(x[k], v[k], te);
  double s0, s1, sm;
  mass_sums(x, m, N, &s0, &s1, &sm);
  const double d0 = shift(p.hw, s0, sm), d1 = shift(p.hw, s1, sm);
  for (int i = 0; i < N; ++i) {
    x[2 * i] = shifted(x[2 * i], d0);
    x[2 * i + 1] = shifted(x[2 * i + 1], d1);
  }
  for (int k = 0; k < 2 * N; ++k) v[k] = slowed(v[k], m[k >> 1], p.fric, p.t, eps);
  for (int i = 0; i < N; ++i) {          // (x is read only from here on, and v[i] depends on nothing but itself: in place)
    double f[2] = {0.0, 0.0};
    for (int j = 0; j < N; ++j)
      if (j != i) attract(f, x[2 * i], x[2 * i + 1], x[2 * j], x[2 * j + 1], m[i], m[j]);
    to_middle(f, x[2 * i], x[2 * i + 1], p.hw);
    for (int ax = 0; ax < 2; ++ax) v[2 * i + ax] = pushed(v[2 * i + ax], clipped(f[ax]), m[i], p.t, eps);
  }
}

// One environment step: `granularity` substeps
ENV_STEP_FN void step(double* x, double* v, const double* m, const env_step::Params& p) {
  ENV_STEP_NO_CONTRACT
  const double eps = 1.0 / (double)p.granularity;
  for (int s = 0; s < p.granularity; ++s) substep(x, v, m, p, eps);
}

// the number of position coordinates strictly inside (0, hw): generate_fitting_run's count of one recorded state
ENV_STEP_FN int inside(const double* x, int N, double hw) {
  int n = 0;
  for (int k = 0; k < 2 * N; ++k) n += (x[k] > 0.0 && x[k] < hw) ? 1 : 0;
  return n;
}

}  // namespace env_gravity
