"""The cases of the supervised baseline's GPU tests (tests/test_gpu_sup.py) and of the CPU test that holds their inputs to the
conditioning the GPU bars assume (tests/test_sup_cpu.py): seeded inputs, and sup_ref run in a given dtype."""
import torch

import sup_ref as S

NL = ('relu', 'leaky_relu')          # = leaky-relu and elu in the kernels (the reference's inverted selection)
DISCOUNT = 0.98
PRED_BAR_STEP, PRED_BAR_ROLLOUT = 2e-6, 3e-6          # the step and rollout bars of tests/test_gpu_dynamics_counts.py
GRAD_BARS = (3e-4, 3.5e-4, 4e-3)
MULT, CAP = 6.0, 10.0                # gpu_helpers.regime_bar lifts a bar to MULT x gap; no bar beyond CAP x its base

# (cl, N, B, V, R, fills): why each shape is here is the last column of the issue's table
SHAPES = [
    (16, 1, 1, 1, 1, ('analytic',)),          # no edges, no warm-up, one step, no delta term
    (16, 3, 11, 3, 4, ('init', 'half')),      # five sequences per workgroup, ragged last workgroup (one sequence)
    (16, 5, 7, 2, 3, ('init', 'half')),       # three per workgroup, 75 edge rows of 80
    (16, 6, 5, 2, 2, ('init', 'half')),       # two per workgroup, ragged
    (16, 3, 11, 6, 8, ('init', 'half')),      # the reference's V and R: 13 dependent steps
    (64, 2, 3, 3, 2, ('init', 'half')),       # one sequence per workgroup
    (64, 6, 2, 2, 3, ('init', 'half')),       # 36 of 48 edge rows, node rows past the 8th
    (64, 3, 4, 1, 1, ('analytic',)),          # one step at the wide layout
]
SEEDS = {}                           # (cl, N, B, V, R, fill, nonlinear) -> seed where the default one is ill-conditioned


def cases():
    """(cl, N, B, V, R, fill, nonlinear): every shape under each of its fills, the nonlinearities alternating so that both meet both"""
    out = []
    for i, (cl, N, B, V, R, fills) in enumerate(SHAPES):
        for j, fill in enumerate(fills):
            out.append((cl, N, B, V, R, fill, NL[(i + j) % 2]))
    return out


def case_id(case):
    return 'cl%d-n%d-B%d-V%d-R%d-%s-%s' % case


def one_step(case):
    return case[3] == 1 and case[4] == 1


def inputs(case):
    """float64 draws rounded to float32: x (B,V,N,4) and future (B,R,N,4) in the data set's scaling (positions in [0, 2], velocities
    within 0.4), latent0 (B,N,cl-4) standard normal, w (B,R,N,4) weights of a second loss"""
    cl, N, B, V, R, fill, nl = case
    seed = SEEDS.get(case, 31000 + 1000 * (cl // 16) + 100 * N + 10 * V + R + (7 if fill == 'half' else 0))
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    f32 = lambda t: t.float().double()          # noqa: E731

    def states(T):
        return torch.cat([2.0 * r(B, T, N, 2), 0.8 * r(B, T, N, 2) - 0.4], -1)
    return {'x': f32(states(V)), 'future': f32(states(R)), 'latent0': f32(torch.randn(B, N, cl - 4, generator=g, dtype=torch.float64)),
            'w': f32(r(B, R, N, 4))}


def ref_case(case, dtype, d=None):
    """sup_ref in `dtype` -> pred, codes, the three losses, and the gradients of the total and of (pred * w).sum() in every parameter
    and in latent0"""
    cl, N, B, V, R, fill, nl = case
    d = d if d is not None else inputs(case)
    c = S.sup_config(cl, nl, num_obj=N)
    params = S.sup_params(cl, fill, dtype)
    lat = d['latent0'].to(dtype).clone().requires_grad_()
    x, fut = d['x'].to(dtype), d['future'].to(dtype)
    pred, codes = S.sup_rollout_ref(c, params, x, lat, R, with_codes=True)
    losses = S.sup_loss_ref(pred, fut, DISCOUNT)
    leaves = list(params.values()) + [lat]
    names = list(params) + ['latent0']
    g_total = torch.autograd.grad(losses[0], leaves, retain_graph=True, allow_unused=True)
    g_w = torch.autograd.grad((pred * d['w'].to(dtype)).sum(), leaves, allow_unused=True)
    zero = lambda g, p: torch.zeros_like(p) if g is None else g          # noqa: E731
    return {'pred': pred.detach(), 'codes': codes.detach(), 'losses': [v.detach() for v in losses],
            'g_total': {k: zero(g, p) for k, g, p in zip(names, g_total, leaves)},
            'g_w': {k: zero(g, p) for k, g, p in zip(names, g_w, leaves)}}
