"""Shared helpers for the parity tests (oracle side)."""
import copy
import os

import numpy as np
import torch

import stove_oracle as O
from analytic_weights import analytic_tensor, fan_ins

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def oracle_setup(dtype=torch.float64, requires_grad=True, regime='analytic', **cfg):
    """config + SPN structures + analytic parameters (weight regime `regime`) keyed by reference state-dict names."""
    c = O.default_config(**cfg)
    structs = O.build_structs(c)
    shapes = O.param_shapes(c, structs)
    fi = fan_ins({k: tuple(v) for k, v in shapes.items()})
    params = {}
    for k, shp in shapes.items():
        t = analytic_tensor(k, shp, dtype, regime, fi.get(k))
        params[k] = t.requires_grad_() if requires_grad else t
    return c, structs, params


def t_(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def reference_at_codes(gold, regime, cfg, codes):
    """The float64 oracle (pinned to the reference on this very fixture, tests/test_oracle_goldens.py) evaluated AT the codes another
    implementation's recognition network produced: a dict with the golden fixture's keys (elbo, p_*, gn_*, g_*, roll_*), everything
    the oracle does not restate (bg / patch / overlap means) copied from `gold`.  For the 'stress' regime, whose six-step recursion and
    its gradients amplify a 1e-5 difference of the codes to 1e-4 in z and 1e-2 in the dynamics' gradients: the recognition network is
    held to the fixture's codes by its own test, everything behind it to the reference at the same codes."""
    dtype = torch.float64
    c, structs, params = oracle_setup(dtype, regime=regime, **cfg)
    x = t_(gold['x'], dtype)
    eps = {'latent': t_(gold['eps_lat'], dtype), 'std': t_(gold['eps_std'], dtype), 'steps': [t_(e, dtype) for e in gold['eps_steps']]}
    actions = t_(gold['actions'], dtype) if 'actions' in gold else None
    elbo, rewards, info = O.stove_forward(c, params, structs, x, eps, actions, detail=True, code_values=codes.detach().double().cpu())
    loss = -elbo
    if actions is not None:
        loss = loss + 3.0 * (rewards ** 2).sum()
    loss.backward()
    out = dict(gold)
    out['elbo'] = elbo.detach().numpy()
    for k in ('z', 'z_dyn', 'z_sup', 'z_std', 'z_sup_std', 'log_q', 'translik'):
        out['p_' + k] = info[k].detach().numpy()
    nan2 = np.full(2, np.nan)
    out['p_z_dyn_std'] = np.concatenate([nan2, info['z_dyn_std'].detach().numpy()])
    if actions is not None:
        out['rewards'] = rewards.detach().numpy()
        out['p_obj_appearances'] = info['obj_appearances'].detach().numpy()
    for k in list(gold):
        if k.startswith('gn_'):
            out[k] = params[k[3:]].grad.norm().numpy()
        elif k.startswith('g_'):
            out[k] = params[k[2:]].grad.numpy()
    with torch.no_grad():
        z_last = info['z'].detach()[:, -1]
        fut = actions[:, :5] if actions is not None else None
        app = info['obj_appearances'].detach()[:, -1] if actions is not None else None
        zp, rp = O.rollout(c, params, z_last, gold['roll_z'].shape[1], fut, app)
        out['roll_z'] = zp.numpy()
        if actions is not None:
            out['roll_rewards'] = rp.numpy()
        if 'eps_roll' in gold:
            zs, lq, _ = O.rollout(c, params, z_last, gold['roll_s_z'].shape[1], eps=[t_(e, dtype) for e in gold['eps_roll']])
            out['roll_s_z'], out['roll_s_logq'] = zs.numpy(), lq.numpy()
    return out


def source_index(z, zm, tol=1e-6):
    """idx[b, t, slot] = k with zm[b, t, slot] == z[b, t, k] (to `tol`): the permutation a matcher applied, recovered from its
    output; every matched row must be exactly one source row (rows of the test tracks differ in their first two columns)."""
    z, zm = torch.as_tensor(z).double().cpu(), torch.as_tensor(zm).double().cpu()
    eq = ((zm.unsqueeze(3) - z.unsqueeze(2)).abs() < tol).all(-1)
    assert bool((eq.sum(-1) == 1).all()), 'a matched row is not exactly one source row'
    return eq.long().argmax(-1)


def replica_index(n, K, seed=0):
    """src[row] = the distinct item (0 .. K-1) that row `row` of an n-row batch holds: item k on ceil / floor(n / K) rows (exactly
    R rows for n = K R), placed by a fixed random permutation.  The placement has no period and no block structure, so a kernel that
    reads row r +- s or row r mod m instead of row r reads another item on nearly every row (tests/test_batch_replication_cpu.py)."""
    g = np.random.default_rng(seed)
    return np.arange(n, dtype=np.int64)[g.permutation(n)] % K


def replica_counts(src, K):
    """how many rows hold each item: the factor of an item's share of a batch-summed gradient"""
    return np.bincount(np.asarray(src), minlength=K)


def oracle_stove(cfg, x, eps, actions=None, regime='analytic', dtype=torch.float64):
    """The float64 oracle's training step on one batch: loss = -ELBO (+ 3 mean(rewards^2) with actions, a batch mean like the ELBO,
    so that the loss of a replicated batch is the loss of its distinct sequences) -> dict(elbo, rewards, info, grads)."""
    c, structs, params = oracle_setup(dtype, regime=regime, **cfg)
    act = actions.to(dtype) if actions is not None else None
    eps = {'latent': eps['latent'].to(dtype), 'std': eps['std'].to(dtype), 'steps': [e.to(dtype) for e in eps['steps']]}
    elbo, rewards, info = O.stove_forward(c, params, structs, x.to(dtype), eps, act, detail=True)
    loss = -elbo
    if act is not None:
        loss = loss + 3.0 * (rewards ** 2).mean()
    loss.backward()
    return {'c': c, 'params': params, 'elbo': elbo.detach(), 'rewards': rewards.detach() if act is not None else None,
            'info': {k: (v.detach() if torch.is_tensor(v) else v) for k, v in info.items()},
            'grads': {k: p.grad for k, p in params.items() if p.grad is not None}}


def replicate_eps(eps, src):
    """the oracle's noise draws (O.draw_eps) of K sequences, row b of the result = row src[b]"""
    idx = torch.as_tensor(np.asarray(src))
    return {'latent': eps['latent'][idx], 'std': eps['std'][idx], 'steps': [e[idx] for e in eps['steps']]}


# ------------------------------------------------------------------------------------------------ dynamics at every object count
# Inputs of tests/test_oracle_counts_cpu.py and tests/test_gpu_dynamics_counts.py: drawn in float64 from a seeded CPU generator, nothing
# symmetric between the objects (every object its own position, scale and appearance row: a swapped or dropped edge changes the numbers).
DYN_VARIANTS = {
    'plain': {},                                                                            # cl/2 inputs per node
    'act': dict(action_conditioned=True, action_space=9),                                   # cl/2 + 4: actions without appearance
    'actapp': dict(action_conditioned=True, action_space=9, debug_core_appearance=True),    # cl/2 + 7
}


def dyn_width_cfg(cl):
    return {} if cl == 32 else dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


_DYN_ORACLES = {}


def dyn_oracle(cl, n_obj, variant, regime='analytic', dtype=torch.float64, nonlinear='relu'):
    """(config, the 'dyn.' parameters) of the oracle at one width / object count / input variant / weight regime: the parameters are
    built once and shared (they carry requires_grad; whoever differentiates clears their .grad first), the config is the caller's."""
    key = (cl, n_obj, variant, regime, dtype)
    if key not in _DYN_ORACLES:
        c, _, params = oracle_setup(dtype, regime=regime, num_obj=n_obj, **DYN_VARIANTS[variant], **dyn_width_cfg(cl))
        _DYN_ORACLES[key] = (c, {k: v for k, v in params.items() if k.startswith('dyn.')})
    c, params = _DYN_ORACLES[key]
    c = copy.copy(c)
    c.debug_nonlinear = nonlinear
    return c, params


def embed_actions(params, actions, n_obj):
    """one-hot actions (..., A) -> the action embedding's rows (..., n_obj, 4), as dynamics_forward appends them to the state"""
    return O._lin(params, 'dyn.action_embedding_layer', actions).view(*actions.shape[:-1], n_obj, 4)


def dyn_state(g, B, n_obj, cl, lo=-0.8, hi=0.8):
    """(B, N, cl/2) core inputs [x, y, vx, vy, latents] in [lo, hi]"""
    return torch.rand(B, n_obj, cl // 2, generator=g, dtype=torch.float64) * (hi - lo) + lo


def dyn_actions(g, variant, *lead):
    """one-hot actions (*lead, 9) in float64, or None for the plain variant"""
    if variant == 'plain':
        return None
    return torch.nn.functional.one_hot(torch.randint(0, 9, lead, generator=g), 9).double()


def dyn_appearance(g, variant, *lead):
    """appearance rows (*lead, 3) in [0, 1], or None"""
    return torch.rand(*lead, 3, generator=g, dtype=torch.float64) if variant == 'actapp' else None


def dyn_recursion_inputs(g, B, Ts, n_obj, cl):
    """-> z1 (B,N,cl/2+2), zsup, zsstd (B,Ts,N,6), eps (B,Ts,N,cl/2+2): scales in [0.15, 0.6], z1's positions in [-0.8, 0.8] (its
    velocities and latents in [-0.3, 0.3]), SuPAIR means in [-0.9, 0.9] with scales in [0.15, 0.6], stds in [0.02, 0.3]"""
    D = cl // 2
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    z1 = torch.cat([r(B, n_obj, 2) * 0.45 + 0.15, r(B, n_obj, 2) * 1.6 - 0.8, r(B, n_obj, D - 2) * 0.6 - 0.3], -1)
    zsup = torch.cat([r(B, Ts, n_obj, 2) * 0.45 + 0.15, r(B, Ts, n_obj, 4) * 1.8 - 0.9], -1)
    zsstd = r(B, Ts, n_obj, 6) * 0.28 + 0.02
    eps = torch.randn(B, Ts, n_obj, D + 2, generator=g, dtype=torch.float64)
    return z1, zsup, zsstd, eps
