"""Generate the g20 fixtures: the reference's dynamics model and full model at state-code lengths cl = 16 and 64.

TEST INFRASTRUCTURE, run where the reference is installed (`python tools/make_goldens_cl.py [dynamics|stove|gap]`).  It borrows the
reference import, the analytic weight fill and the noise replay of oracle/make_goldens.py and writes only tests/golden/g20_*.
Weights are never stored: they are the formula fills of tests/golden/analytic_weights.py ('analytic' and 'init' regimes).

    g20_dynamics_cl{16,64}_{plain3,plain6,ac3}[_init]_f64.npz   as g5, inputs cl/2 wide, plus the state-dict inventory
    g20_stove_cl{16,64}_{n3,n6,ac3}[_init]_f64.npz              as g7: B = 2, T = 8, ELBO, p_*, every parameter gradient,
                                                                an 8-step rollout, the eps that were fed
    g20_reference_fp32_gap.json                                 the reference's float32 run against its float64 run, per case

The reference only accepts a width other than 32 when transition_lik_std has cl // 2 entries; [0.01] * (cl // 2) is used.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))

import numpy as np                    # noqa: E402
import torch                          # noqa: E402

import make_goldens as M              # noqa: E402  (imports the reference)

WIDTHS = (16, 64)
REGIMES = ('analytic', 'init')
DYN_VARIANTS = [
    ('plain3', dict(num_obj=3)),
    ('plain6', dict(num_obj=6)),
    ('ac3', dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True)),
]
STOVE_CASES = [
    ('n3', dict(num_obj=3)),
    ('n6', dict(num_obj=6, debug_match_objects='greedy', overlap_beta=100.0, max_obj_scale=0.22)),
    ('ac3', dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True)),
]


def width_cfg(cl):
    return dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


def save(name, **arrays):
    assert name.startswith('g20_')
    M.save(name, **arrays)


def inventory(module):
    """state-dict names and shapes (padded to two dims with zeros) as plain arrays"""
    sd = module.state_dict()
    names = np.array(list(sd.keys()))
    shapes = np.array([(list(v.shape) + [0, 0])[:2] for v in sd.values()], dtype=np.int64)
    return dict(sd_names=names, sd_shapes=shapes)


def dyn_case(cl, regime, kw, dtype):
    """One reference run of Dynamics.forward + backward in `dtype`; the inputs are drawn in float64 and cast."""
    c = M.ref_config(dtype, **kw, **width_cfg(cl))
    dyn = M.Dynamics(c)
    M.fill(dyn, 'dyn.', regime)
    g = torch.Generator().manual_seed(5 + cl)
    b, n_obj = 6, c.num_obj
    s = (torch.rand(b, n_obj, cl // 2, generator=g, dtype=torch.float64) * 1.6 - 0.8).to(dtype).requires_grad_()
    act = app = None
    if c.action_conditioned:
        act = torch.zeros(b, 9, dtype=dtype)
        act[torch.arange(b), torch.arange(b) % 9] = 1.0
        app = torch.rand(b, n_obj, 3, generator=g, dtype=torch.float64).to(dtype).requires_grad_()
    res, rew = dyn.forward(s, 0, act, app, lim_enc=2)
    w = torch.rand(res.shape, generator=g, dtype=torch.float64).to(dtype)
    loss = (res * w).sum()
    if c.action_conditioned:
        loss = loss + (rew * torch.linspace(1, 2, b, dtype=dtype).view(-1, 1)).sum()
    loss.backward()
    grads = {f'g_{k}': p.grad for k, p in dyn.named_parameters() if p.grad is not None}
    extra = {}
    if c.action_conditioned:
        extra = dict(actions=act, app=app, reward=rew, gapp=app.grad)
    out = dict(s=s, result=res, w=w, gs=s.grad, lim_enc=np.array(2), **inventory(dyn), **extra, **grads)
    return {k: M.np_(v) for k, v in out.items()}


def stove_case(cl, regime, kw, dtype):
    """One reference run of the full model (forward, backward, 8-step rollout) in `dtype` under float64-drawn noise."""
    tdn = M.tdn
    B, T = 2, 8
    lat_dim = cl // 2 - 4
    c = M.ref_config(dtype, **kw, **width_cfg(cl))
    c.debug = True
    N = c.num_obj
    st = M.Stove(c)
    M.fill(st, '', regime)
    x = torch.from_numpy(M.billiards_frames(B, T, n=N, r=1.2 if N == 3 else 1.0)).to(torch.float32).to(dtype)
    g = torch.Generator().manual_seed(123 + cl)
    lat = torch.randn(B, N, lat_dim, 1, generator=g, dtype=torch.float64)
    sd = torch.randn(B, N, lat_dim, 1, generator=g, dtype=torch.float64)
    steps = [torch.randn(B, N, cl // 2 + 2, generator=g, dtype=torch.float64) for _ in range(2, T)]
    actions = None
    if c.action_conditioned:
        actions = torch.zeros(B, T, 9, dtype=dtype)
        ai = torch.randint(0, 9, (B, T), generator=g)
        actions.scatter_(2, ai.unsqueeze(-1), 1.0)
    saved = tdn._standard_normal
    tdn._standard_normal = M.EpsFeeder([lat, sd] + steps)
    try:
        elbo, prop, rewards = st(x, 0, actions)
    finally:
        tdn._standard_normal = saved
    loss = -elbo
    if c.action_conditioned:
        loss = loss + 3.0 * (rewards ** 2).sum()
    loss.backward()
    gnorm = {f'gn_{k}': p.grad.norm() for k, p in st.named_parameters() if p.grad is not None}
    # the norm of every gradient; in full the dynamics model's up to cl x cl (what the new kernels produce) and the
    # small ones of the rest -- the 2 cl x cl layers in full would put the cl = 64 files above 1 MiB
    grads = {f'g_{k}': p.grad for k, p in st.named_parameters()
             if p.grad is not None and p.numel() <= (4200 if k.startswith('dyn.') else 2100)}
    props = {f'p_{k}': v for k, v in prop.items() if v is not None and torch.is_tensor(v)}
    extra = {}
    if actions is not None:
        extra['actions'] = actions
        extra['rewards'] = rewards
    with torch.no_grad():
        z_last = prop['z'][:, -1]
        fut = actions[:, :5] if actions is not None else None
        app = prop['obj_appearances'][:, -1] if actions is not None else None
        z_pred, r_pred = st.rollout(z_last, num=8, actions=fut, appearance=app)
    extra['roll_z'] = z_pred
    if actions is not None:
        extra['roll_rewards'] = r_pred
    out = dict(x=x.to(torch.float32), eps_lat=lat, eps_std=sd, eps_steps=torch.stack(steps, 0), elbo=elbo, **props, **gnorm, **grads, **extra)
    return {k: M.np_(v) for k, v in out.items()}


def cases():
    for cl in WIDTHS:
        for regime in REGIMES:
            yield cl, regime


def dynamics():
    for cl, regime in cases():
        for name, kw in DYN_VARIANTS:
            save(f'g20_dynamics_cl{cl}_{name}{M._rs(regime)}_f64', **dyn_case(cl, regime, kw, torch.float64))


def stove():
    for cl, regime in cases():
        for name, kw in STOVE_CASES:
            save(f'g20_stove_cl{cl}_{name}{M._rs(regime)}_f64', **stove_case(cl, regime, kw, torch.float64))


def gap():
    """The reference's own float32-against-float64 difference on every g20 case -> tests/golden/g20_reference_fp32_gap.json (the
    records and metrics of oracle/fp32_gap.py; the float32 runs are not kept).  What a parity bar that does not hold at a new
    width is set against (6 x the gap, tests/gpu_helpers.regime_bar)."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
    from gpu_helpers import err, err_l2, err_small

    def grads(a, b):
        ks = [k for k in a if k.startswith('g_') and k in b]
        return {'max': max(err(b[k], a[k]) for k in ks), 'l2': max(err_l2(b[k], a[k]) for k in ks),
                'small': max(err_small(b[k], a[k]) for k in ks)}
    out = {}
    for cl, regime in cases():
        for name, kw in DYN_VARIANTS:
            a, b = dyn_case(cl, regime, kw, torch.float64), dyn_case(cl, regime, kw, torch.float32)
            rec = {'result': err(b['result'], a['result']), 'gs': err(b['gs'], a['gs']), 'grad_param': grads(a, b)}
            if 'reward' in a:
                rec.update(reward=err(b['reward'], a['reward']), gapp=err(b['gapp'], a['gapp']))
            out[f'g20_dynamics_cl{cl}_{name}_{regime}'] = rec
        for name, kw in STOVE_CASES:
            a, b = stove_case(cl, regime, kw, torch.float64), stove_case(cl, regime, kw, torch.float32)
            e64, e32 = float(a['elbo']), float(b['elbo'])
            rec = {'elbo_f64': e64, 'elbo_rel': abs(e64 - e32) / abs(e64),
                   'grad_norm_rel_max': max(abs(float(a[k]) - float(b[k])) / (float(a[k]) + 1e-9) for k in a if k.startswith('gn_')),
                   'grad_tensor': grads(a, b),
                   'prop': {k[2:]: err(b[k], a[k]) for k in a if k.startswith('p_') and not np.isnan(a[k]).any()},
                   'rollout_z': err(b['roll_z'], a['roll_z'])}
            if 'rewards' in a:
                rec.update(rewards=err(b['rewards'], a['rewards']), rollout_rewards=err(b['roll_rewards'], a['roll_rewards']))
            out[f'g20_stove_cl{cl}_{name}_{regime}'] = rec
            print(f'g20_stove_cl{cl}_{name}_{regime}', flush=True)
    # the ragged-batch test of tests/test_gpu_cl.py draws its own inputs (seed 3, this order): the same draws through the reference
    RAGGED_PARAMS = ('out.0.0.weight', 'rel_cores.0.0.weight', 'att_net.0.2.bias', 'state_enc.weight', 'rel_cores.0.0.bias')
    for cl in WIDTHS:
        for n_obj in (3, 6):
            g = torch.Generator().manual_seed(3)
            for B in (1, 5, 64, 257):
                s64 = torch.rand(B, n_obj, cl // 2, generator=g, dtype=torch.float64) * 1.6 - 0.8
                w64 = torch.rand(B, n_obj, cl, generator=g, dtype=torch.float64)
                runs = []
                for dtype in (torch.float64, torch.float32):
                    dyn = M.Dynamics(M.ref_config(dtype, num_obj=n_obj, **width_cfg(cl)))
                    M.fill(dyn, 'dyn.', 'analytic')
                    s = s64.clone().to(dtype).requires_grad_()
                    res, _ = dyn.forward(s, 0, None, None, lim_enc=2)
                    (res * w64.to(dtype)).sum().backward()
                    named = dict(dyn.named_parameters())
                    runs.append(dict(result=M.np_(res), gs=M.np_(s.grad), **{'g_' + k: M.np_(named[k].grad) for k in RAGGED_PARAMS}))
                a, b = runs
                out[f'ragged_cl{cl}_n{n_obj}_B{B}'] = {'result': err(b['result'], a['result']), 'gs': err(b['gs'], a['gs']),
                                                      'grad_param': grads(a, b)}
    # the T = 100 on-box test of tests/test_gpu_cl.py (B = 8, the project's own synthetic frames, seed 77 + cl, 92-step rollout from the
    # float64 run's last state): the same inputs through the reference
    sys.path.insert(0, os.path.dirname(HERE))
    from stove_amd.envs import envs as own_envs
    tdn = M.tdn
    for cl in WIDTHS:
        for name, kw in STOVE_CASES[:2]:
            B, T, N = 8, 100, kw['num_obj']
            x32 = torch.from_numpy(own_envs.synth_sequences('billiards' if N == 3 else 'multibilliards', B, T, seed0=900)['X']).float()
            g = torch.Generator().manual_seed(77 + cl)
            lat = torch.randn(B, N, cl // 2 - 4, 1, generator=g, dtype=torch.float64)
            sd = torch.randn(B, N, cl // 2 - 4, 1, generator=g, dtype=torch.float64)
            steps = [torch.randn(B, N, cl // 2 + 2, generator=g, dtype=torch.float64) for _ in range(2, T)]
            runs, z_last = [], None
            for dtype in (torch.float64, torch.float32):
                c = M.ref_config(dtype, **kw, **width_cfg(cl))
                c.debug = True
                st = M.Stove(c)
                M.fill(st, '', 'analytic')
                saved = tdn._standard_normal
                tdn._standard_normal = M.EpsFeeder([lat, sd] + steps)
                try:
                    elbo, prop, _ = st(x32.to(dtype), 0, None)
                finally:
                    tdn._standard_normal = saved
                (-elbo).backward()
                if z_last is None:
                    z_last = prop['z'][:, -1].detach().double()
                with torch.no_grad():
                    roll, _ = st.rollout(z_last.to(dtype), num=92)
                runs.append(dict(elbo=M.np_(elbo), roll=M.np_(roll), **{'p_' + k: M.np_(prop[k]) for k in ('z', 'z_dyn', 'z_sup')},
                                 **{'g_' + k: M.np_(p.grad) for k, p in st.named_parameters() if p.grad is not None}))
            a, b = runs
            out[f'T100_cl{cl}_{name}'] = {'elbo_rel': abs(float(a['elbo']) - float(b['elbo'])) / abs(float(a['elbo'])),
                                          'prop': {k: err(b['p_' + k], a['p_' + k]) for k in ('z', 'z_dyn', 'z_sup')},
                                          'grad_tensor': grads(a, b), 'rollout_z': err(b['roll'], a['roll'])}
            print(f'T100_cl{cl}_{name}', out[f'T100_cl{cl}_{name}'], flush=True)
    torch.set_default_dtype(torch.float32)
    path = os.path.join(M.OUT, 'g20_reference_fp32_gap.json')
    with open(path, 'w') as f:
        json.dump({'what': "the reference's own float32-vs-float64 gap on the g20 fixtures (cl = 16 / 64): max |a-b| / max |b| unless named "
                           "otherwise; l2 / small: tests/gpu_helpers.err_l2 / err_small.  From tools/make_goldens_cl.py gap.",
                   'gaps': out}, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    which = sys.argv[1:] or ['dynamics', 'stove', 'gap']
    for w in which:
        {'dynamics': dynamics, 'stove': stove, 'gap': gap}[w]()
