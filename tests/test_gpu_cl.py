"""GPU parity tests of the width-generic GNN kernels (csrc/gnn_cl.hip) at state-code lengths 16 and 64: the step forward / backward,
the one-launch recursion and rollout, and the full model, against the reference's g20 fixtures (tools/make_goldens_cl.py) and the
float64 oracle.  Bars: the ones tests/test_gpu_dynamics.py applies to the same quantities at cl = 32 (set for exact-f32 arithmetic,
which these kernels keep).  Regimes 'analytic' and 'init'; 'stress' is out of scope here (its bars depend on the equal-codes
machinery of the cl = 32 tests)."""
import ctypes

import numpy as np
import pytest
import torch

import stove_oracle as O
import json
import math
import os

from gpu_helpers import check, check_grad, err, fill_analytic, regime_bar
from helpers import load_golden, oracle_setup, t_
from test_gpu_dynamics import _golden_noise, make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = (16, 64)
DYN_VARIANTS = {
    'plain3': dict(num_obj=3), 'plain6': dict(num_obj=6),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
}
STOVE_CASES = {
    'n3': dict(num_obj=3),
    'n6': dict(num_obj=6, debug_match_objects='greedy', overlap_beta=100.0, max_obj_scale=0.22),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
}


_GAPS = None


def gap(case, *path):
    """What the REFERENCE's own float32 run differs from its float64 run by on a g20 case (tests/golden/g20_reference_fp32_gap.json,
    written by tools/make_goldens_cl.py gap).  A bar below is the cl = 32 bar or, where the case itself amplifies float32 rounding
    beyond it, 6 x this gap (gpu_helpers.regime_bar).  A missing record is an error, never a silent zero."""
    global _GAPS
    if _GAPS is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g20_reference_fp32_gap.json')) as f:
            _GAPS = json.load(f)['gaps']
    v = _GAPS[case]
    for k in path:
        v = v[k]
    return float(v)


def logit_spacing(gold_rewards):
    """One float32 spacing of the largest reward logit, ulp(|q|) = 2^(floor(log2 |q|) - 23), q from the FIXTURE.  A predicted reward
    is sigmoid(q); relative to the reward an error dq of the logit shows as (1 - reward) dq, so no float32 implementation can promise
    the reward closer than half a spacing, and one that rounds a single time the other way than the reference's float32 run did is a
    whole spacing off.  It matters for one model only: the 'analytic' cl = 16 action-conditioned one predicts rewards of 1e-25
    (q = -57, spacing 3.8e-6), where the reference's float32 run happens to land 2.6e-7 from its float64 one, so that 6 x its gap
    (1.6e-6) lies BELOW half a spacing (1.9e-6).  Everywhere else the logits are O(1), the spacing is ~1e-8 and the bar is
    regime_bar(1e-6, gap) alone."""
    r = np.clip(np.asarray(gold_rewards, dtype=np.float64), 1e-300, 1 - 1e-16)
    q = float(np.abs(np.log(r) - np.log1p(-r)).max())
    return 2.0 ** (math.floor(math.log2(max(q, 1e-30))) - 23)


def width_cfg(cl):
    return dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


def gname(stem, regime):
    return f'{stem}_f64' if regime == 'analytic' else f'{stem}_{regime}_f64'


@pytest.mark.parametrize('name', list(DYN_VARIANTS))
@pytest.mark.parametrize('regime,arena', [('analytic', False), ('analytic', True), ('init', True), ('init', False)])
@pytest.mark.parametrize('cl', WIDTHS)
def test_dynamics_step(cl, regime, arena, name):
    """Step forward / backward against the reference's fixture.  Bars: step outputs and gradients 2.5e-5 / 2e-5 / 1e-3 (max / l2 /
    small), or 6 x the reference's own float32 gap on the same case where that is larger -- the 'analytic' action-conditioned case at
    cl = 16 is one (its loss runs through a reward of 1e-25; the reference's float32 gradients are 2.4e-5 off its float64 ones in
    the l2 norm).  Achieved there: 2.6e-5."""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.dynamics import Dynamics
    gold = load_golden(gname(f'g20_dynamics_cl{cl}_{name}', regime))
    case = f'g20_dynamics_cl{cl}_{name}_{regime}'
    dyn = fill_analytic(Dynamics(make_cfg(**DYN_VARIANTS[name], **width_cfg(cl))), 'dyn.', regime).to(DEV)
    if arena:
        assert ParamArena(dyn).has_gnn
    s = t_(gold['s']).float().to(DEV).requires_grad_()
    act = t_(gold['actions']).float().to(DEV) if 'actions' in gold else None
    app = t_(gold['app']).float().to(DEV).requires_grad_() if 'app' in gold else None
    res, rew = dyn(s, 0, act, app, lim_enc=int(gold['lim_enc']))
    assert res.shape[-1] == cl
    key = f'cl{cl}.dyn_step'
    check(key + '.result', err(res, gold['result']), regime_bar(2.5e-5, gap(case, 'result')))
    loss = (res * t_(gold['w']).float().to(DEV)).sum()
    if act is not None:
        check(key + '.reward', err(rew, gold['reward']), regime_bar(1e-6, gap(case, 'reward')))
        loss = loss + (rew * torch.linspace(1, 2, s.shape[0], device=DEV).view(-1, 1)).sum()
    loss.backward()
    check(key + '.grad_s', err(s.grad, gold['gs']), regime_bar(2.5e-5, gap(case, 'gs')))
    if app is not None:
        check(key + '.grad_app', err(app.grad, gold['gapp']), regime_bar(2.5e-5, gap(case, 'gapp')))
    params = dict(dyn.named_parameters())
    n = 0
    gp = lambda m: gap(case, 'grad_param', m)          # noqa: E731
    for k, v in gold.items():
        if k.startswith('g_'):
            assert params[k[2:]].grad is not None, k
            check_grad(key + '.grad_param', params[k[2:]].grad, v, regime_bar(2.5e-5, gp('max')), regime_bar(2e-5, gp('l2')),
                       regime_bar(1e-3, gp('small')))
            n += 1
    assert n >= 26


@pytest.mark.parametrize('n_obj', [3, 6])
@pytest.mark.parametrize('cl', WIDTHS)
def test_dynamics_step_ragged_batches_and_reproducible(cl, n_obj):
    """Batch sizes that do not fill the last workgroup, against the oracle; two runs must agree bitwise.
    The inputs are drawn here; tools/make_goldens_cl.py replays the same draws through the reference in float32 and float64, and a
    bar is 6 x that gap where it exceeds the step bar (cl = 64, six objects, B = 5: the reference's own float32 gradients are 1.9e-5
    off; achieved 3.3e-5)."""
    from stove_amd.video_prediction.dynamics import Dynamics
    c, structs, params = oracle_setup(torch.float64, num_obj=n_obj, **width_cfg(cl))
    dyn = fill_analytic(Dynamics(make_cfg(num_obj=n_obj, **width_cfg(cl))), 'dyn.').to(DEV)
    named = dict(dyn.named_parameters())
    g = torch.Generator().manual_seed(3)
    for B in (1, 5, 64, 257):
        s64 = torch.rand(B, n_obj, cl // 2, generator=g, dtype=torch.float64) * 1.6 - 0.8
        w64 = torch.rand(B, n_obj, cl, generator=g, dtype=torch.float64)
        so = s64.clone().requires_grad_()
        ro, _ = O.dynamics_forward(c, params, so)
        for p in params.values():
            p.grad = None
        (ro * w64).sum().backward()
        outs = []
        for _ in range(2):
            dyn.zero_grad()
            sd = s64.float().to(DEV).requires_grad_()
            rd, _ = dyn(sd, 0)
            (rd * w64.float().to(DEV)).sum().backward()
            outs.append((rd.detach().clone(), sd.grad.clone()) + tuple(named[k].grad.clone() for k in sorted(named) if named[k].grad is not None))
        key = f'cl{cl}.dyn_ragged.B{B}'
        case = f'ragged_cl{cl}_n{n_obj}_B{B}'
        check(key + '.result', err(outs[0][0], ro), regime_bar(2.5e-5, gap(case, 'result')))
        check(key + '.grad_s', err(outs[0][1], so.grad), regime_bar(2.5e-5, gap(case, 'gs')))
        for k in ('out.0.0.weight', 'rel_cores.0.0.weight', 'att_net.0.2.bias', 'state_enc.weight', 'rel_cores.0.0.bias'):
            check_grad(key + '.grad_param', named[k].grad, params['dyn.' + k].grad, regime_bar(2.5e-5, gap(case, 'grad_param', 'max')),
                       regime_bar(2e-5, gap(case, 'grad_param', 'l2')), regime_bar(1e-3, gap(case, 'grad_param', 'small')))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


@pytest.mark.parametrize('name', list(STOVE_CASES))
@pytest.mark.parametrize('cl', WIDTHS)
def test_recursion_matches_step_kernels(cl, name):
    """The one-launch recursion (forward and backward) equals the host time loop over the step kernel + PyTorch full_state."""
    from stove_amd.video_prediction.stove import Stove
    gold = load_golden(f'g20_stove_cl{cl}_{name}_f64')
    cfg = dict(STOVE_CASES[name], **width_cfg(cl))
    out = []
    for fused in (True, False):
        st = fill_analytic(Stove(make_cfg(fused_dynamics=fused, **cfg)), '').to(DEV)
        st.noise_fn = _golden_noise(gold)
        x = t_(gold['x']).float().to(DEV)
        actions = t_(gold['actions']).float().to(DEV) if 'actions' in gold else None
        elbo, prop, rewards = st(x, 0, actions)
        (-elbo).backward()
        out.append((elbo.detach(), {k: prop[k].clone() for k in ('z', 'z_dyn', 'z_std')},
                    {k: p.grad.clone() for k, p in st.named_parameters() if k.startswith('dyn.') and p.grad is not None}))
    key = f'cl{cl}.loop_vs_steps'
    check(key + '.elbo', abs(float(out[0][0]) - float(out[1][0])) / abs(float(out[1][0])), 1.5e-6)
    for k in out[0][1]:
        check(key + '.' + k, err(out[0][1][k], out[1][1][k]), 3e-6)
    assert len(out[0][2]) >= 26 and set(out[0][2]) == set(out[1][2])
    for k in out[0][2]:
        check_grad(key + '.grad', out[0][2][k], out[1][2][k], 3e-4, 3.5e-4, 4e-3)


@pytest.mark.parametrize('name', list(STOVE_CASES))
@pytest.mark.parametrize('regime,fused,arena', [('analytic', True, False), ('analytic', True, True), ('analytic', False, False),
                                                ('analytic', False, True), ('init', True, True), ('init', False, False)])
@pytest.mark.parametrize('cl', WIDTHS)
def test_stove_forward_elbo_and_grads(cl, regime, fused, arena, name):
    """Stove.forward + backward + an 8-step rollout against the reference at cl = 16 / 64, fused and op-by-op, arena on / off: the
    checks of test_gpu_dynamics.full_model_against_golden with the float32-gap records of the g20 cases.  Bars: ELBO 1.5e-6 relative;
    p_* 3e-6 (8e-6 z_sup); gradient norms 1.5e-4; gradient tensors 3e-4 / 3.5e-4 / 4e-3; rollouts 3e-6 -- each or 6 x the reference's own
    float32 gap on the same case, whichever is larger; rewards 1e-6 likewise, and never below one float32 spacing of their logit
    (logit_spacing: one case)."""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    gold = load_golden(gname(f'g20_stove_cl{cl}_{name}', regime))
    case, key = f'g20_stove_cl{cl}_{name}_{regime}', f'cl{cl}.stove'
    cfg = dict(STOVE_CASES[name], **width_cfg(cl))
    st = fill_analytic(Stove(make_cfg(fused_dynamics=fused, fused_state=fused, fused_elbo=fused, **cfg)), '', regime).to(DEV)
    if arena:
        ar = ParamArena(st)
        assert ar.has_spn and ar.has_gnn
    st.noise_fn = _golden_noise(gold)
    x = t_(gold['x']).float().to(DEV)
    actions = t_(gold['actions']).float().to(DEV) if 'actions' in gold else None
    elbo, prop, rewards = st(x, 0, actions)
    rel = abs(float(elbo) - float(gold['elbo'])) / abs(float(gold['elbo']))
    check(key + '.elbo_rel', rel, 1.5e-6)
    for k in ('z', 'z_dyn', 'z_sup', 'z_std', 'z_sup_std', 'log_q', 'translik', 'bg', 'patch', 'overlap'):
        check(key + '.prop_' + k, err(prop[k], gold['p_' + k]), regime_bar(8e-6 if k == 'z_sup' else 3e-6, gap(case, 'prop', k)))
    check(key + '.prop_z_dyn_std', err(prop['z_dyn_std'][2:], gold['p_z_dyn_std'][2:]), 1e-6)
    loss = -elbo
    if actions is not None:
        check(key + '.rewards', err(rewards, gold['rewards']), max(regime_bar(1e-6, gap(case, 'rewards')), logit_spacing(gold['rewards'])))
        loss = loss + 3.0 * (rewards ** 2).sum()
    loss.backward()
    params = dict(st.named_parameters())
    n = 0
    gt = lambda m: gap(case, 'grad_tensor', m)          # noqa: E731
    for k, v in gold.items():
        if k.startswith('gn_'):
            p = params[k[3:]]
            assert p.grad is not None, k
            check(key + '.grad_norm', abs(float(p.grad.norm()) - float(v)) / (float(v) + 1e-9), regime_bar(1.5e-4, gap(case, 'grad_norm_rel_max')))
            n += 1
        elif k.startswith('g_'):
            check_grad(key + '.grad_tensor', params[k[2:]].grad, v, regime_bar(3e-4, gt('max')), regime_bar(3.5e-4, gt('l2')),
                       regime_bar(4e-3, gt('small')))
    assert n > 50
    if arena:                                                  # cores 1-2 are never used: their gradients stay zero
        assert float(params['dyn.self_cores.1.0.weight'].grad.abs().max()) == 0.0
        ar.check()
    with torch.no_grad():
        z_last = prop['z'][:, -1]
        fut = actions[:, :5] if actions is not None else None
        app = prop['obj_appearances'][:, -1] if actions is not None else None
        zp, rp = st.rollout(z_last, num=gold['roll_z'].shape[1], actions=fut, appearance=app)
    assert zp.shape[-1] == cl // 2 + 2
    check(key + '.rollout_z', err(zp, gold['roll_z']), regime_bar(3e-6, gap(case, 'rollout_z')))
    if actions is not None:
        check(key + '.rollout_rewards', err(rp, gold['roll_rewards']), regime_bar(3e-6, gap(case, 'rollout_rewards')))


@pytest.mark.parametrize('name', ['n3', 'n6'])
@pytest.mark.parametrize('cl', WIDTHS)
def test_T100_against_the_oracle_on_the_box(cl, name):
    """B = 8, T = 100 on inputs no fixture holds (the shape of tests/test_gpu_full_length.py::test_T100_against_the_oracle_on_the_box):
    the float64 oracle on the host against the fused kernels and the op-by-op chain -- ELBO, z, EVERY parameter gradient (98 steps of
    carried gradient with the weight-gradient accumulators live across all of them) -- plus a 92-step rollout from the oracle's last
    state.  Bars as at cl = 32 (z 3e-6, gradients 3e-4 / 3.5e-4 / 4e-3, rollout 3e-6), or 6 x the reference's own float32 gap on these
    inputs where that is larger: six objects at cl = 16, where the reference's float32 z is 4.7e-6 off after 98 steps (kernels 3.3e-6)."""
    from stove_amd.arena import ParamArena
    from stove_amd.envs import envs
    from stove_amd.video_prediction.stove import Stove
    cfg = dict(STOVE_CASES[name], **width_cfg(cl))
    B, T, N = 8, 100, cfg['num_obj']
    x = torch.from_numpy(envs.synth_sequences('billiards' if N == 3 else 'multibilliards', B, T, seed0=900)['X']).float()
    g = torch.Generator().manual_seed(77 + cl)
    c, structs, params = oracle_setup(torch.float64, **cfg)
    lat = torch.randn(B, N, cl // 2 - 4, 1, generator=g, dtype=torch.float64)
    sd = torch.randn(B, N, cl // 2 - 4, 1, generator=g, dtype=torch.float64)
    steps = [torch.randn(B, N, cl // 2 + 2, generator=g, dtype=torch.float64) for _ in range(c.skip, T)]
    eps = {'latent': lat, 'std': sd, 'steps': steps}
    elbo_o, _, info = O.stove_forward(c, params, structs, x.double(), eps, None, detail=True)
    (-elbo_o).backward()
    with torch.no_grad():
        z_last = info['z'][:, -1].detach()
        roll_o, _ = O.rollout(c, params, z_last, 92, None, None)
    table = {'latent': lat[..., 0].float().to(DEV), 'std': sd[..., 0].float().to(DEV), 'steps': torch.stack(steps, 1).float().to(DEV)}
    for fused in (True, False):
        st = fill_analytic(Stove(make_cfg(fused_dynamics=fused, fused_state=fused, fused_elbo=fused, **cfg))).to(DEV)
        if fused:
            ParamArena(st)
        st.noise_fn = lambda kind, shape: table[kind].reshape(shape)
        elbo, prop, _ = st(x.to(DEV), 0, None)
        (-elbo).backward()
        tag = f'cl{cl}.stoveT100.oracle.' + ('fused' if fused else 'chain')
        case = f'T100_cl{cl}_{name}'      # the same inputs through the reference in float32 and float64 (tools/make_goldens_cl.py gap)
        check(tag + '.elbo_rel', abs(float(elbo) - float(elbo_o)) / abs(float(elbo_o)), 1.5e-6)
        for k in ('z', 'z_dyn', 'z_sup'):
            check(tag + '.' + k, err(prop[k], info[k].detach()), regime_bar(8e-6 if k == 'z_sup' else 3e-6, gap(case, 'prop', k)))
        n = 0
        gt = lambda m: gap(case, 'grad_tensor', m)          # noqa: E731
        for k, p in st.named_parameters():
            ref = params[k].grad
            if ref is None:
                continue
            check_grad(tag + '.grad', p.grad, ref, regime_bar(3e-4, gt('max')), regime_bar(3.5e-4, gt('l2')), regime_bar(4e-3, gt('small')))
            n += 1
        assert n > 100
        with torch.no_grad():
            zp, _ = st.rollout(z_last.float().to(DEV), num=92)
        check(tag + '.rollout92', err(zp, roll_o), regime_bar(3e-6, gap(case, 'rollout_z')))


def _train_three_steps(graphed):
    """three optimiser steps of the flat-parameter trainer at cl = 16 on three different batches (the runner of tests/test_gpu_replay.py)"""
    from stove_amd.arena import ParamArena
    from stove_amd.envs import envs
    from stove_amd.graphed import GraphedTrainStep
    from stove_amd.optim import FlatAdam
    from stove_amd.video_prediction.stove import Stove
    cfg = make_cfg(num_obj=3, **width_cfg(16))
    cfg.debug, cfg.print_every, cfg.plot_every = False, 10 ** 9, 1e19
    torch.manual_seed(0)
    model = Stove(cfg).to(DEV)
    table = {}

    def noise(kind, shape):
        key = (kind, tuple(shape))
        if key not in table:
            table[key] = torch.randn(shape, generator=torch.Generator().manual_seed(len(table) + 5)).to(DEV)
        return table[key]
    model.noise_fn = noise
    arena = ParamArena(model, 1)
    assert arena.has_gnn
    opt = FlatAdam(arena, lr=cfg.learning_rate, amsgrad=True)
    step = GraphedTrainStep(model, arena, opt, clip=1.0, reward_loss=None)
    d = envs.synth_sequences('billiards', 12, 9 + 3, seed0=5)
    out = []
    for s in range(3):
        rows = slice((s % 2) * 6, (s % 2) * 6 + 6)
        x = torch.from_numpy(d['X'][rows, s:s + 9]).to(DEV).contiguous()
        e = step(x, None, None, reward_weight=0.0) if graphed else step.eager(x, None, None, reward_weight=0.0)
        torch.cuda.synchronize()
        out.append((e.clone(), arena.grad.clone(), arena.data.clone()))
    if graphed:
        assert step.graphs is not None
    return out


def test_three_trainer_steps_graph_on_and_off():
    """Three Trainer steps at cl = 16 with the step captured and replayed, and eagerly: finite loss, parameters bit-equal between the
    two -- the arena's gather / scatter tables of the cl = 16 image and the capturability of the width-generic ops (no host
    synchronisation; zall and the ELBO as PyTorch chains inside the captured step)."""
    ref = _train_three_steps(False)
    got = _train_three_steps(True)
    for i, ((e0, g0, p0), (e1, g1, p1)) in enumerate(zip(ref, got)):
        assert torch.isfinite(e0) and torch.isfinite(e1) and float(g0.abs().max()) > 0
        assert torch.equal(e0, e1), ('elbo', i, float(e0), float(e1))
        assert torch.equal(g0, g1), ('gradient arena', i, float((g0 - g1).abs().max()))
        assert torch.equal(p0, p1), ('parameters', i, float((p0 - p1).abs().max()))
    assert not torch.equal(ref[0][2], ref[-1][2])         # it trained


@pytest.mark.parametrize('ac', [False, True])
def test_recursion_and_rollout_with_several_sequences_per_workgroup(ac):
    """cl = 16, B = 300 > 256: workgroups of the time-loop kernels own two sequences each.  The same batch in chunks of at most 256
    runs one sequence per workgroup (the layout every fixture test above goes through); per sequence the arithmetic is the same, so
    states and input gradients must be bit-equal and the weight gradients (another summation order) equal to float32 rounding."""
    from stove_amd import ops
    from stove_amd.video_prediction.dynamics import Dynamics
    cl, N, B, Ts, E = 16, 3, 300, 5, 7
    kw = dict(action_conditioned=True, action_space=9, debug_core_appearance=True) if ac else {}
    dyn = fill_analytic(Dynamics(make_cfg(num_obj=N, **kw, **width_cfg(cl))), 'dyn.').to(DEV)
    g = torch.Generator().manual_seed(11)
    D = cl // 2
    z1 = (torch.rand(B, N, D + 2, generator=g) - 0.5).to(DEV)
    zsup = (torch.rand(B, Ts, N, 6, generator=g) - 0.5).to(DEV)
    zsstd = (torch.rand(B, Ts, N, 6, generator=g) * 0.1 + 0.05).to(DEV)
    eps = torch.randn(B, Ts, N, D + 2, generator=g).to(DEV)
    extra = (torch.rand(B, Ts, N, E, generator=g) - 0.5).to(DEV) if ac else None
    wz = torch.rand(B, Ts, N, D + 2, generator=g).to(DEV)
    wp = torch.rand(B, Ts, N, cl, generator=g).to(DEV)

    def run(rows):
        dyn.zero_grad()
        a = z1[rows].clone().requires_grad_()
        ex = extra[rows].clone().requires_grad_() if ac else None
        z, zdyn, zdstd, mean, std, pred = ops.dyn_loop(a, zsup[rows], zsstd[rows], eps[rows], ex, dyn.param_image(0), 2, dyn.use_elu,
                                                        dyn.loop_consts(), want_pred=ac)
        loss = (z * wz[rows]).sum() + (zdyn * wz[rows][..., 2:]).sum() + (mean * std).sum()
        if ac:
            loss = loss + (pred * wp[rows]).sum()
        loss.backward()
        with torch.no_grad():
            zr, zs, pr = ops.rollout(z1[rows], extra[rows][:, :3].contiguous() if ac else None, dyn.param_image(0), 6, 2, dyn.use_elu,
                                     dyn.loop_consts(), want_std=True, want_pred=ac)
        grads = torch.cat([p.grad.reshape(-1) for k, p in sorted(dyn.named_parameters()) if p.grad is not None])
        outs = [z.detach(), zdyn.detach(), zdstd.detach(), mean.detach(), std.detach(), a.grad, zr, zs]
        if ac:
            outs += [pred.detach(), ex.grad, pr]
        return outs, grads
    whole, gw = run(slice(0, B))
    parts = [run(slice(0, 200)), run(slice(200, B))]
    for i, t in enumerate(whole):
        assert torch.equal(t, torch.cat([parts[0][0][i], parts[1][0][i]], 0)), i
    check_grad('cl16.loop_groups.grad', gw, parts[0][1] + parts[1][1], 2.5e-5, 2e-5, 1e-3)


def test_abi_rejects_unsupported_widths_and_null_tables():
    from stove_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1 << 16, device=DEV)
    p = ctypes.c_void_p(x.data_ptr())
    st = _lib.stream()
    bad = 1                                         # hipErrorInvalidValue
    assert lib.stove_gnn_fwd_cl(p, p, p, p, 24, 2, 3, 12, 2, 0, st) == bad              # cl
    assert lib.stove_gnn_fwd_cl(p, p, p, p, 32, 2, 3, 16, 2, 0, st) == bad              # cl = 32 has its own entry points
    assert lib.stove_gnn_fwd_cl(p, p, p, p, 16, 2, 3, 17, 2, 0, st) == bad              # sin_dim > cl
    assert lib.stove_gnn_fwd_cl(p, p, p, p, 16, 2, 3, 7, 2, 0, st) == bad               # sin_dim < cl / 2
    assert lib.stove_gnn_fwd_cl(p, p, p, p, 16, 2, 7, 8, 2, 0, st) == bad               # N
    assert lib.stove_gnn_fwd_cl(p, None, p, p, 16, 2, 3, 8, 2, 0, st) == bad            # NULL parameter image
    assert lib.stove_gnn_bwd_cl(p, p, p, None, p, None, p, 16, 2, 3, 8, 2, 0, st) == bad   # NULL gradient image
    assert lib.stove_gnn_bwd_cl(p, p, p, None, p, p, None, 64, 2, 3, 32, 2, 0, st) == bad  # NULL workspace
    assert lib.stove_rollout_fwd_cl(p, None, p, p, None, None, 16, 2, 4, 1, 3, 12, 2, 0, 0.3, 0.04, 0.1, st) == bad   # extra dims without `extra`
    assert lib.stove_dynloop_fwd_cl(*([p] * 4 + [None] + [p] * 6 + [None]), 24, 2, 4, 3, 12, 2, 0, 0.3, 0.04, 0.1, st) == bad
    assert lib.stove_dynloop_bwd_cl(*([p] * 4 + [None] + [p] * 2 + [None] * 5 + [p] * 3 + [None, None, p]), 16, 2, 4, 3, 8, 2, 0, 0.3, 0.04, 0.1, st) == bad
    assert lib.stove_gnn_param_floats_cl(24) == 0 and lib.stove_gnn_bwd_ws_bytes_cl(24, 2, 3) == 0
    torch.cuda.synchronize()
