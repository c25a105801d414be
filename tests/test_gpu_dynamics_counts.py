"""The dynamics kernels (csrc/gnn.hip, gnn_small.hip, gnn_small_bwd.hip, gnn_cl.hip) against the float64 oracle at EVERY object count
their entry points accept -- 1 .. 8 at cl = 32, 1 .. 6 at cl = 16 / 64 -- where the reference-generated fixtures only hold three and six:
one step forward and backward (Dynamics.forward), the one-launch inference recursion forward and backward (ops.dyn_loop against
O.recursion) and the mean rollout (ops.rollout against O.rollout), each with the three input widths the kernels are instantiated for
(plain cl/2, actions cl/2 + 4, actions + appearance cl/2 + 7), both nonlinearities and the 'analytic' and 'init' weights.

Inputs: helpers.dyn_* -- float64 draws of a seeded CPU generator, rounded to float32 so that the oracle and the device see the same
numbers, nothing symmetric between the objects.  Bars: what the same quantity holds at three and six objects (named at each check), or
6 x the oracle's own float32-vs-float64 gap on the same inputs where that is larger (gpu_helpers.regime_bar; the gap is measured here on
the CPU and printed next to what the kernel achieves -- the rule of tests/test_gpu_rollout_sample.py).  Achieved errors:
profiles/dyn_counts_parity.json."""
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, err_l2, err_small, fill_analytic, regime_bar
from helpers import DYN_VARIANTS, dyn_actions, dyn_appearance, dyn_oracle, dyn_recursion_inputs, dyn_state, embed_actions
from test_gpu_cl import logit_spacing
from test_gpu_dynamics import make_cfg
from test_gpu_rollout_sample import width_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (cl, N): the counts no fixture holds; three and six objects at cl = 32 are the anchors that tie the bars to shapes with fixtures
NEW_COUNTS = [(32, n) for n in (1, 2, 4, 5, 7, 8)] + [(cl, n) for cl in (16, 64) for n in (1, 2, 4, 5)]
NL = ('relu', 'leaky_relu')                  # = leaky-relu and elu in the kernels (the reference's inverted selection, dynamics.py:109)
REGIMES = ('analytic', 'init')


def _cases(a, b):
    """(cl, N, variant, nonlinear, regime, x): three cases per (cl, N) -- every variant, both nonlinearities, both regimes, and both
    values (a, b) of the case's own size parameter x (batch size / Ts / num) -- plus one anchor each at three and six objects"""
    out = []
    for i, (cl, n) in enumerate(NEW_COUNTS):
        out.append((cl, n, 'plain', 'relu', 'analytic', (a, b)[i % 2]))
        out.append((cl, n, 'act', 'leaky_relu', 'init', (b, a)[i % 2]))
        out.append((cl, n, 'actapp', NL[i % 2], REGIMES[(i + 1) % 2], a))
    out.append((32, 3, 'actapp', 'relu', 'analytic', a))
    out.append((32, 6, 'plain', 'leaky_relu', 'init', a))
    return out


def _id(case):
    return 'cl%d-n%d-%s-%s-%s-%s' % case


def _dynamics(cl, n_obj, variant, nonlinear, regime):
    from stove_amd.video_prediction.dynamics import Dynamics
    cfg = make_cfg(num_obj=n_obj, debug_nonlinear=nonlinear, **DYN_VARIANTS[variant], **width_cfg(cl))
    return fill_analytic(Dynamics(cfg), 'dyn.', regime).to(DEV)


def _f32(t):
    """a float64 draw rounded to float32 and kept in float64: what the device is handed, to the bit"""
    return None if t is None else t.float().double()


def _dev(t, grad=False):
    return None if t is None else t.float().to(DEV).requires_grad_(grad)


def _to(t, dtype):
    return None if t is None else t.to(dtype)


def _leaf(t, dtype):
    """a copy of `t` in `dtype` that a gradient is asked for"""
    return None if t is None else t.detach().to(dtype).clone().requires_grad_()


def _clear(params):
    for p in params.values():
        p.grad = None


def _grads(params):
    return {k: p.grad.clone() for k, p in params.items() if p.grad is not None}


def _held(key, got, want, low, bar):
    """check(got against the float64 oracle's `want`) at regime_bar(bar, gap), gap = what the oracle's float32 run `low` differs
    from `want` by; the achieved error is printed next to the gap"""
    e, gap = err(got, want), err(low, want)
    print(f'{key}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {regime_bar(bar, gap):.3g})')
    check(key, e, regime_bar(bar, gap))


def _held_grads(key, got, want, low, bars):
    """{name: gradient} against the oracle's on the three scales of check_grad; the float32 gap of each scale is the largest over
    the tensors.  The device must hold a gradient for exactly the tensors the oracle differentiates."""
    assert set(got) == set(want) == set(low), sorted(set(got) ^ set(want))
    gaps = [max(f(low[k], want[k]) for k in want) for f in (err, err_l2, err_small)]
    worst = [max(f(got[k], want[k]) for k in want) for f in (err, err_l2, err_small)]
    print(f'{key}: max {worst[0]:.3g} ({gaps[0]:.3g})  l2 {worst[1]:.3g} ({gaps[1]:.3g})  small {worst[2]:.3g} ({gaps[2]:.3g})  [achieved (oracle f32 gap)]')
    for k in want:
        check_grad(key, got[k], want[k], *[regime_bar(b, g) for b, g in zip(bars, gaps)])
    return len(want)


# ------------------------------------------------------------------------------------------------ a. one step, forward and backward
def _step_oracle(cl, n_obj, variant, nonlinear, regime, dtype, s, actions, app, lim_enc, w):
    c, params = dyn_oracle(cl, n_obj, variant, regime, dtype, nonlinear)
    _clear(params)
    so, ao = _leaf(s, dtype), _leaf(app, dtype)
    res, rew, pred = O.dynamics_forward(c, params, so, _to(actions, dtype), ao, lim_enc=lim_enc, with_pred=True)
    loss = (res * w.to(dtype)).sum()
    if actions is not None:
        loss = loss + (rew * torch.linspace(1, 2, s.shape[0], dtype=dtype).view(-1, 1)).sum()
    loss.backward()
    out = {'result': res.detach(), 'pred': pred.detach(), 'reward': rew.detach() if actions is not None else None, 'gs': so.grad,
           'gapp': ao.grad if ao is not None else None, 'grads': _grads(params)}
    _clear(params)
    return out


def _step_device(dyn, monkeypatch, s, actions, app, lim_enc, w):
    from stove_amd import ops
    dyn.zero_grad(set_to_none=True)
    sd, ad = _dev(s, True), _dev(app, True)
    seen, gnn_step = [], ops.gnn_step
    monkeypatch.setattr(ops, 'gnn_step', lambda *a, **kw: seen.append(gnn_step(*a, **kw)) or seen[-1])
    res, rew = dyn(sd, 0, _dev(actions), ad, lim_enc)
    monkeypatch.undo()
    (_, pred), = seen                                           # the kernel's second output: dynamic_pred, what the reward head reads
    loss = (res * _dev(w)).sum()
    if actions is not None:
        loss = loss + (rew * torch.linspace(1, 2, s.shape[0], device=DEV).view(-1, 1)).sum()
    loss.backward()
    return {'result': res.detach(), 'pred': pred.detach(), 'reward': rew.detach() if actions is not None else None, 'gs': sd.grad,
            'gapp': ad.grad if ad is not None else None,
            'grads': {'dyn.' + k: p.grad.clone() for k, p in dyn.named_parameters() if p.grad is not None}}


@pytest.mark.parametrize('case', _cases(11, 1), ids=_id)
def test_step_against_the_oracle(case, monkeypatch):
    """Dynamics.forward + backward against O.dynamics_forward.  B = 11 (fills no workgroup at any N) and B = 1; lim_enc = 4 on the
    'act' case of every count, 2 elsewhere.  Loss: every element of `result` under a random weight, with actions plus the
    reward under linspace(1, 2, B) (tests/test_gpu_dynamics.py::test_dynamics_step).  Bars, those of that test at three and six
    objects: result (and dynamic_pred, the kernel's other output) 2e-6, reward 1e-6, d s 5e-6, d app 1e-5, parameter gradients
    2.5e-5 / 2e-5 / 1e-3 (max / l2 / entry-wise) -- all 28 of them (state encoder and the five MLPs of core 0), 40 with actions
    (embedding and reward head); cores 1 and 2 get none on either side.  At N = 1 the oracle's relation and attention gradients are
    exact zeros (no edges), so the kernels' must be, too.  Two runs must agree bit for bit."""
    cl, n_obj, variant, nonlinear, regime, B = case
    lim_enc = 4 if variant == 'act' else 2
    g = torch.Generator().manual_seed(10000 + 100 * cl + 10 * n_obj + list(DYN_VARIANTS).index(variant))
    s, actions, app = _f32(dyn_state(g, B, n_obj, cl)), dyn_actions(g, variant, B), _f32(dyn_appearance(g, variant, B, n_obj))
    w = _f32(torch.rand(B, n_obj, cl, generator=g, dtype=torch.float64))
    want = _step_oracle(cl, n_obj, variant, nonlinear, regime, torch.float64, s, actions, app, lim_enc, w)
    low = _step_oracle(cl, n_obj, variant, nonlinear, regime, torch.float32, s, actions, app, lim_enc, w)
    dyn = _dynamics(cl, n_obj, variant, nonlinear, regime)
    got = _step_device(dyn, monkeypatch, s, actions, app, lim_enc, w)
    again = _step_device(dyn, monkeypatch, s, actions, app, lim_enc, w)
    key = f'dyn_counts.step.cl{cl}.n{n_obj}'
    _held(key + '.result', got['result'], want['result'], low['result'], 2e-6)
    _held(key + '.pred', got['pred'], want['pred'], low['pred'], 2e-6)
    if actions is not None:
        # never below one float32 spacing of the reward's logit (test_gpu_cl.logit_spacing: a reward is sigmoid(q), and relative to it
        # an error dq of the logit shows as (1 - reward) dq -- models that predict rewards of 1e-25 sit at q = -57, spacing 3.8e-6)
        e, gap = err(got['reward'], want['reward']), err(low['reward'], want['reward'])
        bar = max(regime_bar(1e-6, gap), logit_spacing(want['reward'].numpy()))
        print(f'{key}.reward: {e:.3g} (oracle f32 gap {gap:.3g}, bar {bar:.3g})')
        check(key + '.reward', e, bar)
    _held(key + '.grad_s', got['gs'], want['gs'], low['gs'], 5e-6)
    if app is not None:
        _held(key + '.grad_app', got['gapp'], want['gapp'], low['gapp'], 1e-5)
    n = _held_grads(key + '.grad_param', got['grads'], want['grads'], low['grads'], (2.5e-5, 2e-5, 1e-3))
    assert n == (28 if variant == 'plain' else 40)
    for k in ('result', 'pred', 'reward', 'gs', 'gapp'):
        assert got[k] is None or torch.equal(got[k], again[k]), k
    for k, v in got['grads'].items():
        assert torch.equal(v, again['grads'][k]), k


# ------------------------------------------------------------------------------------------------ b. the recursion, forward and backward
LOOP_OUT = ('z', 'z_dyn', 'z_dyn_std', 'mean', 'std')          # ops.dyn_loop's outputs in order, under O.recursion's names


def _loop_extra(params64, n_obj, actions, app):
    """[embedded one-hot actions | appearance rows] (..., N, 4 or 7) in float64, or None: the kernels' `extra` input"""
    rows = ([embed_actions(params64, actions, n_obj).detach()] if actions is not None else []) + ([app] if app is not None else [])
    return torch.cat(rows, -1) if rows else None


def _loop_oracle(cl, n_obj, variant, nonlinear, regime, dtype, z1, zsup, zsstd, eps, extra, ws):
    c, params = dyn_oracle(cl, n_obj, variant, regime, dtype, nonlinear)
    _clear(params)
    ins = [_leaf(t, dtype) for t in (z1, zsup, zsstd, extra)]
    r = O.recursion(c, params, ins[0], ins[1], ins[2], eps.to(dtype).unbind(1), None, ins[3])
    # z_dyn_std carries no weight: ops.dyn_loop marks it non-differentiable (the model reads the dynamics' stds through `std` only)
    loss = sum((r[k] * ws[k].to(dtype)).sum() for k in ('z', 'z_dyn', 'mean', 'std'))
    if extra is not None:
        loss = loss + (r['dynamic_pred'] * ws['pred'].to(dtype)).sum()
    loss.backward()
    out = {k: r[k].detach() for k in LOOP_OUT}
    out['pred'] = r['dynamic_pred'].detach()
    out['gin'] = {k: t.grad for k, t in zip(('z1', 'zsup', 'zsstd', 'extra'), ins) if t is not None}
    out['grads'] = _grads(params)
    _clear(params)
    return out


@pytest.mark.parametrize('case', _cases(4, 1), ids=_id)
def test_recursion_against_the_oracle(case):
    """ops.dyn_loop, called directly on given states (no recognition network, no matcher: their float32 codes and tie-breaks stay out
    of the comparison), against O.recursion on the same arrays.  B = 5; Ts = 4 and Ts = 1 (no carried state).  With actions `extra`
    holds the embedded one-hot actions (and the appearance rows), `pred` is asked for and the loss weights it, too: the backward
    with a gradient for pred; the plain cases run the one without.  The loss weights every differentiable output with a random tensor
    of its own.  Bars, those of test_stove_forward_elbo_and_grads for p_z / p_z_dyn / p_z_std and g_*: outputs 3e-6, input and
    parameter gradients 3e-4 / 3.5e-4 / 4e-3.  The forward that saves nothing (torch.no_grad) returns bit for bit what the saving
    one returns -- at every count here, one and eight objects included."""
    from stove_amd import ops
    cl, n_obj, variant, nonlinear, regime, Ts = case
    B, D = 5, cl // 2
    g = torch.Generator().manual_seed(20000 + 100 * cl + 10 * n_obj + list(DYN_VARIANTS).index(variant))
    z1, zsup, zsstd, eps = [_f32(t) for t in dyn_recursion_inputs(g, B, Ts, n_obj, cl)]
    _, params64 = dyn_oracle(cl, n_obj, variant, regime, torch.float64, nonlinear)
    extra = _f32(_loop_extra(params64, n_obj, dyn_actions(g, variant, B, Ts), dyn_appearance(g, variant, B, Ts, n_obj)))
    assert (extra is None) == (variant == 'plain') and (extra is None or extra.shape[-1] == {'act': 4, 'actapp': 7}[variant])
    r = lambda *shape: _f32(torch.rand(*shape, generator=g, dtype=torch.float64))          # noqa: E731
    ws = {'z': r(B, Ts, n_obj, D + 2), 'z_dyn': r(B, Ts, n_obj, D), 'mean': r(B, Ts, n_obj, D + 2), 'std': r(B, Ts, n_obj, D + 2),
          'pred': r(B, Ts, n_obj, cl)}
    want = _loop_oracle(cl, n_obj, variant, nonlinear, regime, torch.float64, z1, zsup, zsstd, eps, extra, ws)
    low = _loop_oracle(cl, n_obj, variant, nonlinear, regime, torch.float32, z1, zsup, zsstd, eps, extra, ws)

    dyn = _dynamics(cl, n_obj, variant, nonlinear, regime)
    ins = [_dev(z1, True), _dev(zsup, True), _dev(zsstd, True), _dev(eps), _dev(extra, True)]
    image, sink = dyn.kernel_params(0)
    assert sink is None
    want_pred = extra is not None
    outs = ops.dyn_loop(*ins, image, 2, dyn.use_elu, dyn.loop_consts(), want_pred)
    with torch.no_grad():
        plain = ops.dyn_loop(*[t.detach() if t is not None else None for t in ins], image, 2, dyn.use_elu, dyn.loop_consts(), want_pred)
    assert outs[0].grad_fn is not None and plain[0].grad_fn is None
    for k, u, v in zip(LOOP_OUT + ('pred',), outs, plain):
        assert torch.equal(u, v), k
    got = dict(zip(LOOP_OUT + ('pred',), outs))
    loss = sum((got[k] * _dev(ws[k])).sum() for k in ('z', 'z_dyn', 'mean', 'std'))
    if want_pred:
        loss = loss + (got['pred'] * _dev(ws['pred'])).sum()
    loss.backward()

    key = f'dyn_counts.loop.cl{cl}.n{n_obj}'
    for k in LOOP_OUT + (('pred',) if want_pred else ()):
        assert got[k].shape == want[k].shape, k
        _held(f'{key}.{k}', got[k], want[k], low[k], 3e-6)
    gin = {k: t.grad for k, t in zip(('z1', 'zsup', 'zsstd', 'extra'), (ins[0], ins[1], ins[2], ins[4])) if t is not None}
    assert all(v is not None for v in gin.values())
    _held_grads(key + '.grad_in', gin, want['gin'], low['gin'], (3e-4, 3.5e-4, 4e-3))
    grads = {'dyn.' + k: p.grad for k, p in dyn.named_parameters() if p.grad is not None}
    n = _held_grads(key + '.grad_param', grads, want['grads'], low['grads'], (3e-4, 3.5e-4, 4e-3))
    assert n == 28                                   # core 0; the embedding and the reward head lie outside the recursion kernels


# ------------------------------------------------------------------------------------------------ c. the mean rollout
def _rollout_oracle(cl, n_obj, variant, nonlinear, regime, dtype, z_last, num, actions, app):
    """O.rollout -> z; the stds and dynamic_pred of every step from one more pass of the core over the states the rollout visited"""
    c, params = dyn_oracle(cl, n_obj, variant, regime, dtype, nonlinear)
    D = cl // 2
    with torch.no_grad():
        z0, act, ap = z_last.to(dtype), _to(actions, dtype), _to(app, dtype)
        z, _ = O.rollout(c, params, z0, num, act, ap)
        prev = torch.cat([z0[:, None], z[:, :-1]], 1)
        sds, preds = [], []
        for t in range(num):
            out, _, pred = O.dynamics_forward(c, params, prev[:, t, :, 2:], act[:, t % act.shape[1]] if act is not None else None, ap,
                                              with_pred=True)
            m, sd = O.constrain_z_dyn(c, out[..., :D], out[..., D:])
            assert err(torch.cat([prev[:, t, :, 2:4] + m[..., :2], m[..., 2:]], -1), z[:, t, :, 2:]) < 64 * torch.finfo(dtype).eps      # the same step again
            sds.append(sd)
            preds.append(pred)
    return {'z': z, 'zstd': torch.stack(sds, 1), 'pred': torch.stack(preds, 1)}


@pytest.mark.parametrize('case', _cases(7, 1), ids=_id)
def test_mean_rollout_against_the_oracle(case):
    """ops.rollout(want_std, want_pred) against O.rollout, B = 5, num = 7 and 1.  With actions: A = 4 action rows, so that seven steps
    go round the t % A cycle; the oracle embeds the one-hot actions itself, the kernel is handed the float64 embedding rounded to
    float32.  Bars: z and the stds 3e-6 (rollout_z at three and six objects), pred likewise; the scale columns are copies."""
    from stove_amd import ops
    cl, n_obj, variant, nonlinear, regime, num = case
    B, A = 5, 4
    g = torch.Generator().manual_seed(30000 + 100 * cl + 10 * n_obj + list(DYN_VARIANTS).index(variant))
    z_last = _f32(dyn_recursion_inputs(g, B, 1, n_obj, cl)[0])
    actions, app = dyn_actions(g, variant, B, A), _f32(dyn_appearance(g, variant, B, n_obj))
    want = _rollout_oracle(cl, n_obj, variant, nonlinear, regime, torch.float64, z_last, num, actions, app)
    low = _rollout_oracle(cl, n_obj, variant, nonlinear, regime, torch.float32, z_last, num, actions, app)
    _, params64 = dyn_oracle(cl, n_obj, variant, regime, torch.float64, nonlinear)
    extra = _loop_extra(params64, n_obj, actions, app[:, None].expand(-1, A, -1, -1) if app is not None else None)
    dyn = _dynamics(cl, n_obj, variant, nonlinear, regime)
    with torch.no_grad():
        image = dyn.kernel_params(0)[0]
        zd = _dev(z_last)
        z, zstd, pred = ops.rollout(zd, _dev(extra).contiguous() if extra is not None else None, image, num, 2, dyn.use_elu,
                                    dyn.loop_consts(), want_std=True, want_pred=True)
    D = cl // 2
    assert z.shape == (B, num, n_obj, D + 2) and zstd.shape == (B, num, n_obj, D) and pred.shape == (B, num, n_obj, cl)
    assert torch.equal(z[..., :2], zd[:, None, :, :2].expand(-1, num, -1, -1))            # scales: copied, exactly
    key = f'dyn_counts.rollout.cl{cl}.n{n_obj}'
    _held(key + '.z', z, want['z'], low['z'], 3e-6)
    _held(key + '.zstd', zstd, want['zstd'], low['zstd'], 3e-6)
    _held(key + '.pred', pred, want['pred'], low['pred'], 3e-6)
