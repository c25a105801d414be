"""GPU tests of the differentiable one-launch rollout (stove_rollout_bwd / _cl behind ops.rollout and Stove.rollout): gradients of both
branches against the float64 oracle's autograd at every kind of shape the kernels take, the t % A cycle of the extra rows, the fused
sampling rollout against the loop of single steps it may one day replace, the forward left bit for bit where it was, run-to-run
reproducibility, the arena path and the C ABI's argument checks.

Inputs: helpers.dyn_* -- float64 draws of a seeded CPU generator rounded to float32, so that oracle and device see the same numbers.
Gradient bars: the recursion's, 3e-4 / 3.5e-4 / 4e-3 on check_grad's three scales (largest entry, l2, entry-wise), each through
gpu_helpers.regime_bar with the oracle's own float32-vs-float64 gap on the same inputs, measured on the CPU inside the test and printed
next to the achieved error (the rule of tests/test_gpu_dynamics_counts.py).  A case whose gap would lift a bar beyond 10 x its base
value fails: such a seed is replaced (SEEDS), not excused.

Gaps of the cases in use, checked on the CPU before any GPU run (largest over the 54 cases of group 1 and the eight of group 2;
max / l2 / entry-wise): inputs 1.2e-5 / 4.3e-6 / 5.9e-4, parameters 3.9e-5 / 3.9e-5 / 1.4e-3.  Only the entry-wise scale is lifted
at all (to at most 8.5e-3 of the 4e-2 allowed); one seed was replaced for that (SEEDS) and two shapes rotated (ROTATION)."""
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, err_l2, err_small, fill_analytic, regime_bar
from helpers import DYN_VARIANTS, dyn_actions, dyn_appearance, dyn_oracle, dyn_recursion_inputs, dyn_state
from test_gpu_dynamics import make_cfg
from test_gpu_dynamics_counts import NL, REGIMES, _clear, _dev, _f32, _grads, _leaf, _to
from test_gpu_rollout_sample import width_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INVALID = 1          # hipErrorInvalidValue
BARS = (3e-4, 3.5e-4, 4e-3)

# (cl, N): one object (no edges), the small-graph forwards of cl = 32 (3, 6) under the block-wise backward, block-wise both ways (7);
# cl = 16 with one, three (N = 5) and two (N = 6) sequences per workgroup at B = 11; cl = 64 (one sequence per workgroup)
SHAPES = [(32, 1), (32, 3), (32, 6), (32, 7), (16, 1), (16, 5), (16, 6), (64, 2), (64, 6)]
ACTION_ROWS = 4      # A of group 1: seven steps go round the t % A cycle, one step leaves three rows unread
SEEDS = {(64, 6, 'plain'): 146460}          # (cl, N, variant) -> seed, where the default seed's rollout is too ill-conditioned for the bars
# cl = 16 under the 'analytic' weights: seven steps at N = 1 ('plain') and N = 5 ('actapp') are ill-conditioned at nearly EVERY seed
# (float32 gap of the oracle 1e-3 ... 1e-1 at 29 of 29 seeds tried, each), a property of that model, not of a draw.  The rotation gives
# these two shapes their seven steps under the 'init' weights and the 'analytic' ones where they are well-conditioned.
ROTATION = {(16, 1): [('plain', 'relu', 'init', 11, 7), ('act', 'leaky_relu', 'analytic', 11, 1), ('actapp', 'relu', 'init', 1, 7)],
            (16, 5): [('plain', 'relu', 'analytic', 11, 7), ('act', 'leaky_relu', 'init', 11, 1), ('actapp', 'leaky_relu', 'init', 1, 7)]}


def _cases():
    """(cl, N, variant, nonlinear, regime, B, num): three per shape -- every variant, both nonlinearities, both regimes; B = 11 with
    num = 7 always, B = 1 and num = 1 (no carry) once each"""
    out = []
    for i, (cl, n) in enumerate(SHAPES):
        if (cl, n) in ROTATION:
            out += [(cl, n) + rest for rest in ROTATION[(cl, n)]]
            continue
        out.append((cl, n, 'plain', 'relu', 'analytic', 11, 7))
        out.append((cl, n, 'act', 'leaky_relu', 'init', (1, 11)[i % 2], (7, 1)[i % 2]))
        out.append((cl, n, 'actapp', NL[i % 2], REGIMES[(i + 1) % 2], (11, 1)[i % 2], (1, 7)[i % 2]))
    return out


def _id(case):
    return 'cl%d-n%d-%s-%s-%s-B%d-num%d' % case


def _inputs(case):
    """z_last (B,N,D+2), one-hot actions (B,A,9) or None, appearance (B,N,3) or None, eps (B,num,N,D), and the loss weights"""
    cl, n_obj, variant, _, _, B, num = case
    D = cl // 2
    seed = SEEDS.get((cl, n_obj, variant), 40000 + 100 * cl + 10 * n_obj + list(DYN_VARIANTS).index(variant))
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: _f32(torch.rand(*shape, generator=g, dtype=torch.float64))          # noqa: E731
    z_last = _f32(torch.cat([dyn_recursion_inputs(g, B, 1, n_obj, cl)[0][..., :2], dyn_state(g, B, n_obj, cl)], -1))
    d = {'z_last': z_last, 'actions': dyn_actions(g, variant, B, ACTION_ROWS), 'app': _f32(dyn_appearance(g, variant, B, n_obj)),
         'eps': _f32(torch.randn(B, num, n_obj, D, generator=g, dtype=torch.float64)),
         'wz': r(B, num, n_obj, D + 2), 'wr': r(B, num, 1), 'wq': r(B, num, n_obj, D)}
    return d


def _loss(d, z, rewards, log_q, cast):
    loss = (z * cast(d['wz'])).sum()
    if d['actions'] is not None:
        loss = loss + (rewards * cast(d['wr'])).sum()
    if log_q is not None:
        loss = loss + (log_q * cast(d['wq'])).sum()
    return loss


def _oracle_case(case, sample, dtype, d):
    """O.rollout in `dtype` with requires_grad leaves -> outputs, input gradients, parameter gradients"""
    cl, n_obj, variant, nonlinear, regime, B, num = case
    c, params = dyn_oracle(cl, n_obj, variant, regime, dtype, nonlinear)
    _clear(params)
    z0, ap = _leaf(d['z_last'], dtype), _leaf(d['app'], dtype)
    out = O.rollout(c, params, z0, num, _to(d['actions'], dtype), ap, eps=[e.to(dtype) for e in d['eps'].unbind(1)] if sample else None)
    z, rewards, log_q = out[0], out[-1], (out[1] if sample else None)
    _loss(d, z, rewards, log_q, lambda t: t.to(dtype)).backward()
    res = {'z': z.detach(), 'gin': {'z_last': z0.grad}, 'grads': _grads(params)}
    if ap is not None:
        res['gin']['app'] = ap.grad
    _clear(params)
    return res


def _gaps(got, want):
    return [max(f(got[k], want[k]) for k in want) for f in (err, err_l2, err_small)]


def _held_grads(key, got, want, low):
    """{name: gradient} against the float64 oracle's at regime_bar(BARS, the float32 oracle's gap); exactly the oracle's tensors"""
    assert set(got) == set(want) == set(low), sorted(set(got) ^ set(want))
    gaps, worst = _gaps(low, want), _gaps(got, want)
    print(f'{key}: max {worst[0]:.3g} ({gaps[0]:.3g})  l2 {worst[1]:.3g} ({gaps[1]:.3g})  small {worst[2]:.3g} ({gaps[2]:.3g})  [achieved (oracle f32 gap)]')
    bars = [regime_bar(b, g) for b, g in zip(BARS, gaps)]
    assert all(bar <= 10 * b for bar, b in zip(bars, BARS)), (key, 'the oracle itself is ill-conditioned on this seed: replace it', gaps)
    for k in want:
        check_grad(key, got[k], want[k], *bars)
    return len(want)


def _stove(cl, n_obj, variant, nonlinear='relu', regime='analytic', **kw):
    from stove_amd.video_prediction.stove import Stove
    if n_obj != 3:
        kw.setdefault('debug_match_objects', 'greedy')
    cfg = make_cfg(num_obj=n_obj, debug_nonlinear=nonlinear, **kw, **DYN_VARIANTS[variant], **width_cfg(cl))
    return fill_analytic(Stove(cfg), '', regime).to(DEV)


def _feed(eps):
    it = iter(eps.unbind(1))
    return lambda kind, shape: next(it).reshape(shape)


def _device_case(st, sample, d, num, fused=True, arena=None):
    """Stove.rollout + backward on the device -> outputs, input gradients, the gradients of the dynamics' parameters"""
    if arena is not None:
        arena.zero_grad()          # (the parameters' .grad are views of the arena's flat gradient: zeroed, not dropped)
    else:
        st.zero_grad(set_to_none=True)
    z0, ap = _dev(d['z_last'], True), _dev(d['app'], True)
    st.noise_fn = _feed(_dev(d['eps'])) if sample else None
    out = st.rollout(z0, num=num, sample=sample, actions=_dev(d['actions']), appearance=ap, fused=fused if sample else None)
    st.noise_fn = None
    z, rewards, log_q = out[0], out[-1], (out[1] if sample else None)
    assert z.grad_fn is not None
    _loss(d, z, rewards, log_q, _dev).backward()
    res = {'z': z.detach(), 'log_q': log_q.detach() if sample else None, 'gin': {'z_last': z0.grad},
           'grads': {'dyn.' + k: p.grad.clone() for k, p in st.dyn.named_parameters() if p.grad is not None}}
    if ap is not None:
        res['gin']['app'] = ap.grad
    return res


# ------------------------------------------------------------------------------------------------ 1. against the float64 oracle
@pytest.mark.parametrize('sample', [False, True], ids=['mean', 'sample'])
@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_rollout_gradients_against_the_oracle(case, sample):
    """Stove.rollout (mean; sample=True, fused=True with eps through noise_fn) + backward against O.rollout's autograd in float64.
    Loss: every element of z_pred under a random weight, with actions the rewards, when sampling log q, each under weights of its
    own.  Checked: d z_last (scale columns included: the sum of their weights over the steps), d appearance, and every parameter
    gradient -- core 0, with actions the embedding (the d extra of the kernel, through its Linear) and the reward head (d pred);
    the device holds a gradient for exactly the tensors the oracle differentiates.  One object: no edges, so the relation and
    attention gradients are exact zeros on both sides."""
    cl, n_obj, variant, nonlinear, regime, B, num = case
    d = _inputs(case)
    want = _oracle_case(case, sample, torch.float64, d)
    low = _oracle_case(case, sample, torch.float32, d)
    st = _stove(cl, n_obj, variant, nonlinear, regime)
    got = _device_case(st, sample, d, num)
    key = f'rollout_grad.{"sample" if sample else "mean"}.cl{cl}.n{n_obj}'
    assert got['z'].shape == want['z'].shape
    e, gap = err(got['z'], want['z']), err(low['z'], want['z'])
    print(f'{key}.z: {e:.3g} (oracle f32 gap {gap:.3g})')
    check(key + '.z', e, regime_bar(3e-6, gap))
    _held_grads(key + '.grad_in', got['gin'], want['gin'], low['gin'])
    n = _held_grads(key + '.grad_param', got['grads'], want['grads'], low['grads'])
    assert n == (28 if variant == 'plain' else 40)
    if n_obj == 1:
        for k, v in got['grads'].items():
            if '.rel_cores.' in k or '.att_net.' in k:
                assert float(want['grads'][k].abs().max()) == 0.0 and float(v.abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------ 2. the action cycle
def _poison(*shapes):
    """NaN into blocks of the caching allocator that the next allocations of these sizes are served from"""
    for _ in range(2):
        blocks = [torch.full(s, float('nan'), device=DEV) for s in shapes]
        del blocks
    torch.cuda.synchronize()


CYCLES = [(32, 3, 3, 'analytic'), (32, 3, 9, 'analytic'), (16, 5, 3, 'init'), (64, 2, 9, 'analytic')]          # (cl, N, A, weights), num = 7


def _cycle_data(cl, n_obj, A, B=5, num=7):
    D = cl // 2
    g = torch.Generator().manual_seed(50000 + 100 * cl + 10 * n_obj + A)
    r = lambda *shape: _f32(torch.rand(*shape, generator=g, dtype=torch.float64))          # noqa: E731
    z_last = _f32(torch.cat([dyn_recursion_inputs(g, B, 1, n_obj, cl)[0][..., :2], dyn_state(g, B, n_obj, cl)], -1))
    return {'z_last': z_last, 'emb': r(B, A, n_obj, 4) - 0.5, 'app': r(B, n_obj, 3),
            'eps': _f32(torch.randn(B, num, n_obj, D, generator=g, dtype=torch.float64)),
            'wz': r(B, num, n_obj, D + 2), 'wq': r(B, num, n_obj, D)}


def _cycle_oracle(cl, n_obj, A, regime, d, sample, dtype):
    """O.rollout with an identity embedding, handed extra's action columns as its actions -> d z_last, d extra[..., :4], d app"""
    B, num = d['eps'].shape[:2]
    c, params = dyn_oracle(cl, n_obj, 'actapp', regime, dtype, 'relu')
    params = dict(params)
    params['dyn.action_embedding_layer.weight'] = torch.eye(4 * n_obj, dtype=dtype)
    params['dyn.action_embedding_layer.bias'] = torch.zeros(4 * n_obj, dtype=dtype)
    z0, a, ap = _leaf(d['z_last'], dtype), _leaf(d['emb'].reshape(B, A, 4 * n_obj), dtype), _leaf(d['app'], dtype)
    out = O.rollout(c, params, z0, num, a, ap, eps=[e.to(dtype) for e in d['eps'].unbind(1)] if sample else None)
    loss = (out[0] * d['wz'].to(dtype)).sum() + ((out[1] * d['wq'].to(dtype)).sum() if sample else 0)
    gz, ga, gp = torch.autograd.grad(loss, (z0, a, ap))
    return {'z_last': gz, 'extra_actions': ga.view(B, A, n_obj, 4), 'app': gp}


@pytest.mark.parametrize('sample', [False, True], ids=['mean', 'sample'])
@pytest.mark.parametrize('cl,n_obj,A,regime', CYCLES)
def test_extra_rows_accumulate_round_the_cycle(cl, n_obj, A, regime, sample):
    """ops.rollout on a given `extra` (B, A, N, 7) with num = 7: at A = 3 the rows are read 3 / 2 / 2 times and their gradients
    accumulate; at A = 9 rows 7 and 8 are read by no step and come back as exact zeros -- out of allocator blocks that held NaN.
    The oracle receives the action columns through an identity embedding (Linear(4 N, 4 N), weight 1, bias 0: its d actions IS
    d extra[..., :4], row by row) and the appearance columns as its appearance (their gradient is d extra[..., 4:] summed over A)."""
    from stove_amd import ops
    B, num, D = 5, 7, cl // 2
    d = _cycle_data(cl, n_obj, A, B, num)
    z_last, emb, app, eps, wz, wq = (d[k] for k in ('z_last', 'emb', 'app', 'eps', 'wz', 'wq'))
    want, low = (_cycle_oracle(cl, n_obj, A, regime, d, sample, dtype) for dtype in (torch.float64, torch.float32))

    st = _stove(cl, n_obj, 'actapp', regime=regime)
    dyn = st.dyn
    z0 = _dev(z_last, True)
    extra = torch.cat([emb, app[:, None].expand(-1, A, -1, -1)], -1).float().to(DEV).contiguous().requires_grad_()
    image, sink = dyn.kernel_params(0)
    assert sink is None
    out = ops.rollout(z0, extra, image, num, 2, dyn.use_elu, dyn.loop_consts(), eps=_dev(eps) if sample else None, want_logq=sample)
    loss = (out[0] * _dev(wz)).sum() + ((out[3] * _dev(wq)).sum() if sample else 0)
    _poison(tuple(extra.shape), tuple(z0.shape), (B, num, n_obj, D + 2), (ops.gnn_width(cl).size('stove_gnn_grad_floats'),))
    loss.backward()
    ge = extra.grad
    assert bool(torch.isfinite(ge).all()) and bool(torch.isfinite(z0.grad).all())
    if A > num:
        assert float(ge[:, num:].abs().max()) == 0.0 and float(want['extra_actions'][:, num:].abs().max()) == 0.0
        assert float(ge[:, :num].abs().max()) > 0.0
    got = {'z_last': z0.grad, 'extra_actions': ge[..., :4], 'app': ge[..., 4:].sum(1)}
    _held_grads(f'rollout_grad.cycle.{"sample" if sample else "mean"}.cl{cl}.A{A}', got, want, low)


# ------------------------------------------------------------------------------------------------ 3. against the differentiable loop
@pytest.mark.parametrize('n_obj', [3, 6])
def test_fused_sampling_gradients_equal_the_step_loops(n_obj):
    """Same model, same draws: Stove.rollout(sample=True, fused=True) under autograd against fused=None, which under autograd is
    the loop of single differentiable steps.  z within 1e-5 (test_fused_sampling_rollout_equals_the_step_loop's bar), log q
    1.5e-5; the gradients of z_last and of all parameters at the bars of group 1."""
    case = (32, n_obj, 'plain', 'relu', 'analytic', 7, 5)
    d = _inputs(case)
    st = _stove(32, n_obj, 'plain')
    loop = _device_case(st, True, d, 5, fused=None)
    fused = _device_case(st, True, d, 5, fused=True)
    check('rollout_grad.fused_vs_loop.z', err(fused['z'], loop['z']), 1e-5)
    check('rollout_grad.fused_vs_loop.log_q', err(fused['log_q'], loop['log_q']), 1.5e-5)
    assert set(fused['grads']) == set(loop['grads']) and len(loop['grads']) == 28
    for k, v in list(loop['gin'].items()) + list(loop['grads'].items()):
        check_grad('rollout_grad.fused_vs_loop.grad', fused['gin'][k] if k in fused['gin'] else fused['grads'][k], v, *BARS)


# ------------------------------------------------------------------------------------------------ 4. forward untouched, backward reproducible
@pytest.mark.parametrize('cl,n_obj', [(32, 3), (32, 7), (16, 3), (64, 6)])
def test_forward_is_bit_for_bit_the_no_grad_call_and_the_backward_reproducible(cl, n_obj):
    from stove_amd import ops
    case = (cl, n_obj, 'actapp', 'relu', 'analytic', 11, 7)
    d = _inputs(case)
    B, num, A, D = 11, 7, 3, cl // 2
    st = _stove(cl, n_obj, 'actapp')
    dyn = st.dyn
    g = torch.Generator().manual_seed(cl + n_obj)
    extra_v = torch.rand(B, A, n_obj, 7, generator=g).to(DEV)
    consts = dyn.loop_consts()
    for eps in (None, _dev(d['eps'])):
        with torch.no_grad():
            plain = ops.rollout(_dev(d['z_last']), extra_v, dyn.kernel_params(0)[0], num, 2, dyn.use_elu, consts, want_std=True,
                                want_pred=True, eps=eps, want_logq=eps is not None)
        assert all(t.grad_fn is None and not t.requires_grad for t in plain)
        runs = []
        for _ in range(2):
            dyn.zero_grad(set_to_none=True)
            z0, extra = _dev(d['z_last'], True), extra_v.clone().requires_grad_()
            out = ops.rollout(z0, extra, dyn.kernel_params(0)[0], num, 2, dyn.use_elu, consts, want_std=True, want_pred=True, eps=eps,
                              want_logq=eps is not None)
            assert len(out) == len(plain) == (3 if eps is None else 4)
            for u, v in zip(out, plain):
                assert torch.equal(u, v)
            assert out[0].requires_grad and out[2].requires_grad and not out[1].requires_grad
            loss = (out[0] * _dev(d['wz'])).sum() + (out[2] ** 2).sum() + ((out[3] * _dev(d['wq'])).sum() if eps is not None else 0)
            loss.backward()
            runs.append([z0.grad, extra.grad] + [p.grad.clone() for p in dyn.parameters() if p.grad is not None])
        assert len(runs[0]) == len(runs[1]) == 2 + 28
        for u, v in zip(*runs):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ 5. API
def test_mean_rollout_under_autograd_is_differentiable():
    """(on the parent commit ops.rollout ran under no_grad: z_pred came back without a grad_fn)"""
    st = _stove(32, 3, 'actapp')
    d = _inputs((32, 3, 'actapp', 'relu', 'analytic', 4, 3))
    z, zstd, rew = st.rollout(_dev(d['z_last']), num=3, return_std=True, actions=_dev(d['actions']), appearance=_dev(d['app']))
    assert z.requires_grad and z.grad_fn is not None and rew.requires_grad
    assert not zstd.requires_grad
    (z.sum() + rew.sum()).backward()
    named = dict(st.dyn.named_parameters())
    for k in ('state_enc.weight', 'out.0.1.bias', 'action_embedding_layer.weight', 'reward_head1.4.weight'):
        assert named[k].grad is not None and float(named[k].grad.abs().max()) > 0, k
    with torch.no_grad():
        z2, _ = st.rollout(_dev(d['z_last']), num=3, actions=_dev(d['actions']), appearance=_dev(d['app']))
    assert not z2.requires_grad and torch.equal(z2, z)
    # the sampling branch keeps its default: the loop under autograd, one launch only when asked for
    st.noise_fn = _feed(_dev(d['eps']))
    zs, lq, _ = st.rollout(_dev(d['z_last']), num=3, sample=True, actions=_dev(d['actions']), appearance=_dev(d['app']), fused=True)
    assert zs.requires_grad and lq.requires_grad


@pytest.mark.parametrize('cl', [32, 16])
def test_arena_gradients_land_in_the_arena_bit_for_bit(cl):
    from stove_amd.arena import ParamArena
    case = (cl, 3, 'act', 'relu', 'analytic', 6, 4)
    d = _inputs(case)
    plain = _device_case(_stove(cl, 3, 'act'), True, d, 4)
    st = _stove(cl, 3, 'act')
    arena = ParamArena(st.dyn)
    assert arena.has_gnn and st.dyn.kernel_params(0)[1] is not None
    got = _device_case(st, True, d, 4, arena=arena)
    assert torch.equal(got['z'], plain['z']) and torch.equal(got['gin']['z_last'], plain['gin']['z_last'])
    n = 0
    for k, p in st.dyn.named_parameters():
        if 'dyn.' + k not in plain['grads']:
            continue
        o = arena.offset[id(p)]
        assert p.grad is not None and p.grad.data_ptr() == arena.grad.data_ptr() + 4 * o, k          # the arena's own slice
        if k.startswith(('action_embedding_layer', 'reward_head')):      # (their kernels add into the slice themselves)
            assert err(p.grad, plain['grads']['dyn.' + k]) < 1e-6, k
        else:
            assert torch.equal(arena.grad[o:o + p.numel()].view(p.shape), plain['grads']['dyn.' + k]), k
            n += 1
    assert n == 28
    arena.check()


def test_rollout_backward_rejects_bad_arguments():
    """An invalid-value code that stove_error_string() names, nothing enqueued, the outputs untouched, the stream usable.  Only
    what validate.h refuses on the host: nothing here would reach a kernel."""
    from stove_amd import _lib
    lib = _lib.load()
    S = _lib.stream()
    B, N, num = 4, 3, 4
    p = _lib.ptr
    k = (0.3, 0.04, 0.04)

    def expect_invalid(code, what):
        assert code == INVALID, (what, code)
        msg = lib.stove_error_string(code)
        assert msg and b'invalid' in msg.lower(), (what, msg)
        torch.cuda.synchronize()
    for cl in (32, 16, 64):
        D = cl // 2
        if cl == 32:
            n_par, n_grad, ws_b = lib.stove_gnn_param_floats(), lib.stove_gnn_grad_floats(), lib.stove_rollout_bwd_ws_bytes(B, N)
        else:
            n_par, n_grad, ws_b = lib.stove_gnn_param_floats_cl(cl), lib.stove_gnn_grad_floats_cl(cl), lib.stove_rollout_bwd_ws_bytes_cl(cl, B, N)
        assert ws_b > 0
        params = torch.zeros(n_par, device=DEV)
        z1 = torch.zeros(B, N, D + 2, device=DEV)
        eps = torch.zeros(B, num, N, D, device=DEV)
        zp = torch.zeros(B, num, N, D + 2, device=DEV)
        dzp, dlq = torch.ones_like(zp), torch.ones_like(eps)
        dz1 = torch.full_like(z1, 7.0)
        gp = torch.full((n_grad,), 7.0, device=DEV)
        ws = torch.empty(ws_b // 4 + 1, device=DEV)

        def call(ptrs, *dims):
            if cl == 32:
                return lib.stove_rollout_bwd(*ptrs, *dims, 2, 0, *k, S)
            return lib.stove_rollout_bwd_cl(*ptrs, cl, *dims, 2, 0, *k, S)
        #       z_last extra params    eps     z_pred d_z_pred d_log_q d_pred d_z_last d_extra g_params ws
        good = [p(z1), None, p(params), p(eps), p(zp), p(dzp), p(dlq), None, p(dz1), None, p(gp), p(ws)]
        for i, what in ((3, 'd_log_q without eps'), (11, 'NULL workspace'), (0, 'NULL z_last'), (4, 'NULL z_pred'), (8, 'NULL d_z_last'),
                        (10, 'NULL g_params')):
            bad = list(good)
            bad[i] = None
            expect_invalid(call(bad, B, num, 1, N, D), f'cl {cl}: {what}')
        expect_invalid(call(good, B, num, 1, N, D + 4), f'cl {cl}: sin_dim > D without extra')
        expect_invalid(call(good, B, -1, 1, N, D), f'cl {cl}: num = -1')
        expect_invalid(call(good, B, num, 1, 9 if cl == 32 else 7, D), f'cl {cl}: N past the width\'s limit')
        assert float(dz1.min()) == 7.0 and float(gp.min()) == 7.0              # nothing was written
        assert call(good, B, num, 1, N, D) == 0                                # and the stream still works
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dz1).all()) and bool(torch.isfinite(gp).all()) and float(dz1.max()) < 7.0
        gp.fill_(7.0)
        dz1.fill_(7.0)
        assert call(good, B, 0, 1, N, D) == 0                                  # num = 0: everything comes back as zeros
        torch.cuda.synchronize()
        assert float(dz1.abs().max()) == 0.0 and float(gp.abs().max()) == 0.0
