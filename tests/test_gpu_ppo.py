"""GPU tests of the PPO arm's one-launch collection (stove_ppo_collect, csrc/ppo_collect.hip; ops.ppo_collect; PPORunner on a device
batch): the kernel against the host forest PolicyForest -- the same text, csrc/ppo_policy.h, is held to that forest on the CPU by
tests/test_ppo_cpu.py -- bit for bit in obs, actions, rewards, values, next_value, returns, status and the final x, v; logp to one
float32 ulp.  The only library calls are exp and log, in the draw: every compared environment has a host decision margin >= 1e-9
(asserted, none dropped), seven orders of magnitude above a last-bit difference in exp, so both sides draw the same actions and
everything else is the same IEEE operations.  (All fail before the feature: the package and the symbols do not exist.)"""
import numpy as np
import pytest
import torch

import ppo_cases as P
from control_harness import guarded, margins_intact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOATS = ('obs', 'rewards', 'values', 'logp', 'next_value', 'returns')


def _device_collect(name, image=None, batch=None, graph=False):
    """ops.ppo_collect on guarded device copies of the case's start state, image and table; the outputs pre-filled with NaN / -77
    -> (out dict, the state tensors, every guarded buffer)"""
    from stove_amd import ops
    B, S, N, H, deep = P.CASES[name][:5]
    b = P.envs(name) if batch is None else batch
    image = P.policy(N, H, deep).flat_params() if image is None else image
    buffers, state, out = {}, {}, {}
    for k in ('x', 'v', 'r', 'm'):
        state[k], buffers[k] = guarded(torch.from_numpy(np.array(getattr(b, k))), float('nan'))
    params, buffers['params'] = guarded(image, float('nan'))
    u, buffers['u'] = guarded(torch.from_numpy(np.array(P.table(name))), float('nan'))
    shapes = {'obs': (B, S + 1, 4 * N), 'actions': (B, S), 'rewards': (B, S), 'values': (B, S), 'logp': (B, S), 'next_value': (B,),
              'returns': (B, S), 'status': (B,)}
    for k, shape in shapes.items():
        fill = torch.full(shape, float('nan')) if k in FLOATS else torch.full(shape, -77, dtype=torch.int32)
        out[k], buffers[k] = guarded(fill, float('nan') if k in FLOATS else -77)
    call = lambda: ops.ppo_collect(state['x'], state['v'], state['r'], state['m'], params, u, H, deep, b.granularity, b.hw, b.t, b.friction,
                                   b.action_force, b.drift, P.DISCOUNT, out=out)
    if not graph:
        call()
    else:
        fresh = {k: ten.clone() for k, ten in list(state.items()) + list(out.items())}
        restore = lambda: [ten.copy_(fresh[k]) for k, ten in list(state.items()) + list(out.items())]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        restore()                                           # (a capture runs nothing)
        g.replay()
    torch.cuda.synchronize()
    return out, state, buffers


def _assert_equals_host(out, state, name, rows=None):
    host, x, v, margin = P.host_collect(name)
    assert (margin >= P.MIN_MARGIN).all() and not host['status'].any()               # every environment, none dropped
    rows = slice(None) if rows is None else rows
    got = {k: ten.cpu().numpy() for k, ten in out.items()}
    for k in ('obs', 'rewards', 'values', 'next_value', 'returns'):
        assert np.array_equal(got[k][rows].view(np.int32), host[k][rows].view(np.int32)), k
    assert np.array_equal(got['actions'][rows], host['actions'][rows]) and np.array_equal(got['status'][rows], host['status'][rows])
    assert np.array_equal(state['x'].cpu().numpy()[rows].view(np.int64), x[rows].view(np.int64))
    assert np.array_equal(state['v'].cpu().numpy()[rows].view(np.int64), v[rows].view(np.int64))
    worst = int(P.ulps32(got['logp'][rows], host['logp'][rows]).max()) if host['logp'][rows].size else 0
    assert worst <= 1, worst
    return worst


# ------------------------------------------------------------------------------------------------ 1. kernel = host forest
@pytest.mark.parametrize('name', list(P.CASES))
def test_kernel_equals_the_host_forest_bit_for_bit(name):
    out, state, buffers = _device_collect(name)
    worst = _assert_equals_host(out, state, name)
    print(f'{name}: smallest host decision margin {P.host_collect(name)[3].min():.3g}, logp within {worst} ulp')
    for k in ('r', 'm'):
        assert np.array_equal(state[k].cpu().numpy(), getattr(P.envs(name), k)), k
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 2. non-finite outputs
def _untouched(out, rows):
    for k, ten in out.items():
        if k == 'status':
            continue
        part = ten[rows].cpu()
        assert bool(torch.isnan(part).all()) if k in FLOATS else bool((part == -77).all()), k


@pytest.mark.parametrize('name', ['b5_s16_n6_h64_deep', 'b4_s8_n3_h128_deep'])
def test_a_nan_weight_stops_every_environment_with_nothing_written(name):
    """on the staged image and on the one read from global memory"""
    B, S, N, H, deep = P.CASES[name][:5]
    image = P.policy(N, H, deep).flat_params().clone()
    image[7] = float('nan')
    b = P.envs(name)
    out, state, buffers = _device_collect(name, image=image)
    assert out['status'].tolist() == [3] * B
    _untouched(out, slice(None))
    assert np.array_equal(state['x'].cpu().numpy(), b.x) and np.array_equal(state['v'].cpu().numpy(), b.v)
    margins_intact(buffers)


def test_a_non_finite_environment_spares_its_wave_and_block_mates():
    """an infinite velocity of ball 1 in environment 1 of 'b5_s16_n6_h64_deep' (block mates 0, 2, 3; environment 4 in the next block):
    status 3 at step 0 and nothing of it written; every other environment bit-equal to the clean run"""
    name = 'b5_s16_n6_h64_deep'
    b = P.envs(name)
    b.v[1, 1, 0] = np.inf
    start_x, start_v = b.x.copy(), b.v.copy()
    out, state, buffers = _device_collect(name, batch=b)
    assert out['status'].tolist() == [0, 3, 0, 0, 0]
    _untouched(out, 1)
    assert np.array_equal(state['x'].cpu().numpy()[1], start_x[1]) and np.array_equal(state['v'].cpu().numpy()[1], start_v[1])
    _assert_equals_host(out, state, name, rows=[0, 2, 3, 4])
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 3. empty calls
def test_empty_collections_are_accepted():
    from stove_amd import _lib, ops
    assert _lib.load().stove_ppo_collect(*([None] * 14), 0, 8, 3, 64, 0, 5, 0, 10.0, 1.0, 0.0, 0.3, 0.95, None) == 0
    image = P.policy(3, 64, False).flat_params().to(DEV)
    e = torch.zeros(0, 3, 2, dtype=torch.float64, device=DEV)
    s = torch.zeros(0, 3, dtype=torch.float64, device=DEV)
    out = ops.ppo_collect(e, e, s, s, image, torch.zeros(0, 8, device=DEV), 64, False, 5, 10.0)
    assert tuple(out['obs'].shape) == (0, 9, 12) and tuple(out['status'].shape) == (0,)
    # S = 0: the observation, next_value and status only
    b = P.envs('b3_s5_n3_h64')
    state = [torch.from_numpy(np.array(getattr(b, k))).to(DEV) for k in ('x', 'v', 'r', 'm')]
    out = ops.ppo_collect(*state, image, torch.zeros(3, 0, device=DEV), 64, False, b.granularity, b.hw, b.t, b.friction, b.action_force)
    host = P.host_collect('b3_s5_n3_h64')[0]
    assert out['status'].tolist() == [0] * 3 and tuple(out['returns'].shape) == (3, 0)
    assert np.array_equal(out['obs'].cpu().numpy()[:, 0], host['obs'][:, 0]) and np.array_equal(out['next_value'].cpu().numpy(), host['values'][:, 0])
    assert np.array_equal(state[0].cpu().numpy(), b.x) and np.array_equal(state[1].cpu().numpy(), b.v)


# ------------------------------------------------------------------------------------------------ 4. graph capture
def test_captured_collection_replays_bit_for_bit():
    name = 'b5_s16_n6_h64_deep'
    out, state, buffers = _device_collect(name, graph=True)
    _assert_equals_host(out, state, name)
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 5. the runner
COMPOSED_MARGIN = 1e-4


def _runner(device, case=0, B=4, S=8, seed=5):
    """a runner on the reference's seeded policy of golden case `case` (N = 3, H = 64), main_rl's environment settings"""
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.runners import PPORunner
    env = envs.BillardsEnv(n=3, granularity=2, seed=seed)
    task = envs.AvoidanceTask(env, action_force=.3)
    policy = P.golden_policy(case)
    agent = PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
    return PPORunner(env, task, None, device, agent, policy, num_steps=S, batch_size=B, discount=P.DISCOUNT)


def test_fused_and_composed_collections_agree():
    """The same start states, the same table u: equal actions, rewards and states (bit for bit: once the actions agree the float64
    steps are the same operations).  Fair because the host forest's smallest decision margin on this table is >= 1e-4 (asserted): torch's
    GEMM order moves a logit by about 4e-7 (the recorded float32 gap), and so a cumulative probability by about as much, more than two
    orders below.  values and logp differ by that GEMM order; the bar is the one of tests/test_ppo_cpu.py, 4 x the reference's recorded
    float32 gap of this policy (value 2.5e-7, logp 1.3e-6)."""
    from stove_amd.rl.collect import PolicyForest
    gap = P.fp32_gap()['case0']
    u = np.random.RandomState(11).random_sample((4, 8)).astype(np.float32)
    twin = _runner(None)
    forest = PolicyForest.from_policy(twin.actor_critic)
    host = forest.collect(twin.start_batch(4), u, P.DISCOUNT)
    print(f'smallest host decision margin {forest.margin.min():.3g}')
    assert (forest.margin >= COMPOSED_MARGIN).all()
    state = torch.get_rng_state()
    outs = {}
    for fused in (True, False):
        torch.manual_seed(2)
        runner = _runner(DEV)
        out = runner.run_batch_states(fused=fused, u=u)
        outs[fused] = ({k: ten.cpu().numpy() for k, ten in out.items()}, runner.last_batch.x.cpu().numpy(), runner.last_batch.v.cpu().numpy())
    torch.set_rng_state(state)
    (a, ax, av), (c, cx, cv) = outs[True], outs[False]
    assert np.array_equal(a['actions'], host['actions']) and np.array_equal(a['obs'], host['obs'])          # the kernel is the forest
    assert np.array_equal(a['actions'], c['actions']) and np.array_equal(a['rewards'], c['rewards']) and np.array_equal(a['obs'], c['obs'])
    assert np.array_equal(ax.view(np.int64), cx.view(np.int64)) and np.array_equal(av.view(np.int64), cv.view(np.int64))
    dv = max(np.abs(a['values'] - c['values']).max(), np.abs(a['next_value'] - c['next_value']).max())
    dl = np.abs(a['logp'] - c['logp']).max()
    print(f'fused against composed: values differ by {dv:.3g} (bar {4 * gap["value"]:.3g}), logp by {dl:.3g} (bar {4 * gap["eval_logp"]:.3g})')
    assert dv <= 4 * gap['value'] and dl <= 4 * gap['eval_logp']
    with pytest.raises(ValueError, match='fused=True'):
        _runner(None).run_batch_states(fused=True)


def test_two_fused_batches_train_the_policy():
    state = torch.get_rng_state()
    torch.manual_seed(3)
    np_state = np.random.get_state()
    np.random.seed(3)
    runner = _runner(DEV)
    before = {k: v.detach().clone() for k, v in runner.actor_critic.state_dict().items()}
    first = runner.run_batch_states(fused=True)
    middle = {k: v.detach().clone() for k, v in runner.actor_critic.state_dict().items()}
    second = runner.run_batch_states(fused=True)
    np.random.set_state(np_state)
    torch.set_rng_state(state)
    after = runner.actor_critic.state_dict()
    assert runner.batch_counter == 2 and not first['status'].any() and not second['status'].any()
    assert any(not torch.equal(before[k], middle[k]) for k in before) and any(not torch.equal(middle[k], after[k]) for k in before)
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert not torch.equal(first['obs'], second['obs'])                               # fresh start states


# ------------------------------------------------------------------------------------------------ 6. argument checks
def test_ops_ppo_collect_checks_its_arguments():
    from stove_amd import ops
    name = 'b3_s5_n3_h64'
    b = P.envs(name)
    x, v, r, m = (torch.from_numpy(np.array(getattr(b, k))).to(DEV) for k in ('x', 'v', 'r', 'm'))
    image = P.policy(3, 64, False).flat_params().to(DEV)
    u = torch.from_numpy(np.array(P.table(name))).to(DEV)
    call = lambda x=x, v=v, r=r, m=m, image=image, u=u, H=64, deep=False, out=None: ops.ppo_collect(x, v, r, m, image, u, H, deep, 5, 10.0, out=out)
    with pytest.raises(RuntimeError, match='x must be a contiguous float64 tensor'):
        call(x=x.float())
    with pytest.raises(RuntimeError, match='v must be a tensor on the GPU'):
        call(v=v.cpu())
    with pytest.raises(RuntimeError, match='r must be a contiguous float64'):
        call(r=r.t().contiguous().t())
    with pytest.raises(ValueError, match='argument shapes do not fit B = 3'):
        call(m=m[:2].contiguous())
    with pytest.raises(RuntimeError, match='params must be a contiguous float32 tensor'):
        call(image=image.double())
    with pytest.raises(RuntimeError, match='u must be a contiguous float32 tensor'):
        call(u=u.cpu())
    with pytest.raises(ValueError, match=r'params is .* the policy needs'):
        call(H=40)
    with pytest.raises(ValueError, match=r'params is .* the policy needs'):
        call(deep=True)
    with pytest.raises(ValueError, match='head widths 1 .. 128'):
        call(H=129)
    with pytest.raises(ValueError, match=r'u is .* the batch needs \(3, S\)'):
        call(u=u[:2].contiguous())
    good = call()
    assert good['status'].tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match='out actions must be a contiguous int32'):
        call(out=dict(good, actions=good['actions'].long()))
    with pytest.raises(ValueError, match='out obs is'):
        call(out=dict(good, obs=good['obs'][:, :5].contiguous()))
    with pytest.raises(RuntimeError, match='out status must be'):
        call(out={k: t for k, t in good.items() if k != 'status'})
