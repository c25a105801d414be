"""GPU tests of the one-launch PPO update (stove_ppo_update, csrc/ppo_update.hip; ops.ppo_update; PPOAgent(fused=True)): the kernel
against the reference's recorded float64 updates (tests/golden/g25_ppo_update.npz) and, on edge shapes, against this project's
float64 torch update on the CPU.  The bar is 4 x the float32-to-float64 gap of the same update, per case and quantity, from
g25_reference_fp32_gap.json or from the in-test float32 torch run -- never from the kernel.  Every decision of the float64 runs
(clip range of the ratio and of the value, which squared error is larger, the sign of the advantage, whether the norm clips) has a
margin >= 1e-5, two orders above a float32 rounding, so both sides decide alike.  Nothing here reads the reference.  (All fail before
the feature: the symbol, ops.ppo_update and the `fused` keyword do not exist.)"""
import numpy as np
import pytest
import torch

import ppo_update_cases as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -77.0


def _device_update(shape, k, batch, max_steps=None, clipped=True, poison=True):
    """ops.ppo_update on device copies of the kernel inputs -> dict of numpy image, m, v, step, losses, gnorm, status"""
    from stove_amd import ops
    N, H, deep = shape
    E, n = k['perm'].shape
    M = batch['M']
    t = {key: torch.from_numpy(a).to(DEV) for key, a in k.items()}
    m, v, step = torch.zeros_like(t['image']), torch.zeros_like(t['image']), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = {'losses': torch.full((E * M, 3), POISON, device=DEV), 'gnorm': torch.full((E * M,), POISON, device=DEV),
           'status': torch.full((2,), -77, dtype=torch.int32, device=DEV)} if poison else None
    out = ops.ppo_update(t['image'], m, v, step, t['obs'], t['actions'], t['returns'], t['values'], t['logp'], t['adv'], t['perm'], M, H, deep,
                         *(batch[h] for h in U.HYPER), clipped, max_steps, out)
    res = {key: ten.cpu().numpy() for key, ten in out.items()}
    res.update(image=t['image'].cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), step=int(step.cpu()))
    return res


@pytest.mark.parametrize('c', U.CASES)
def test_kernel_holds_the_recorded_updates_to_the_bar(c):
    """the six g25 cases: parameters after the update, the losses of every step and the gradient norms"""
    G, batch, shape = U.golden(), U.golden_batch(c), U.GOLDEN_SHAPES[c // 2]
    out = _device_update(shape, U.kernel_inputs(U.golden_start(c), batch), batch)
    assert out['status'].tolist() == [0, 8] and out['step'] == 8
    got = U.distances(shape, out['image'], out['losses'], out['gnorm'], U.golden_after(c), G['c%d_losses' % c], G['c%d_gnorm' % c])
    U.hold_to_the_bar('case %d (kernel)' % c, got, U.gaps()['case%d' % c]['gap'])


@pytest.mark.parametrize('name', list(U.EDGES))
def test_kernel_holds_the_edge_shapes_to_the_bar(name):
    """shapes the fixture lacks -- an H that is no multiple of 32, the image that does not fit LDS, one object, a tile that is not
    full with rows dropped, one row per step, one step per epoch, one epoch -- against the float64 CPU run of PPOAgent.update"""
    shape, start, batch, r64, gap, seed, skipped = U.edge(name)
    assert skipped <= 1, 'more than one seed in four had a margin below 1e-5'
    E, M = U.EDGES[name][4:6]
    out = _device_update(shape, U.kernel_inputs(U.policy_of(shape, start), batch), batch)
    assert out['status'].tolist() == [0, E * M] and out['step'] == E * M
    U.hold_to_the_bar('%s (kernel, seed %d)' % (name, seed), U.distances(shape, out['image'], out['losses'], out['gnorm'], r64['sd'], r64['losses'],
                                                                       r64['gnorm']), gap)


def _agent_update(policy, batch, seed=0, **kw):
    """PPOAgent(fused=True).update on the device under torch.manual_seed(seed) -> the returned losses; policy is updated in place"""
    from stove_amd.rl.agents import PPOAgent
    E = batch['perm'].shape[0]
    agent = PPOAgent(policy.to(DEV), batch['clip'], E, batch['M'], batch['value_coef'], batch['entropy_coef'], lr=batch['lr'], eps=batch['eps'],
                     max_grad_norm=batch['max_grad_norm'], fused=True, **kw)
    col = lambda key: torch.from_numpy(np.asarray(batch[key], dtype=np.float32)).reshape(-1, 1).to(DEV)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    try:
        return agent.update(torch.from_numpy(batch['obs']).to(DEV), torch.from_numpy(np.asarray(batch['actions'])).long().reshape(-1, 1).to(DEV),
                            col('returns'), col('values'), col('logp'), col('adv'))
    finally:
        torch.set_rng_state(state)


def test_agent_without_the_clipped_value_loss_switch_follows_the_torch_update():
    """PPOAgent(fused=True, use_clipped_value_loss=False): the torch update never reads that switch (nor does the reference), so
    the fused agent computes the same clipped update; held to the float64 torch run with the switch off.  The permutations come from
    torch.randperm under the same seed on both sides."""
    shape, start, batch, r64, gap, seed, skipped = U.edge('e1')
    off = U.traced_update(U.policy_of(shape, start, torch.float64), batch, torch.float64, seed=0, use_clipped_value_loss=False)
    assert np.array_equal(off['perm'], batch['perm'])
    policy = U.policy_of(shape, start)
    returned = _agent_update(policy, batch, use_clipped_value_loss=False)
    got = max(float(np.abs(t.double().cpu().numpy() - off['sd'][k]).max()) for k, t in policy.state_dict().items())
    print(f'parameters off by {got:.3g} (bar {U.FACTOR * gap["params"]:.3g})')
    assert got <= U.FACTOR * gap['params']
    for q, value, want in zip(U.QUANTITIES[1:4], returned, off['returned']):
        assert abs(value - want) <= U.FACTOR * gap[q], q


def test_two_launches_agree_bit_for_bit():
    for name in ('n70_m4', 'n6_h128_deep'):
        shape, start, batch = U.edge(name)[:3]
        k = U.kernel_inputs(U.policy_of(shape, start), batch)
        a, b = _device_update(shape, k, batch), _device_update(shape, k, batch)
        for key in ('image', 'm', 'v', 'losses', 'gnorm'):
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), (name, key)
        assert a['status'].tolist() == b['status'].tolist() and a['step'] == b['step']


@pytest.mark.parametrize('k_steps', [0, 3, 8])
def test_max_steps_stops_there(k_steps):
    batch, shape = U.golden_batch(0), U.GOLDEN_SHAPES[0]
    k = U.kernel_inputs(U.golden_start(0), batch)
    out = _device_update(shape, k, batch, max_steps=k_steps)
    assert out['status'].tolist() == [0, k_steps] and out['step'] == k_steps
    assert (out['losses'][k_steps:] == POISON).all() and (out['gnorm'][k_steps:] == POISON).all()
    assert (out['losses'][:k_steps] != POISON).all() and (out['gnorm'][:k_steps] != POISON).all()
    if k_steps == 0:
        assert np.array_equal(out['image'], k['image']) and not out['m'].any() and not out['v'].any()
    if k_steps == 8:
        whole = _device_update(shape, k, batch)
        assert np.array_equal(whole['image'].view(np.int32), out['image'].view(np.int32))


@pytest.mark.parametrize('deep_case', [0, 2])
def test_a_nan_advantage_stops_the_update_at_its_step(deep_case):
    """a NaN in an input is data: status (3, k), everything bit for bit as a clean call with max_steps = k left it; an index of perm
    out of range stops the same way with status 2; PPOAgent.update raises"""
    c, step_k = deep_case, 5
    batch, shape = U.golden_batch(c), U.GOLDEN_SHAPES[c // 2]
    k = U.kernel_inputs(U.golden_start(c), batch)
    M, mb = batch['M'], 64 // batch['M']
    steps_of = lambda r: [at for at in range(8) if r in k['perm'][at // M][(at % M) * mb:(at % M + 1) * mb]]
    row = next(int(r) for r in k['perm'][step_k // M][(step_k % M) * mb:(step_k % M + 1) * mb] if steps_of(r)[0] > 0)
    first = steps_of(row)[0]                                    # (every row belongs to a step of the first epoch too: that one stops)
    assert 0 < first < step_k
    clean = _device_update(shape, k, batch, max_steps=first)
    bad = dict(k, adv=k['adv'].copy())
    bad['adv'][row] = np.nan
    out = _device_update(shape, bad, batch)
    assert out['status'].tolist() == [3, first] and out['step'] == first
    for key in ('image', 'm', 'v', 'losses', 'gnorm'):
        assert np.array_equal(out[key].view(np.int32), clean[key].view(np.int32)), key
    idx = dict(k, perm=k['perm'].copy())
    idx['perm'][first // M][(first % M) * mb + 1] = 64
    out = _device_update(shape, idx, batch)
    assert out['status'].tolist() == [2, first] and out['step'] == first
    for key in ('image', 'm', 'v', 'losses', 'gnorm'):
        assert np.array_equal(out[key].view(np.int32), clean[key].view(np.int32)), key
    nan_batch = dict(batch, adv=bad['adv'])
    with pytest.raises(RuntimeError, match='step %d' % first):
        _agent_update(U.golden_start(c), nan_batch)


def test_runner_with_a_fused_agent_matches_the_torch_agent():
    """PPORunner.run_batch_states on a device BatchedAvoidance, B = 4, S = 8, M = 4, E = 2: the same collection (the same uniforms) and
    the same torch seed, once with the torch agent and once with the fused one.  The bar: 4 x the gap between the float32 and the
    float64 torch update of that very batch, both run on the CPU."""
    import ppo_cases as P
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    from stove_amd.rl.runners import PPORunner
    u = np.random.RandomState(3).random_sample((4, 8)).astype(np.float32)
    after, outs = {}, {}
    for fused in (None, True):
        env = envs.BillardsEnv(n=3, granularity=2, seed=5)
        task = envs.AvoidanceTask(env, action_force=.3)
        policy = Policy(12, 9, hidden_size=64, base='control')
        policy.load_state_dict(P.policy(3, 64, False).state_dict())
        agent = PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused=fused)
        runner = PPORunner(env, task, None, DEV, agent, policy, num_steps=8, batch_size=4, discount=P.DISCOUNT)
        state = torch.get_rng_state()
        torch.manual_seed(1)
        outs[fused] = runner.run_batch_states(u=u)
        torch.set_rng_state(state)
        after[fused] = {k: t.detach().double().cpu().numpy() for k, t in policy.state_dict().items()}
    for k in ('obs', 'actions', 'returns', 'values', 'logp'):
        assert torch.equal(outs[None][k], outs[True][k]), k
    o = {k: t.cpu().numpy() for k, t in outs[None].items()}
    batch = {'obs': o['obs'][:, :-1].reshape(32, 12), 'actions': o['actions'].reshape(32), 'returns': o['returns'].reshape(32),
             'values': o['values'].reshape(32), 'logp': o['logp'].reshape(32), 'adv': (o['returns'] - o['values']).reshape(32), 'M': 4, 'E': 2,
             'clip': .1, 'value_coef': .5, 'entropy_coef': .01, 'lr': 2e-4, 'eps': 1e-5, 'max_grad_norm': 40.}
    start = P.policy(3, 64, False).state_dict()
    r64 = U.traced_update(U.policy_of((3, 64, False), start, torch.float64), batch, torch.float64, seed=1)
    r32 = U.traced_update(U.policy_of((3, 64, False), start), batch, torch.float32, seed=1)
    gap = U.gap_of(r64, r32)['params']
    assert min(r64['margins'].values()) >= U.MIN_MARGIN, r64['margins']
    moved = max(float(np.abs(after[True][k] - start[k].double().numpy()).max()) for k in start)
    for who in (None, True):
        got = max(float(np.abs(after[who][k] - r64['sd'][k]).max()) for k in start)
        print(f'fused={who}: parameters off the float64 update by {got:.3g} (bar {U.FACTOR * gap:.3g}); moved by {moved:.3g}')
        assert got <= U.FACTOR * gap
    apart = max(float(np.abs(after[True][k] - after[None][k]).max()) for k in start)
    print(f'the two agents are {apart:.3g} apart')
    assert apart <= U.FACTOR * gap and moved > 1e-4
