"""CPU-side checks (-m "not gpu") of the model-free PPO arm: Policy and the host forest PolicyForest of stove_amd/rl held to the
reference's recorded outputs (tests/golden/g24_ppo.npz); evaluate_actions, PPOAgent.update and the returns in float64; the forest
against a plain per-environment loop over AvoidanceTask.step; the text the kernel runs, stove_amd/csrc/ppo_policy.h, compiled host-only
under sanitizers with contraction off (tests/abi/ppo_collect_driver.cpp) and held to PolicyForest bit for bit; reset(); the C ABI
addition refusing host-visible nonsense.  (All fail before the feature: the header, the package and the symbols do not exist.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import control_harness
import ppo_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logsumexp64(logits):
    l = logits.astype(np.float64)
    top = l.max(axis=1, keepdims=True)
    return l - top - np.log(np.exp(l - top).sum(axis=1, keepdims=True))


# ------------------------------------------------------------------------------------------------ 1. the policy = the reference
@pytest.mark.parametrize('case', range(3))
def test_policy_and_forest_reproduce_the_reference(case):
    """Policy in float32 (torch's GEMM order) and PolicyForest (one serial float32 sum per neuron) against the reference's float64 value
    and normalised logits.  The bar is 4 x the reference's own float32-to-float64 gap, recorded per case in
    g24_reference_fp32_gap.json (value 6.3e-8 / 1.6e-8 / 1.0e-7, logits 3.7e-7 / 3.7e-7 / 4.2e-7): a serial sum of K terms may err
    about twice as far as the pairwise / blocked sum behind the recorded gap, and the normalisation adds its own rounding.  Measured:
    Policy (the reference's own float32 arithmetic on a CPU, so the gap itself) value 6.3e-8 / 1.6e-8 / 1.0e-7, logits 3.7e-7 / 3.7e-7 /
    4.2e-7; PolicyForest value 6.4e-8 / 3.0e-8 / 6.0e-8 (bars 2.5e-7 / 6.6e-8 / 4.1e-7), logits 1.1e-7 / 4.2e-8 / 1.2e-7 (bars 1.5e-6 /
    1.5e-6 / 1.7e-6)."""
    G, N = P.golden(), P.GOLDEN_SHAPES[case][0]
    gap = P.fp32_gap()['case%d' % case]
    assert gap['shape'] == list(P.GOLDEN_SHAPES[case])
    pre = 'c%d_' % case
    obs = G[pre + 'obs']
    assert obs.shape == (64, 4 * N) and obs.dtype == np.float32
    policy = P.golden_policy(case)
    with torch.no_grad():
        value, dist = policy.head(policy.base(torch.from_numpy(obs)))
    from stove_amd.rl.collect import PolicyForest
    heads = PolicyForest.from_policy(policy).forward(obs)
    for who, val, logits in (('Policy', value.numpy()[:, 0], dist.logits.numpy().astype(np.float64)),
                             ('PolicyForest', heads[:, 0], _logsumexp64(heads[:, 1:]))):
        dv = np.abs(val.astype(np.float64) - G[pre + 'value64'][:, 0]).max()
        dl = np.abs(logits - G[pre + 'logits64']).max()
        print(f'case {case} {who}: value off by {dv:.3g} (bar {4 * gap["value"]:.3g}), logits by {dl:.3g} (bar {4 * gap["logits"]:.3g})')
        assert dv <= 4 * gap['value'] and dl <= 4 * gap['logits'], who
    # in float64 the classes are the reference's, to rounding
    p64 = P.golden_policy(case, torch.float64)
    with torch.no_grad():
        value, dist = p64.head(p64.base(torch.from_numpy(obs).double()))
    assert np.abs(value.numpy() - G[pre + 'value64']).max() <= 1e-12 and np.abs(dist.logits.numpy() - G[pre + 'logits64']).max() <= 1e-12


@pytest.mark.parametrize('case', range(3))
def test_evaluate_actions_and_update_reproduce_the_reference_in_float64(case):
    """to 1e-10 of each tensor's largest entry"""
    from stove_amd.rl.agents import PPOAgent
    G, pre = P.golden(), 'c%d_' % case
    close = lambda got, want: np.abs(np.asarray(got) - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-300)
    policy = P.golden_policy(case, torch.float64)
    obs, actions = torch.from_numpy(G[pre + 'obs']).double(), torch.from_numpy(G[pre + 'actions']).reshape(-1, 1)
    with torch.no_grad():
        value, logp, entropy = policy.evaluate_actions(obs, actions)
    assert close(value.numpy(), G[pre + 'eval_value64']) and close(logp.numpy(), G[pre + 'eval_logp64'])
    assert close(entropy.numpy(), G[pre + 'eval_entropy64'])
    agent = PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
    state = torch.get_rng_state()
    torch.manual_seed(0)
    losses = agent.update(obs, actions, *(torch.from_numpy(G[pre + 'upd_' + k]) for k in ('returns', 'values', 'logp', 'adv')))
    torch.set_rng_state(state)
    assert close(np.array(losses), G[pre + 'upd_losses'])
    moved = 0.0
    for key, ten in policy.state_dict().items():
        assert close(ten.numpy(), G[pre + 'upd_sd_' + key]), key
        moved = max(moved, float(np.abs(G[pre + 'upd_sd_' + key] - G[pre + 'sd_' + key]).max()))
    assert moved > 1e-4                                         # (the update did something)


def test_returns_reproduce_the_reference():
    """Runner._calculate_returns, PolicyForest.discounted: float32, a multiply and an add per step -- the golden bit for bit"""
    from stove_amd.rl.collect import PolicyForest
    from stove_amd.rl.runners import Runner
    G = P.golden()
    runner = Runner.__new__(Runner)
    runner.discount = 0.95
    rewards, nxt = torch.from_numpy(G['ret_rewards']), torch.from_numpy(G['ret_next'])
    got = runner._calculate_returns(nxt, rewards, torch.zeros_like(rewards)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), G['ret_out'].view(np.int32))
    host = PolicyForest.discounted(G['ret_rewards'][:, :, 0], G['ret_next'][:, 0], 0.95)
    assert np.array_equal(host.view(np.int32), G['ret_out'][:, :, 0].view(np.int32))


# ------------------------------------------------------------------------------------------------ 2. the forest = plain loops
# the numpy class against envs.py: tests/test_env_batched_cpu.py's bar (100 x the deviation it measured, BLAS norms and dots against the
# plain forms in the last bit)
ENVS_PY_BAR = 8.62e-12


def _naive(name, on_task):
    """one environment after the other, one step per step, the policy row by row through PolicyForest's functions.  on_task: the step
    is AvoidanceTask.step of envs.py; else BatchedAvoidance.step of a batch of that one environment"""
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.rl.collect import PolicyForest
    B, S, N, H, deep = P.CASES[name][:5]
    f = PolicyForest.from_policy(P.policy(N, H, deep))
    tasks, u = P.envs(name).tasks(), P.table(name)
    out = {'actions': np.zeros((B, S), np.int32), 'rewards': np.zeros((B, S), np.float32), 'states': np.zeros((B, S + 1, N, 4))}
    for b, task in enumerate(tasks):
        one = None if on_task else BatchedAvoidance.from_tasks([task])
        state = lambda: np.concatenate([task.env.x, task.env.v], axis=1) if on_task else one.state()[0]
        for s in range(S):
            out['states'][b, s] = state()
            heads = f.forward(f.observe(out['states'][b, s, None, :, :2], out['states'][b, s, None, :, 2:]))
            a = int(f.draw(heads[:, 1:], u[b, s:s + 1])[0][0])
            reward = task.step(a)[2] if on_task else one.step(np.array([a]), render=False)[1][0]
            out['actions'][b, s], out['rewards'][b, s] = a, reward
        out['states'][b, S] = state()
    return out


@pytest.mark.parametrize('name', ['b3_s5_n3_h64', 'b5_s16_n6_h64_deep', 'b4_s8_n3_g2', 'b4_s8_n3_fric'])
def test_forest_equals_a_plain_loop_per_environment(name):
    """Against a per-environment loop over one-environment batches: states bit for bit, actions and rewards equal.  Against the same
    loop over AvoidanceTask.step of envs.py: actions and rewards equal, the float32 observations equal, and the float64 states within
    the bar tests/test_env_batched_cpu.py holds the numpy class to -- envs.py takes its norms and dot products from BLAS, which
    differs from the plain forms in the last bit after a collision (measured here: at most 1.2e-15 in v, 0 in x)."""
    B, S, N = P.CASES[name][:3]
    host, x, v, margin = P.host_collect(name)
    assert not host['status'].any() and (margin >= P.MIN_MARGIN).all()
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    for on_task in (False, True):
        naive = _naive(name, on_task)
        assert np.array_equal(host['actions'], naive['actions']) and np.array_equal(host['rewards'], naive['rewards'])
        assert np.array_equal(host['obs'], naive['states'].reshape(B, S + 1, 4 * N).astype(np.float32))
        last = naive['states'][:, S]
        if on_task:
            print(f'{name}: envs.py differs by {np.abs(x - last[:, :, :2]).max():.3g} in x, {np.abs(v - last[:, :, 2:]).max():.3g} in v')
            assert np.abs(x - last[:, :, :2]).max() <= ENVS_PY_BAR and np.abs(v - last[:, :, 2:]).max() <= ENVS_PY_BAR
        else:
            assert np.array_equal(bits(x), bits(last[:, :, :2])) and np.array_equal(bits(v), bits(last[:, :, 2:]))
    assert len({tuple(r) for r in host['actions']}) > 1 or B == 1      # the draw matters: the environments act differently


def test_case_shapes_cover_what_they_claim():
    from stove_amd.rl.collect import param_floats
    shapes = {n: c[:5] for n, c in P.CASES.items()}
    assert {s[0] for s in shapes.values()} >= {1, 3, 4, 5, 32} and {s[2] for s in shapes.values()} == {1, 3, 6}
    assert {s[3] for s in shapes.values()} >= {32, 40, 64, 128} and {s[4] for s in shapes.values()} == {False, True}
    assert P.CASES['b4_s8_n3_g2'][5] == 2 and P.action_force('b4_s8_n3_g2') == 0.3 and P.CASES['b4_s8_n3_fric'][6] > 0
    # 160 KiB of LDS hold a block's rows (6016 bytes) and the image of every case but the H = 128 deep one
    fits = {n: 6016 + 4 * param_floats(s[2], s[3], s[4]) <= 160 * 1024 for n, s in shapes.items()}
    assert [n for n, ok in fits.items() if not ok] == ['b4_s8_n3_h128_deep']
    for name in P.CASES:
        out, _, _, margin = P.host_collect(name)
        print(f'{name}: smallest decision margin {margin.min():.3g}')
        assert (margin >= P.MIN_MARGIN).all() and not out['status'].any()


def test_forest_stops_an_environment_with_a_non_finite_output():
    from stove_amd.rl.collect import PolicyForest
    name = 'b4_s8_n3_h40'
    B, S, N, H, deep = P.CASES[name][:5]
    clean, x, v, _ = P.host_collect(name)
    policy = P.policy(N, H, deep)
    image = policy.flat_params().numpy().copy()
    image[7] = np.nan
    b = P.envs(name)
    x0, v0 = b.x.copy(), b.v.copy()
    out = PolicyForest(image, N, H, deep).collect(b, P.table(name), P.DISCOUNT)
    assert out['status'].tolist() == [3] * B and all(not out[k].any() for k in out if k != 'status')
    assert np.array_equal(b.x, x0) and np.array_equal(b.v, v0)
    b = P.envs(name)
    b.v[2, 1, 0] = np.inf
    out = PolicyForest.from_policy(policy).collect(b, P.table(name), P.DISCOUNT)
    assert out['status'].tolist() == [0, 0, 3, 0] and all(not out[k][2].any() for k in out if k != 'status')
    for k in out:
        assert np.array_equal(out[k][[0, 1, 3]], clean[k][[0, 1, 3]]), k
    assert np.array_equal(b.x[[0, 1, 3]], x[[0, 1, 3]]) and np.array_equal(b.v[[0, 1, 3]], v[[0, 1, 3]])


# ------------------------------------------------------------------------------------------------ 3. the header on the CPU
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'ppo_collect_driver')


def _drive(exe, tmp_path, name):
    B, S, N, H, deep = P.CASES[name][:5]
    b = P.envs(name)
    outputs = [('obs', (B, S + 1, 4 * N), np.float32), ('actions', (B, S), np.int32), ('rewards', (B, S), np.float32), ('values', (B, S), np.float32),
               ('logp', (B, S), np.float32), ('next_value', (B,), np.float32), ('returns', (B, S), np.float32), ('status', (B,), np.int32),
               ('x', (B, N, 2), np.float64), ('v', (B, N, 2), np.float64), ('margin', (B,), np.float64)]
    arrays = [np.asarray(a, dtype=np.float64) for a in (b.x, b.v, b.r, b.m)] + [P.policy(N, H, deep).flat_params().numpy(), P.table(name)]
    return control_harness.run_driver(exe, tmp_path, [B, S, N, H, deep, b.granularity, b.drift], [b.hw, b.t, b.friction, b.action_force, P.DISCOUNT],
                                      arrays, outputs)


def assert_equals_host(got, name, rows=None):
    """everything bit for bit but logp, which is within one float32 ulp (exp and log are library calls)"""
    host, x, v, margin = P.host_collect(name)
    rows = slice(None) if rows is None else rows
    for k in ('obs', 'rewards', 'values', 'next_value', 'returns'):
        assert np.array_equal(got[k][rows].view(np.int32), host[k][rows].view(np.int32)), k
    assert np.array_equal(got['actions'][rows], host['actions'][rows]) and np.array_equal(got['status'][rows], host['status'][rows])
    assert np.array_equal(got['x'][rows].view(np.int64), x[rows].view(np.int64)) and np.array_equal(got['v'][rows].view(np.int64), v[rows].view(np.int64))
    worst = int(P.ulps32(got['logp'][rows], host['logp'][rows]).max()) if host['logp'][rows].size else 0
    assert worst <= 1, worst
    return worst


@pytest.mark.parametrize('name', list(P.CASES))
def test_header_equals_the_host_forest_bit_for_bit(driver, tmp_path, name):
    out = _drive(driver, tmp_path, name)
    margin = P.host_collect(name)[3]
    assert (margin >= P.MIN_MARGIN).all()                             # every environment: exp is a library call on either side
    worst = assert_equals_host(out, name)
    assert np.allclose(out['margin'], margin, rtol=0, atol=1e-12)
    print(f'{name}: smallest host decision margin {margin.min():.3g}, logp within {worst} ulp')


def test_validation_and_status_under_sanitizers(driver):
    """stove_ppo_collect's host-side argument check (csrc/validate.h: ppo_collect) through the driver: every documented bad argument
    returns hipErrorInvalidValue, empty calls are accepted, nothing is dereferenced; status 3: a NaN weight stops every environment with
    nothing written, an infinite velocity stops its environment alone; nothing read or written out of bounds."""
    control_harness.run_modes(driver, ['validate', 'status'])


def test_reset_consumes_the_stream_as_the_reference_does():
    from stove_amd.envs import envs
    G = P.golden()
    assert int(G['resets']) == 4
    for k in range(int(G['resets'])):
        env = envs.BillardsEnv(n=int(G['reset%d_n' % k]), seed=int(G['reset%d_seed' % k]))
        task = envs.AvoidanceTask(env)
        assert env.get_state_shape() == (env.n, 4)
        for i in range(3):
            env.reset()
            task.step(0)
            assert np.array_equal(env.x, G['reset%d_x' % k][i]) and np.array_equal(env.v, G['reset%d_v' % k][i]), (k, i)


def _runner(B=4, S=8, device=None, H=64, **kw):
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    from stove_amd.rl.runners import PPORunner
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, action_force=.3)
    policy = Policy(12, 9, hidden_size=H, base='control')
    policy.load_state_dict(P.policy(3, H, False).state_dict())
    agent = PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
    return PPORunner(env, task, None, device, agent, policy, num_steps=S, batch_size=B, discount=P.DISCOUNT, **kw)


def test_runner_collects_and_trains_on_the_host():
    class Writer:
        rows = []

        def add_scalar(self, key, value, step):
            self.rows.append((key, float(value), step))

    state = torch.get_rng_state()
    torch.manual_seed(1)
    runner = _runner(writer=Writer())
    before = {k: v.clone() for k, v in runner.actor_critic.state_dict().items()}
    u = np.random.RandomState(3).random_sample((4, 8)).astype(np.float32)
    out = runner.run_batch_states(u=u)
    assert tuple(out['obs'].shape) == (4, 9, 12) and tuple(out['actions'].shape) == (4, 8) and not out['status'].any()
    # the start states are the reference's: reset() + one step with action 0, one after the other on the one environment
    from stove_amd.envs import envs
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, action_force=.3)
    for b in range(4):
        env.reset()
        task.step(0)
        assert np.array_equal(out['obs'][b, 0].numpy(), np.concatenate([env.x, env.v], 1).reshape(-1).astype(np.float32))
    after = runner.actor_critic.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before) and all(bool(torch.isfinite(v).all()) for v in after.values())
    assert runner.batch_counter == 1 and {r[0] for r in Writer.rows} == {'/losses/value_loss', '/losses/action_loss', '/losses/entropy',
                                                                         '/info/rewards'}
    assert isinstance(runner._test_actorcritic(2, 3), float)
    with pytest.raises(ValueError, match='fused=True'):
        runner.run_batch_states(fused=True)
    torch.set_rng_state(state)


def test_a_reference_keyed_state_dict_loads_and_the_packages_import():
    from stove_amd.rl.rl_model import DiscreteActionHead, Policy, SimpleCNNBase, SimpleControlBase
    G = P.golden()
    keys = {k[len('c0_sd_'):] for k in G.files if k.startswith('c0_sd_')}
    policy = Policy(12, 9, hidden_size=64, base='control')
    assert set(policy.state_dict()) == keys == {'base.main.0.weight', 'base.main.0.bias', 'base.main.2.weight', 'base.main.2.bias',
                                               'head.main.weight', 'head.main.bias', 'head.in_between.0.weight', 'head.in_between.0.bias',
                                               'head.in_between.2.weight', 'head.in_between.2.bias', 'head.values_head.weight',
                                               'head.values_head.bias', 'head.actor_head.weight', 'head.actor_head.bias'}
    assert isinstance(P.golden_policy(0).base, SimpleControlBase) and isinstance(policy.head, DiscreteActionHead)
    image = Policy((32, 32, 12), 9, hidden_size=512)
    assert isinstance(image.base, SimpleCNNBase) and set(image.state_dict()) >= {'base.main.0.weight', 'base.main.2.bias', 'head.main.weight'}
    value, action, logp = image.act(torch.zeros(2, 12, 32, 32))
    assert tuple(value.shape) == (2, 1) and tuple(action.shape) == (2,) and tuple(logp.shape) == (2, 1)
    assert image.kernel_shape() is None and policy.kernel_shape() == (3, 64, False)
    with pytest.raises(ValueError, match='flat_params'):
        image.flat_params()
    import model.rl.agents as ma
    import model.rl.collect as mc
    import model.rl.main_rl as mm
    import model.rl.rl_model as mr
    import model.rl.runners as mu
    from stove_amd.rl import agents, collect, main_rl, runners
    assert mr.Policy is Policy and ma.PPOAgent is agents.PPOAgent and mc.PolicyForest is collect.PolicyForest
    assert mu.PPORunner is runners.PPORunner and mu.BatchStorage is runners.BatchStorage and mm.parse_args is main_rl.parse_args
    args = main_rl.parse_args(['--use-states', '--experiment_id', 'x', '--device-envs', '--num-balls', '4'])
    assert args.use_states and args.device_envs and args.num_balls == 4 and args.gran == 2 and args.action_force == .3
    assert args.num_steps == 128 and args.batch_size == 32 and args.num_ppo_mb == 32 and args.num_ppo_epochs == 4 and args.lr == 2e-4
    with pytest.raises(NotImplementedError):
        main_rl.build(main_rl.parse_args(['--experiment_id', 'x']))


def test_main_saves_state_dicts(tmp_path):
    from stove_amd.rl import main_rl
    state = torch.get_rng_state()
    runner = main_rl.main(['--use-states', '--experiment_id', 'run', '--device', 'cpu', '--num-steps', '4', '--batch-size', '2', '--num-ppo-mb', '2',
                           '--num-ppo-epochs', '1', '--num-env-steps', '24', '--save-interval', '2', '--summary-dir', str(tmp_path / 's'),
                           '--model-dir', str(tmp_path / 'm')])
    torch.set_rng_state(state)
    assert runner.batch_counter == 3
    assert sorted(os.listdir(tmp_path / 'm' / 'run')) == ['model0.pt', 'model2.pt'] and os.path.exists(tmp_path / 's' / 'run' / 'args.json')
    sd = torch.load(tmp_path / 'm' / 'run' / 'model2.pt')
    assert set(sd) == set(runner.actor_critic.state_dict())


# ------------------------------------------------------------------------------------------------ 5. bookkeeping
def test_ppo_collect_refuses_host_visible_nonsense_and_sizes_its_image():
    from stove_amd import _lib, build, ops
    from stove_amd.rl.collect import param_floats
    build.build_library()
    fn = _lib.load().stove_ppo_collect
    for N, H, deep in ((3, 64, False), (6, 64, True), (1, 32, False), (3, 128, True), (6, 1, False), (2, 40, True)):
        assert ops.ppo_param_floats(N, H, deep) == param_floats(N, H, deep) == P.policy(N, H, deep).flat_params().numel()
    assert ops.ppo_param_floats(0, 64, 0) == 0 and ops.ppo_param_floats(7, 64, 0) == 0 and ops.ppo_param_floats(3, 129, 0) == 0
    # host-visible nonsense is refused before anything touches a device (this machine may have none): hipErrorInvalidValue == 1
    Pv = ctypes.c_void_p
    good = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(good)
    call = lambda x=addr, B=1, S=1, N=3, H=64, gran=5: fn(Pv(x), *([Pv(addr)] * 13), B, S, N, H, 0, gran, 0, 10.0, 1.0, 0.0, 0.3, 0.95, None)
    assert call(x=None) == 1 and call(B=-1) == 1 and call(S=-1) == 1 and call(N=0) == 1 and call(N=7) == 1 and call(H=0) == 1
    assert call(H=129) == 1 and call(gran=0) == 1
    assert call(B=0) == 0
    import importlib.util
    spec = importlib.util.spec_from_file_location('run_ppo_tool', os.path.join(ROOT, 'tools', 'run_ppo.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert callable(tool.main) and callable(ops.ppo_collect)


def test_ops_ppo_collect_refuses_host_tensors():
    from stove_amd import ops
    b = P.envs('b3_s5_n3_h64')
    cpu = [torch.from_numpy(np.array(a)) for a in (b.x, b.v, b.r, b.m)]
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_collect(*cpu, P.policy(3, 64, False).flat_params(), torch.from_numpy(np.array(P.table('b3_s5_n3_h64'))), 64, False, 5, 10.0)
