"""GPU tests of the model-based PPO arm's one-launch collection (stove_ppo_collect_model, csrc/ppo_model.hip; ops.ppo_collect_model;
PPORunner.run_pretrained_batch).  The check is compositional: every output is held bit for bit to a component that is pinned to
float64 elsewhere -- the policy half to the host forest's decide_model on the kernel's own states (tests/test_ppo_model_cpu.py holds
the header to it), the model half to stove_small_linear + stove_rollout_fwd + stove_reward_head_fwd on the kernel's own actions, the
returns to Runner._calculate_returns -- so no tolerance is invented; logp alone (exp, log) is held to one float32 ulp.  Every compared
draw has a host decision margin >= 1e-9 (asserted, none dropped).  (All fail before the feature: the entry point does not exist.)"""
import types

import numpy as np
import pytest
import torch

import ppo_cases as P
import ppo_model_cases as C
from control_harness import margins_intact

pytestmark = pytest.mark.gpu
DEV = C.DEV


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the policy half
@pytest.mark.parametrize('name', list(C.CASES))
def test_policy_half_equals_the_host_forest_on_the_kernels_states(name):
    from stove_amd.rl.collect import PolicyForest
    B, S, N, H, deep = C.CASES[name][:5]
    got = C.kernel_run(name)
    assert not got['status'].any()
    forest = PolicyForest.from_policy(C.policy(name))
    z, u = C.states_before(name, got), C.table(name)
    worst, smallest = 0, np.inf
    for t in range(S):
        obs, values, actions, logp, margin = forest.decide_model(z[:, t], C.HW, u[:, t])
        smallest = min(smallest, float(margin.min()))
        assert (margin >= C.MIN_MARGIN).all(), (name, t)               # every trajectory, none dropped
        assert np.array_equal(_bits(got['obs'][:, t]), _bits(obs)) and np.array_equal(_bits(got['values'][:, t]), _bits(values)), (name, t)
        assert np.array_equal(got['actions'][:, t], actions), (name, t)
        worst = max(worst, int(P.ulps32(got['logp'][:, t], logp).max()))
    last = forest.observe_model(z[:, S], C.HW)
    assert np.array_equal(_bits(got['obs'][:, S]), _bits(last))
    assert np.array_equal(_bits(got['next_value']), _bits(forest.forward(last)[:, 0]))
    print(f'{name}: smallest host decision margin {smallest:.3g}, logp within {worst} ulp')
    assert worst <= 1, worst


# ------------------------------------------------------------------------------------------------ 2. the model half
@pytest.mark.parametrize('name', list(C.CASES))
def test_model_half_equals_the_existing_rollout_on_the_kernels_actions(name):
    """extra rows from stove_small_linear on one-hot rows plus the appearance, stove_rollout_fwd with num = A = S, then
    stove_reward_head_fwd on its pred, minus 1.0f"""
    from stove_amd import ops
    B, S, N, H, deep, app_dim = C.CASES[name][:6]
    got = C.kernel_run(name)
    st = C.case_model(name)
    z0, app = C.start(name)
    with torch.no_grad():
        one_hot = torch.nn.functional.one_hot(torch.from_numpy(got['actions'].astype(np.int64)), 9).float().to(DEV)
        emb = st.dyn.embed_actions(one_hot).view(B, S, N, st.dyn.n_action_enc)
        extra = emb if app is None else torch.cat([emb, app.unsqueeze(1).expand(-1, S, -1, -1)], -1)
        image, sink = st.dyn.kernel_params(0)
        z_full, _, pred = ops.rollout(z0, extra.contiguous(), image, S, 2, st.dyn.use_elu, st.dyn.loop_consts(), want_pred=True, sink=sink)
        rewards = st.dyn.reward_from_pred(pred).reshape(B, S) - 1.0
    dz = float(np.abs(z_full.cpu().numpy().astype(np.float64) - got['z_pred']).max())
    dp = float(np.abs(pred.cpu().numpy().astype(np.float64) - got['pred']).max())
    dr = float(np.abs(rewards.cpu().numpy().astype(np.float64) - got['rewards']).max())
    print(f'{name}: largest differences z_pred {dz:.3g}, pred {dp:.3g}, rewards {dr:.3g}')
    assert np.array_equal(_bits(z_full.cpu().numpy()), _bits(got['z_pred']))
    assert np.array_equal(_bits(pred.cpu().numpy()), _bits(got['pred']))
    assert np.array_equal(_bits(rewards.cpu().numpy()), _bits(got['rewards']))


@pytest.mark.parametrize('name', ['b1_s1_n1_h32', 'b3_s5_n3_h64', 'b5_s6_n6_h128_deep'])
def test_rewards_equal_the_planning_kernels(name):
    """Bit for bit, the cl = 32 twin of tests/test_gpu_ppo_model_cl.py's test: the state before every step (b, t) in slot 0 of a pool
    of M = B S trees, one ops.plan_expand (stove_plan_expand: plan_finish_k<32>) with A = 9, L = 1 and the trajectory's appearance:
    r_first[m, actions[b, t]] - 1.0f is rewards[b, t], the child state of that action is z_pred[b, t]."""
    from stove_amd import ops
    B, S, N, H, deep, app_dim = C.CASES[name][:6]
    got = C.kernel_run(name)
    st = C.case_model(name)
    _, app = C.start(name)
    before = torch.from_numpy(C.states_before(name, got)[:, :S]).reshape(B * S, N, 18)
    M, A, cap = B * S, 9, 10
    pool = torch.full((M, cap, N, 18), float('nan'))
    pool[:, 0] = before
    pool = pool.to(DEV)
    emb_w, emb_b, gnn, rh = C.weights(st)
    i32 = lambda v: torch.full((M,), v, dtype=torch.int32, device=DEV)                     # noqa: E731
    acts = torch.from_numpy(np.random.RandomState(32 + N).randint(0, A, (M * A, 1)).astype(np.int32)).to(DEV)
    apps = None if app is None else app.repeat_interleave(S, 0).contiguous()
    q, r_first, r_roll = ops.plan_expand(pool, i32(0), i32(1), i32(1), apps, acts, emb_w, emb_b, gnn, rh, 2, 2, st.dyn.use_elu,
                                         st.dyn.loop_consts(), 0.95, want_rewards=True)
    torch.cuda.synchronize()
    chosen = torch.from_numpy(got['actions'].astype(np.int64)).reshape(M)
    rows = torch.arange(M)
    want = (r_first.cpu()[rows, chosen] - torch.tensor(1.0, dtype=torch.float32)).numpy().reshape(B, S)
    assert want.dtype == np.float32 and np.array_equal(_bits(want), _bits(got['rewards']))
    kids = pool.cpu()[rows, 1 + chosen].numpy().reshape(B, S, N, 18)
    assert np.array_equal(_bits(kids), _bits(got['z_pred']))


# ------------------------------------------------------------------------------------------------ 3. the returns
@pytest.mark.parametrize('name', list(C.CASES))
def test_returns_equal_the_runners(name):
    from stove_amd.rl.runners import Runner
    got = C.kernel_run(name)
    rewards = torch.from_numpy(np.array(got['rewards'])).unsqueeze(-1)
    want = Runner._calculate_returns(types.SimpleNamespace(discount=C.DISCOUNT), torch.from_numpy(np.array(got['next_value'])).unsqueeze(-1),
                                     rewards, torch.zeros_like(rewards))
    assert np.array_equal(_bits(want[:, :, 0].numpy()), _bits(got['returns']))


# ------------------------------------------------------------------------------------------------ 4. composed against fused
COMPOSED_MARGIN = 1e-4
RUN_CASE = 'b3_s5_n3_h64'
# the u table of the runner tests: collect.uniforms(3, 5, seed).  The first seed from 11 on whose smallest host decision margin on the
# fused run's observations is >= 1e-4 (asserted); seeds passed over: none.
RUN_TABLE_SEED = 11


def _runner(fused_update=False):
    """a runner on the reference's seeded policy of golden case 0 (N = 3, H = 64), main_rl's environment settings"""
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.runners import PPORunner
    B, S = C.CASES[RUN_CASE][:2]
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, action_force=.3)
    policy = P.golden_policy(0)
    agent = PPOAgent(policy, .1, 2, 3, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused=True if fused_update else None)
    return PPORunner(env, task, None, DEV, agent, policy, num_steps=S, batch_size=B, discount=P.DISCOUNT)


def _encoded(count=7):
    """`count` start states and appearances: the case's, repeated"""
    z0, app = C.start(RUN_CASE)
    rows = torch.arange(count) % z0.shape[0]
    return z0[rows].clone(), app[rows].clone()


def test_fused_and_composed_batches_agree():
    """The same start states (the same torch seed), the same table u: equal actions, rewards, obs and final states -- once the actions
    agree the model steps are the same launches' arithmetic.  Fair because the host forest's smallest decision margin on the fused run's
    observations is >= 1e-4 (asserted): torch's GEMM order moves a logit by about 4e-7 (the recorded float32 gap), and so a cumulative
    probability by about as much, more than two orders below.  values and logp differ by that GEMM order; the bar is the one of
    tests/test_gpu_ppo.py, 4 x the reference's recorded float32 gap of this policy."""
    from stove_amd.rl.collect import PolicyForest
    gap = P.fp32_gap()['case0']
    B, S = C.CASES[RUN_CASE][:2]
    u = C.uniforms(B, S, RUN_TABLE_SEED)
    st = C.case_model(RUN_CASE)
    encoded, apps = _encoded()
    state, np_state = torch.get_rng_state(), np.random.get_state()
    outs = {}
    for fused in (True, False):
        torch.manual_seed(2)
        np.random.seed(2)
        runner = _runner()
        assert runner.fused_serves_model(st)
        outs[fused] = {k: ten.cpu().numpy() for k, ten in runner.run_pretrained_batch(st, encoded, apps, fused=fused, u=u).items()
                       if isinstance(ten, torch.Tensor)}
    torch.set_rng_state(state)
    np.random.set_state(np_state)
    a, c = outs[True], outs[False]
    forest = PolicyForest.from_policy(P.golden_policy(0))
    margin = np.stack([forest.draw(forest.forward(a['obs'][:, t])[:, 1:], u[:, t])[2] for t in range(S)])
    print(f'smallest host decision margin on the fused run: {margin.min():.3g}')
    assert (margin >= COMPOSED_MARGIN).all()
    assert not a['status'].any() and not c['status'].any()
    assert np.array_equal(a['actions'], c['actions']) and np.array_equal(_bits(a['rewards']), _bits(c['rewards']))
    assert np.array_equal(_bits(a['obs']), _bits(c['obs'])) and np.array_equal(_bits(a['z_pred']), _bits(c['z_pred']))
    dv = max(np.abs(a['values'] - c['values']).max(), np.abs(a['next_value'] - c['next_value']).max())
    dl = np.abs(a['logp'] - c['logp']).max()
    print(f'fused against composed: values differ by {dv:.3g} (bar {4 * gap["value"]:.3g}), logp by {dl:.3g} (bar {4 * gap["eval_logp"]:.3g})')
    assert dv <= 4 * gap['value'] and dl <= 4 * gap['eval_logp']
    from stove_amd.rl.runners import PPORunner
    host = PPORunner(runner.env, runner.task, None, None, runner.agent, P.golden_policy(0), num_steps=S, batch_size=B)
    with pytest.raises(ValueError, match='fused=True'):
        host.collect_model(st, encoded[:B], apps[:B], fused=True)


# ------------------------------------------------------------------------------------------------ 5. edges and status
def test_empty_collections_are_accepted():
    from stove_amd import _lib, ops
    assert _lib.load().stove_ppo_collect_model(*([None] * 18), 0, 8, 3, 64, 0, 3, 2, 0, 0.3, 0.04, 0.04, 10.0, 0.95, None) == 0
    name = 'b3_s5_n3_h64'
    B, S, N, H, deep = C.CASES[name][:5]
    st = C.case_model(name)
    z0, app = C.start(name)
    emb_w, emb_b, gnn, rh = C.weights(st)
    image = C.policy(name).flat_params().to(DEV)
    call = lambda z, a, u: ops.ppo_collect_model(z, a, image, emb_w, emb_b, gnn, rh, u, H, deep, 2, st.dyn.use_elu, st.dyn.loop_consts(), C.HW)
    out = call(z0[:0].contiguous(), app[:0].contiguous(), torch.zeros(0, 8, device=DEV))
    assert tuple(out['obs'].shape) == (0, 9, 12) and tuple(out['status'].shape) == (0,)
    # S = 0: the observation, next_value and status only
    out = call(z0, app, torch.zeros(B, 0, device=DEV))
    got = C.kernel_run(name)
    assert out['status'].tolist() == [0] * B and tuple(out['returns'].shape) == (B, 0) and tuple(out['z_pred'].shape) == (B, 0, N, 18)
    assert np.array_equal(_bits(out['obs'].cpu().numpy()[:, 0]), _bits(got['obs'][:, 0]))
    assert np.array_equal(_bits(out['next_value'].cpu().numpy()), _bits(got['values'][:, 0]))


def test_a_nan_start_state_stops_its_trajectory_alone():
    """a NaN in the velocity of object 1 of trajectory 1's z0: status 3 at step 0 and nothing of it written; every other trajectory
    bit-equal to the clean run"""
    name = 'b5_s6_n6_h128_deep'
    clean = C.kernel_run(name)
    z0 = C.start(name)[0].clone()
    z0[1, 1, 4] = float('nan')
    out, buffers = C.collect(name, z0=z0)
    assert out['status'].tolist() == [0, 3, 0, 0, 0]
    for k, ten in out.items():
        part = ten.cpu()
        if k != 'status':
            assert bool(torch.isnan(part[1]).all()) if k in C.FLOATS else bool((part[1] == -77).all()), k
        rows = [0, 2, 3, 4]
        assert np.array_equal(_bits(part.numpy()[rows]), _bits(clean[k][rows])), k
    margins_intact(buffers)


def test_two_calls_agree_bit_for_bit():
    name = 'b3_s4_n5_h64_deep'
    first = C.kernel_run(name)
    out, buffers = C.collect(name)
    for k, ten in out.items():
        assert np.array_equal(_bits(ten.cpu().numpy()), _bits(first[k])), k
    margins_intact(buffers)


def test_captured_collection_replays_bit_for_bit():
    name = 'b3_s5_n3_h64'
    first = C.kernel_run(name)
    out, buffers = C.collect(name, graph=True)
    for k, ten in out.items():
        assert np.array_equal(_bits(ten.cpu().numpy()), _bits(first[k])), k
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 5b. the start states
def test_load_and_encode_batches_the_windows_red_first():
    """two recorded avoidance sequences of ten frames: 2 x (10 - 8) windows in one batched forward, channel-first or channel-last
    frames alike; every state finite, the object with the largest first appearance channel in front"""
    from stove_amd.envs import envs
    from stove_amd.rl.pretrained import load_and_encode
    st = C.case_model(RUN_CASE)
    data = envs.synth_sequences('avoidance', 2, 10, res=32)
    state = torch.get_rng_state()
    torch.manual_seed(4)
    z, apps = load_and_encode(data, st, DEV)
    torch.manual_seed(4)
    last = dict(data, X=np.transpose(data['X'], (0, 1, 3, 4, 2)))
    z2, apps2 = load_and_encode(last, st, DEV, chunk=3)
    torch.set_rng_state(state)
    assert tuple(z.shape) == (4, 3, 18) and tuple(apps.shape) == (4, 3, 3) and z.dtype == torch.float32 and z.is_cuda
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(apps).all())
    assert bool((apps[:, 0, 0] >= apps[:, 1:, 0].max(dim=1).values).all())
    assert tuple(z2.shape) == (4, 3, 18) and bool((apps2[:, 0, 0] >= apps2[:, 1:, 0].max(dim=1).values).all())
    with pytest.raises(ValueError, match='no window of 8'):
        load_and_encode(dict(data, X=data['X'][:, :8], action=data['action'][:, :8]), st, DEV)


# ------------------------------------------------------------------------------------------------ 6. training
def test_two_fused_batches_train_the_policy():
    state, np_state = torch.get_rng_state(), np.random.get_state()
    torch.manual_seed(3)
    np.random.seed(3)
    st = C.case_model(RUN_CASE)
    encoded, apps = _encoded()
    runner = _runner(fused_update=True)
    before = {k: v.detach().clone() for k, v in runner.actor_critic.state_dict().items()}
    first = runner.run_pretrained_batch(st, encoded, apps, fused=True)
    middle = {k: v.detach().clone() for k, v in runner.actor_critic.state_dict().items()}
    second = runner.run_pretrained_batch(st, encoded, apps, fused=True)
    np.random.set_state(np_state)
    torch.set_rng_state(state)
    after = runner.actor_critic.state_dict()
    assert runner.batch_counter == 2 and not first['status'].any() and not second['status'].any()
    assert any(not torch.equal(before[k], middle[k]) for k in before) and any(not torch.equal(middle[k], after[k]) for k in before)
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    for out in (first, second):
        assert all(np.isfinite(float(x)) for x in out['losses']) and np.isfinite(out['test_reward'])
