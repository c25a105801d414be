"""CPU-side checks (-m "not gpu") of the model-based PPO arm: the text the kernel runs between two steps of the model,
stove_amd/csrc/ppo_policy.h (observe_model, forward, draw), compiled host-only under sanitizers with contraction off
(tests/abi/ppo_model_driver.cpp) and held to PolicyForest.decide_model bit for bit; the observation against torch's float32 arithmetic
on the reference's expression; load_and_encode's reordering; the argument checks that need no GPU; main_rl's wiring; the C ABI
addition.  (All fail before the feature: the header function, the methods and the entry point do not exist.)"""
import numpy as np
import pytest
import torch

import control_harness
import ppo_cases as P

HW = 10.0


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'ppo_model_driver')


def _states(K, N, seed):
    """K model states: positions, velocities and latents uniform in [-1.2, 1.2] (past the [-1, 1] the model puts out), scales 0.1"""
    rs = np.random.RandomState(seed)
    z = rs.uniform(-1.2, 1.2, (K, N, 18)).astype(np.float32)
    z[:, :, :2] = 0.1
    return z


# ------------------------------------------------------------------------------------------------ 1. the header = the host forest
@pytest.mark.parametrize('N', [1, 3, 6])
@pytest.mark.parametrize('H,deep', [(32, False), (40, False), (128, True)])
def test_header_equals_decide_model_bit_for_bit(driver, tmp_path, N, H, deep):
    """obs, values and actions bit for bit, logp to one float32 ulp (exp and log are library calls on either side); every draw's host
    margin is >= 1e-9 (asserted, none dropped)"""
    from stove_amd.rl.collect import PolicyForest, uniforms
    K = 64
    policy = P.policy(N, H, deep)
    z, u = _states(K, N, 300 + N), uniforms(K, 1, 400 + N + H)[:, 0]
    forest = PolicyForest.from_policy(policy)
    obs, values, actions, logp, margin = forest.decide_model(z, HW, u)
    assert (margin >= P.MIN_MARGIN).all() and len(set(actions.tolist())) > 1               # (the draw matters)
    got = control_harness.run_driver(driver, tmp_path, [K, N, H, int(deep)], np.asarray([HW], dtype=np.float32),
                                     [z, policy.flat_params().numpy(), u],
                                     [('obs', (K, 4 * N), np.float32), ('values', (K,), np.float32), ('actions', (K,), np.int32),
                                      ('logp', (K,), np.float32), ('margin', (K,), np.float64)])
    assert np.array_equal(got['obs'].view(np.int32), obs.view(np.int32)) and np.array_equal(got['values'].view(np.int32), values.view(np.int32))
    assert np.array_equal(got['actions'], actions)
    assert int(P.ulps32(got['logp'], logp).max()) <= 1
    assert np.allclose(got['margin'], margin, rtol=1e-6, atol=1e-12)


def test_decide_model_checks_its_arguments():
    from stove_amd.rl.collect import PolicyForest
    forest = PolicyForest.from_policy(P.policy(3, 64, False))
    z = _states(4, 3, 1)
    with pytest.raises(ValueError, match='the policy reads'):
        forest.decide_model(z[:, :2], HW, np.zeros(4, np.float32))
    with pytest.raises(ValueError, match='float32 vector of 4 uniforms'):
        forest.decide_model(z, HW, np.zeros(4))


# ------------------------------------------------------------------------------------------------ 2. the observation = torch's float32
def test_observe_model_equals_torch_float32():
    """(z + 1) / 2 * hw and z / 2 * hw as the reference writes them (runners.py:241-243), on 4096 random z in [-1.2, 1.2] and an hw
    that is no float32 (rounded once, as torch rounds the scalar)"""
    from stove_amd.rl.collect import PolicyForest
    z = _states(256, 4, 77)
    assert z[:, :, 2:6].size == 4096
    for hw in (10.0, 9.7):
        t = torch.from_numpy(z)[:, :, 2:6].clone()
        t[:, :, :2] = ((t[:, :, :2] + 1) / 2) * hw
        t[:, :, 2:] = t[:, :, 2:] / 2 * hw
        got = PolicyForest.observe_model(z, hw)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), t.reshape(256, -1).numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------ 3. load_and_encode's reordering
def test_red_first_moves_the_first_largest_channel_to_the_front():
    from stove_amd.rl.pretrained import red_first
    import model.rl.pretrained as mp
    assert mp.red_first is red_first and mp.load_and_encode.__module__ == 'stove_amd.rl.pretrained'
    apps = torch.tensor([[[.1, .9, .9], [.8, .0, .0], [.3, .5, .5]],          # object 1 is red
                         [[.7, .2, .2], [.7, .9, .9], [.1, .1, .1]],          # a tie between 0 and 1: argmax takes the first
                         [[.2, .0, .0], [.4, .0, .0], [.4, .1, .1]],          # a tie between 1 and 2
                         [[.0, .0, .0], [.0, .0, .0], [.5, .0, .0]]])         # the last object
    states = torch.arange(4 * 3 * 18, dtype=torch.float32).reshape(4, 3, 18)
    want = [[1, 0, 2], [0, 1, 2], [1, 0, 2], [2, 0, 1]]
    z, a = red_first(states, apps)
    for k, order in enumerate(want):
        assert torch.equal(z[k], states[k][order]) and torch.equal(a[k], apps[k][order]), k
    # the reference's own lines on the same table (main_rl.py:148-155)
    red = torch.argmax(apps[:, :, 0], dim=1).numpy()
    assert [[i, *sorted(set([0, 1, 2]) - set([i]))] for i in red] == want


# ------------------------------------------------------------------------------------------------ 4. argument checks that need no GPU
def test_ops_ppo_collect_model_checks_its_arguments_on_the_host():
    from stove_amd import ops
    z0 = torch.zeros(3, 3, 18)
    rest = (None, torch.zeros(8554), torch.zeros(12, 9), torch.zeros(12), torch.zeros(10), torch.zeros(10), torch.zeros(3, 5), 64, False, 2, False,
            (0.3, 0.04, 0.04), HW)
    with pytest.raises(ValueError, match=r'z0 must be a \(B, N, 18\) tensor'):
        ops.ppo_collect_model(z0[:, :, :17], *rest)
    with pytest.raises(ValueError, match=r'z0 must be a \(B, N, 18\) tensor'):
        ops.ppo_collect_model(z0.numpy(), *rest)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_collect_model(z0, *rest)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.ppo_collect_model(z0.requires_grad_(True), *rest)


# ------------------------------------------------------------------------------------------------ 5. main_rl
def test_main_rl_builds_the_model_based_arm():
    from stove_amd.rl import main_rl
    args = main_rl.parse_args(['--use-pretrained-model', '--experiment_id', 'x', '--checkpoint', 'run_dir', '--data', 'seq.pkl', '--device', 'cpu'])
    assert args.use_pretrained_model and args.checkpoint == 'run_dir' and args.data == 'seq.pkl' and not args.use_states
    runner, policy = main_rl.build(args)
    assert policy.kernel_shape() == (3, 64, False) and callable(runner.run_pretrained_batch)
    with pytest.raises(ValueError, match='--checkpoint DIR'):
        main_rl.build(main_rl.parse_args(['--use-pretrained-model', '--experiment_id', 'x', '--device', 'cpu']))
    for other in (['--experiment_id', 'x'], ['--use-pretrained-model', '--task', 'maxdist', '--checkpoint', 'a', '--data', 'b']):
        with pytest.raises(NotImplementedError):
            main_rl.build(main_rl.parse_args(other))
    none = main_rl.parse_args(['--use-states', '--experiment_id', 'x'])
    assert none.checkpoint is None and none.data is None


def test_the_host_runner_composes_and_refuses_fused():
    """fused_serves_model needs a device; the composed loop's observation is the forest's to the bit"""
    from stove_amd.rl import main_rl
    from stove_amd.rl.collect import PolicyForest
    runner, policy = main_rl.build(main_rl.parse_args(['--use-states', '--experiment_id', 'x', '--device', 'cpu']))
    z = torch.from_numpy(_states(5, 3, 9))
    got = runner._observe_model(z).numpy()
    assert np.array_equal(got.view(np.int32), PolicyForest.observe_model(z.numpy(), runner.env.hw).view(np.int32))


# ------------------------------------------------------------------------------------------------ 6. the C ABI
def test_driver_modes(driver):
    control_harness.run_modes(driver, ['validate'])


def test_the_entry_point_is_declared_and_bound():
    from stove_amd import _lib
    ret, params = control_harness.header_decl('stove_ppo_collect_model')
    assert ret == 'int' and len(params) == 32 and params[0] == 'const float* z0' and params[-1] == 'void* stream'
    assert [p.split()[-1].lstrip('*') for p in params[18:31]] == ['B', 'S', 'N', 'H', 'deep', 'app_dim', 'lim_enc', 'elu', 'pos_var', 'vel_std',
                                                                  'lat_std', 'hw', 'discount']
    assert _lib.ABI_VERSION == 7

    class Recorder:
        def __getattr__(self, name):
            fn = type('Fn', (), {})()
            setattr(self, name, fn)
            return fn
    rec = Recorder()
    _lib._declare(rec)
    assert len(rec.stove_ppo_collect_model.argtypes) == 32
