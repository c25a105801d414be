"""CPU tests of the image policy's PPO update on the device: the fixture the GPU suite is held to (this project's float64 torch update
reproduces the reference's record), the seeded cases' margins, the host-only driver under the sanitizers, and the host side of
ops.ppo_update_images, PPOAgent(fused_images=True), PPORunner and main_rl where no GPU is needed.  (They fail before the feature: the
symbol, the op, the keyword and update_windows do not exist.)"""
import numpy as np
import pytest
import torch

import control_harness
import ppo_image_cases as P
import ppo_image_update_cases as U
from ppo_update_cases import traced_update


@pytest.mark.parametrize('c', U.GOLDEN_CASES)
def test_float64_torch_update_reproduces_the_reference_record(c):
    """g27: PPOAgent.update in float64 under the recorded permutations -> the recorded parameters, losses and norms to 1e-10"""
    G, batch, shape = U.golden(), U.golden_batch(c), P.GOLDEN_SHAPES[c // 2]
    run = traced_update(U.policy_of(shape, U.golden_start(c), torch.float64), batch, torch.float64, perm=batch['perm'])
    after = U.golden_after(c)
    assert set(after) == set(U.used_keys(shape, run['sd']))
    for k, want in after.items():
        assert np.abs(run['sd'][k] - want).max() <= 1e-10, k
    assert np.abs(run['losses'] - G['c%d_losses' % c]).max() <= 1e-10 and np.abs(run['gnorm'] - G['c%d_gnorm' % c]).max() <= 1e-10
    info = U.golden_gaps()['case%d' % c]
    assert min(info['margins'].values()) >= U.MIN_MARGIN and info['shape'] == [shape[0], shape[1], bool(shape[2])]
    clipped = [g > batch['max_grad_norm'] for g in G['c%d_gnorm' % c]]
    assert all(clipped) if c % 2 else not any(clipped)
    assert G['s%d_obs' % (c // 2)].shape == (16, 3 * shape[0], 32, 32) and G['s%d_obs' % (c // 2)].dtype == np.float32


def test_the_seeded_cases_meet_their_margins():
    """no more than one seed in four is passed over, every decision of the float64 run has a margin >= 1e-5, the shapes are the
    ones the table names"""
    rows = {'b5_s3_n3_f4_h16': 15, 'b9_s2_n2_f2_h33_deep': 18, 'b2_s2_n6_f4_h512_deep': 4, 'b3_s4_n1_f1_h1': 12, 'b4_s3_n3_f3_h64': 12,
            'b10_s7_n3_f4_h16': 70}
    assert set(rows) == set(U.CASES) and set(P.CASES) <= set(U.CASES)
    skipped = 0
    for name, n in rows.items():
        c = U.case(name)
        E, M, max_grad_norm = U.CASES[name]
        assert c['batch']['obs'].shape == (n, 3 * c['shape'][0], 32, 32) and c['r64']['losses'].shape == (E * M, 3)
        assert min(c['r64']['margins'].values()) >= U.MIN_MARGIN, (name, c['r64']['margins'])
        assert np.array_equal(c['r64']['perm'], c['r32']['perm'])
        clipped = [g > max_grad_norm for g in c['r64']['gnorm']]
        assert all(clipped) if max_grad_norm < 1 else not any(clipped), (name, c['r64']['gnorm'])
        for q in U.STEP_QUANTITIES:
            assert c['floor'][q] > 0 and np.isfinite(c['gap'][q])
        skipped += c['skipped']
    assert skipped <= len(rows) // 4, skipped
    assert U.case('b10_s7_n3_f4_h16')['batch']['obs'].shape[0] // 2 == 35          # more than one 32-row tile, a multiple of neither 16 nor 32


def test_a_window_of_frames_is_a_row_of_the_stacked_observations():
    """the addressing rule of the kernels in numpy: the 3072 F floats at (r / S) env_stride + (r % S) 3072 of the flat frames equal row
    r of flat(stacked(frames)[:, :-1]); the dense layout is S = 1, env_stride = 3072 F"""
    from stove_amd.rl.runners import PPORunner
    rs = np.random.RandomState(0)
    for F in (1, 2, 3, 4):
        B, S = 3, 5
        frames = rs.random_sample((B, F + S, 3, 32, 32)).astype(np.float32)
        obs = PPORunner.stacked(torch.from_numpy(frames), F)[:, :-1].reshape(B * S, 3 * F, 32, 32).numpy()
        flat, dense = frames.reshape(-1), np.ascontiguousarray(obs).reshape(-1)
        for r in range(B * S):
            at = (r // S) * (F + S) * 3072 + (r % S) * 3072
            assert np.array_equal(flat[at:at + 3072 * F], obs[r].reshape(-1)), (F, r)
            assert np.array_equal(dense[r * 3072 * F:(r + 1) * 3072 * F], obs[r].reshape(-1))
        assert (B * S - 1) // S * (F + S) * 3072 + ((B * S - 1) % S) * 3072 + 3072 * F <= flat.size


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'ppo_image_update_driver')


def test_driver_passes_its_modes_under_the_sanitizers(driver):
    control_harness.run_modes(driver, ['validate', 'windows'])


def test_header_and_binding_declare_the_entry():
    from stove_amd import _lib
    ret, params = control_harness.header_decl('stove_ppo_update_images')
    assert ret == 'int' and len(params) == 33 and params[13] == 'float* grad' and params[15] == 'void* ws' and params[-1] == 'void* stream'
    ret, params = control_harness.header_decl('stove_ppo_update_images_ws_bytes')
    assert ret == 'size_t' and len(params) == 5
    assert _lib.ABI_VERSION == 7


def test_fused_images_is_accepted_for_the_image_policy_only():
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    make = lambda policy, **kw: PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, **kw)
    image = U.policy_of((4, 16, False), P.policy(4, 16, False).state_dict())
    agent = make(image, fused_images=True)
    assert agent.fused_images and not agent.fused
    for off in (None, False):
        plain = make(image, fused_images=off)
        assert not plain.fused_images and not plain.fused
    with pytest.raises(ValueError, match='fused=True'):
        make(image, fused=True)
    with pytest.raises(ValueError, match='fused_images=True'):
        make(Policy(12, 9, hidden_size=64, base='control'), fused_images=True)
    with pytest.raises(ValueError, match='fused_images=True'):
        make(Policy((32, 32, 12), 9, hidden_size=16, use_grid=True), fused_images=True)
    with pytest.raises(ValueError, match='update_windows'):
        make(image).update_windows(torch.zeros(2, 7, 3, 32, 32), 3, *[torch.zeros(6)] * 5)


def test_host_tensors_are_refused_and_the_policy_is_untouched():
    from stove_amd import ops
    from stove_amd.rl.agents import PPOAgent
    c = U.case('b5_s3_n3_f4_h16')
    b, shape = c['batch'], c['shape']
    policy = U.policy_of(shape, c['start'])
    agent = PPOAgent(policy, .1, 2, 3, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused_images=True)
    col = lambda key: torch.from_numpy(np.asarray(b[key], dtype=np.float32)).reshape(-1, 1)
    acts = torch.from_numpy(b['actions']).reshape(-1, 1)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match='GPU'):
        agent.update(torch.from_numpy(b['obs']), acts, col('returns'), col('values'), col('logp'), col('adv'))
    with pytest.raises(RuntimeError, match='GPU'):
        agent.update_windows(torch.from_numpy(c['frames']), c['S'], acts, col('returns'), col('values'), col('logp'), col('adv'))
    assert torch.equal(torch.get_rng_state(), state)                 # (no permutation was drawn)
    for k, t in policy.state_dict().items():
        assert torch.equal(t, c['start'][k]), k
    k = U.kernel_inputs(shape, c['start'], b)
    t = {key: torch.from_numpy(a) for key, a in k.items()}
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_update_images(t['image'], torch.zeros_like(t['image']), torch.zeros_like(t['image']), torch.zeros(1, dtype=torch.int32), t['obs'],
                              t['actions'], t['returns'], t['values'], t['logp'], t['adv'], t['perm'], 3, 4, 16, False, .1, .5, .01, 2e-4, 1e-5, 40.)


def test_entry_points_build_the_fused_image_arm():
    from stove_amd.rl import main_rl
    args = main_rl.parse_args(['--use-images', '--fused-update', '--experiment_id', 'x', '--device', 'cpu'])
    assert args.use_images and args.fused_update
    with pytest.raises(ValueError, match='--fused-update'):
        main_rl.build(args)
    runner, policy = main_rl.build(main_rl.parse_args(['--use-images', '--experiment_id', 'x', '--device', 'cpu', '--hidden-size', '8']))
    assert not runner.agent.fused_images and not runner.agent.fused
    with pytest.raises(ValueError, match='--fused-update'):
        main_rl.build(main_rl.parse_args(['--use-states', '--fused-update', '--device', 'cpu']))
    if torch.cuda.is_available():
        runner, policy = main_rl.build(main_rl.parse_args(['--use-images', '--fused-update', '--experiment_id', 'x', '--hidden-size', '8']))
        assert runner.agent.fused_images and not runner.agent.fused
        with pytest.raises(ValueError, match='--use-grid'):
            main_rl.build(main_rl.parse_args(['--use-images', '--fused-update', '--use-grid', '--hidden-size', '8']))
