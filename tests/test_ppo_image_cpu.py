"""CPU-side checks (-m "not gpu") of the PPO arm on images: Task's frame buffer and Runner.reset(frame_buffer=True) held to the reference's
recorded buffers (tests/golden/g26_ppo_images.npz); the host forest ImageForest against this package's Policy in float64 and that
against the reference's recorded outputs; the parameter image; the text the kernel runs, stove_amd/csrc/ppo_image.h, compiled host-only
under sanitizers with contraction off (tests/abi/ppo_image_driver.cpp) and held to the specification compositionally; the full numpy
collection; the entry points.  (All fail before the feature: the names do not exist.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import control_harness
import ppo_image_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# draw_image against the reference: the bar tests/test_envs_cpu.py holds the environment fixture's frames to
FRAME_BAR = 1e-12


# ------------------------------------------------------------------------------------------------ 1. the frame buffer = the reference
@pytest.mark.parametrize('case', range(2))
def test_frame_buffer_reproduces_the_reference(case):
    """layout (res, res, 3F), the newest frame last, zero rows before the buffer fills; reset(frame_buffer=True) is env.reset(), the
    buffer zeroed and four steps with action 0; the states bit for bit"""
    from stove_amd.rl.runners import Runner
    G, pre, F = P.golden(), 'c%d_' % case, P.GOLDEN_SHAPES[case][0]
    task = P.golden_task(case)
    assert task.get_framebuffer_shape() == (32, 32, 3 * F) == G[pre + 'buf'].shape[1:]
    task.env.reset()
    task.frame_buffer[:] = 0.
    for k in range(4):
        buf, state, reward, done = task.step_frame_buffer(0)
        assert buf is task.frame_buffer and state.shape == (3, 4) and done is False
        assert np.abs(buf - G[pre + 'warm'][k]).max() <= FRAME_BAR, k
        assert not buf[:, :, :max(3 * (F - 1 - k), 0)].any()                      # (no frame has reached these rows yet)
    task = P.golden_task(case)
    runner = Runner.__new__(Runner)
    runner.env, runner.task = task.env, task
    task.frame_buffer[:] = 7.                                                     # (reset zeroes it)
    for k in range(4):
        buf, state, reward, done = runner.reset(frame_buffer=True) if k == 0 else task.step_frame_buffer(int(G[pre + 'buf_actions'][k - 1]))
        worst = np.abs(buf - G[pre + 'buf'][k]).max()
        assert worst <= FRAME_BAR, (k, worst)
        assert np.array_equal(task.env.x, G[pre + 'x'][k]) and np.array_equal(task.env.v, G[pre + 'v'][k]), k
        assert np.array_equal(state, np.concatenate([task.env.x, task.env.v], 1))
    # the default keeps what it did: (frame, state) after one step with action 0
    img, state = runner.reset()
    assert img.shape == (32, 32, 3) and state.shape == (3, 4)


def test_greyscale_buffer_weighs_the_channels():
    from stove_amd.envs import envs as E
    task = E.AvoidanceTask(E.BillardsEnv(n=3, granularity=2, seed=1), num_stacked=3, greyscale=True)
    assert task.get_framebuffer_shape() == (32, 32, 3)
    buf, _, _, _ = task.step_frame_buffer(2)
    img = task.env.draw_image()
    assert np.array_equal(buf[:, :, 2], img[:, :, 0] * 0.3 + img[:, :, 1] * 0.59 + img[:, :, 2] * 0.11) and not buf[:, :, :2].any()


# ------------------------------------------------------------------------------------------------ 2. the policy half
def _logsoftmax64(logits):
    l = logits.astype(np.float64)
    top = l.max(axis=1, keepdims=True)
    return l - top - np.log(np.exp(l - top).sum(axis=1, keepdims=True))


@pytest.mark.parametrize('case', range(2))
def test_forest_policy_half_against_float64_torch(case):
    """ImageForest (one serial float32 sum per output) on the fixture's buffers against this package's Policy in float64 with the fixture's
    state dict: value, normalised logits and the log-probabilities of the fixture's actions within 4 x the reference's own
    float32-to-float64 gap of that case (g26_reference_fp32_gap.json), the project's standing bar; Policy in float64 is the reference's,
    to 1e-12.  Measured (deviation / bar, cases 0 / 1): value 2.2e-8 / 5.3e-9 (0.75 / 0.25), logits 2.5e-8 / 1.1e-8 (0.03 / 0.01), logp
    8.6e-9 / 9.0e-9 (0.01 / 0.01); printed at every run."""
    from stove_amd.rl.collect import ImageForest
    G, pre = P.golden(), 'c%d_' % case
    F, H, deep = P.GOLDEN_SHAPES[case]
    gap = P.fp32_gap()['case%d' % case]
    assert gap['shape'] == [F, H, deep]
    windows = P.golden_windows(case)
    actions = G[pre + 'actions']
    p64 = P.golden_policy(case, torch.float64)
    obs64 = torch.from_numpy(G[pre + 'buf']).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        value, dist = p64.head(p64.base(obs64))
        ev, elp, ent = p64.evaluate_actions(obs64, torch.from_numpy(actions).reshape(4, 1))
    close = lambda got, want: np.abs(np.asarray(got) - want).max() <= 1e-12
    assert close(value.numpy(), G[pre + 'value64']) and close(dist.logits.numpy(), G[pre + 'logits64'])
    assert close(ev.numpy(), G[pre + 'eval_value64']) and close(elp.numpy(), G[pre + 'eval_logp64']) and close(ent.numpy(), G[pre + 'eval_entropy64'])
    # the float32 windows are the float64 buffers rounded once: the policy in float64 on them is the reference for the forest
    with torch.no_grad():
        value, dist = p64.head(p64.base(torch.from_numpy(windows.reshape(4, 3 * F, 32, 32)).double()))
    heads = ImageForest.from_policy(P.golden_policy(case)).forward(windows)
    logits = _logsoftmax64(heads[:, 1:])
    dv = np.abs(heads[:, 0].astype(np.float64) - value.numpy()[:, 0]).max()
    dl = np.abs(logits - dist.logits.numpy()).max()
    dp = np.abs(logits[np.arange(4), actions] - dist.logits.numpy()[np.arange(4), actions]).max()
    print(f'case {case}: value off by {dv:.3g} ({dv / (4 * gap["value"]):.2f} of the bar), logits by {dl:.3g} '
          f'({dl / (4 * gap["logits"]):.2f}), logp by {dp:.3g} ({dp / (4 * gap["eval_logp"]):.2f})')
    assert dv <= 4 * gap['value'] and dl <= 4 * gap['logits'] and dp <= 4 * gap['eval_logp']


# ------------------------------------------------------------------------------------------------ 3. the parameter image
def test_parameter_image_round_trips_and_sizes():
    from stove_amd import build, ops
    from stove_amd.rl.collect import image_param_floats
    from stove_amd.rl.rl_model import Policy
    build.build_library()
    for F, H, deep in ((4, 16, False), (2, 8, True), (1, 1, False), (4, 512, True), (3, 33, True)):
        p = P.policy(F, H, deep)
        assert p.image_kernel_shape() == (F, H, deep) and p.kernel_shape() is None
        image = p.flat_image_params()
        assert image.dtype == torch.float32 and image.numel() == image_param_floats(F, H, deep) == ops.ppo_image_param_floats(F, H, deep)
        q = Policy((32, 32, 3 * F), 9, hidden_size=H, stacked_frames=F, use_deep_layers=deep)
        q.load_flat_image_params(image)
        used = lambda k: deep or 'in_between' not in k
        assert all(torch.equal(ten, q.state_dict()[k]) for k, ten in p.state_dict().items() if used(k))
        assert torch.equal(q.flat_image_params(), image)
        with pytest.raises(ValueError, match='length of flat_image_params'):
            q.load_flat_image_params(image[:-1])
    # the layout, entry by entry
    p = P.policy(2, 8, True)
    image, sd = p.flat_image_params().numpy(), p.state_dict()
    assert image[(3 * 16 + 2 * 4 + 1) * 32 + 5] == sd['base.main.0.weight'][5, 3, 2, 1]
    at = 97 * 32
    assert image[96 * 32 + 7] == sd['base.main.0.bias'][7] and image[at + (11 * 9 + 1 * 3 + 2) * 32 + 30] == sd['base.main.2.weight'][30, 11, 1, 2]
    at += 289 * 32
    assert image[at + (5 * 49 + 3 * 7 + 6) * 8 + 4] == sd['head.main.weight'][4, 5 * 49 + 3 * 7 + 6]
    assert image[-10] == sd['head.values_head.bias'][0] and image[-1] == sd['head.actor_head.bias'][8]
    for F, H in ((0, 16), (5, 16), (4, 0), (4, 513)):
        assert ops.ppo_image_param_floats(F, H, 0) == 0 == image_param_floats(F, H, False)
    assert Policy((32, 32, 14), 9, hidden_size=16, use_grid=True).image_kernel_shape() is None
    assert Policy(12, 9, hidden_size=64, base='control').image_kernel_shape() is None
    assert Policy((32, 32, 12), 10, hidden_size=16).image_kernel_shape() is None
    with pytest.raises(ValueError, match='one-launch collection on images'):
        Policy(12, 9, hidden_size=64, base='control').flat_image_params()


# ------------------------------------------------------------------------------------------------ 4. the header on the CPU
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'ppo_image_driver')


def _drive(exe, tmp_path, name, image=None):
    B, S, N, F, H, deep, warm, gran = P.CASES[name]
    b = P.envs(name)
    outputs = [('frames', (B, F + S, 3, 32, 32), np.float32), ('actions', (B, S), np.int32), ('rewards', (B, S), np.float32),
               ('values', (B, S), np.float32), ('logp', (B, S), np.float32), ('next_value', (B,), np.float32), ('returns', (B, S), np.float32),
               ('status', (B,), np.int32), ('x', (B, N, 2), np.float64), ('v', (B, N, 2), np.float64), ('margin', (B,), np.float64)]
    image = P.policy(F, H, deep).flat_image_params().numpy() if image is None else image
    arrays = [np.asarray(a, dtype=np.float64) for a in (b.x, b.v, b.r, b.m)] + [image, P.table(name)]
    return control_harness.run_driver(exe, tmp_path, [B, S, N, F, H, deep, warm, b.granularity, b.drift, b.use_colors],
                                      [b.hw, b.t, b.friction, b.action_force, P.DISCOUNT], arrays, outputs)


@pytest.mark.parametrize('name', list(P.CASES))
def test_header_composes_from_the_specification(driver, tmp_path, name):
    """ppo_image.h's collect under the sanitizers (guards around every output row intact: the driver fails otherwise) against ImageForest
    on its own frames, the host batch under its own actions and _calculate_returns: see ppo_image_cases.assert_composes.  Then the full
    numpy collection, which renders its own frames (within one ulp of the driver's): the same actions, values within 4 x the gap."""
    out = _drive(driver, tmp_path, name)
    worst_logp, worst_frame, margin = P.assert_composes(out, name)
    assert np.allclose(out['margin'], P.host_collect(name)[3], rtol=0, atol=1e-9)
    host, x, v, host_margin = P.host_collect(name)
    assert (host_margin >= P.MIN_MARGIN).all() and not host['status'].any()           # these very cases, no draw left out
    assert np.array_equal(out['actions'], host['actions']) and np.array_equal(out['rewards'], host['rewards'])
    assert np.array_equal(out['x'], x) and np.array_equal(out['v'], v)
    gap = max(g['value'] for g in P.fp32_gap().values())
    dv = max(np.abs(out['values'] - host['values']).max(), np.abs(out['next_value'] - host['next_value']).max())
    print(f'{name}: smallest decision margin {margin:.3g}, logp within {worst_logp} ulp, frames within {worst_frame} ulp, values of the numpy '
          f'collection differ by {dv:.3g} ({dv / (4 * gap):.2f} of the bar)')
    assert dv <= 4 * gap


def test_a_nan_weight_stops_the_header_with_nothing_written(driver, tmp_path):
    name = 'b4_s3_n3_f3_h64'
    B, S, N, F, H, deep, warm, gran = P.CASES[name]
    image = P.policy(F, H, deep).flat_image_params().numpy().copy()
    image[7] = np.nan
    out = _drive(driver, tmp_path, name, image)
    assert out['status'].tolist() == [3] * B
    for k in ('frames', 'rewards', 'values', 'logp', 'next_value', 'returns'):
        assert np.isnan(out[k]).all(), k
    assert (out['actions'] == -77).all()
    b = P.envs(name)                                                                  # (the state stands as the warm-up left it)
    for _ in range(warm):
        b.step(np.zeros(B, dtype=np.int64), render=False)
    assert np.array_equal(out['x'], b.x) and np.array_equal(out['v'], b.v)
    # the numpy collection says the same
    from stove_amd.rl.collect import ImageForest
    b2 = P.envs(name)
    host = ImageForest(image, F, H, deep).collect(b2, P.table(name), P.DISCOUNT, warm)
    assert host['status'].tolist() == [3] * B and all(not host[k].any() for k in host if k != 'status')
    assert np.array_equal(b2.x, b.x) and np.array_equal(b2.v, b.v)


def test_validation_under_sanitizers(driver):
    """stove_ppo_collect_images' host-side argument check (csrc/validate.h: ppo_collect_images) through the driver: every documented bad
    argument returns hipErrorInvalidValue, empty calls are accepted, nothing is dereferenced; the image's length and ranges"""
    control_harness.run_modes(driver, ['validate'])


def test_case_shapes_cover_what_they_claim():
    shapes = list(P.CASES.values())
    assert {s[3] for s in shapes} == {1, 2, 3, 4} and {s[4] for s in shapes} >= {1, 16, 33, 64, 512} and {s[5] for s in shapes} == {False, True}
    assert any(s[6] > s[3] for s in shapes) and any(s[6] < s[3] for s in shapes) and {s[2] for s in shapes} >= {1, 2, 3, 6}
    for name in P.CASES:
        out, _, _, margin = P.host_collect(name)
        print(f'{name}: smallest decision margin {margin.min():.3g}')
        assert (margin >= P.MIN_MARGIN).all() and not out['status'].any()
        assert len({tuple(r) for r in out['actions']}) > 1                            # the draw matters


# ------------------------------------------------------------------------------------------------ 5. entry points
def test_entry_points_build_the_image_arm():
    from stove_amd.rl import main_rl
    from stove_amd.rl.rl_model import SimpleCNNBase
    args = main_rl.parse_args(['--use-images', '--experiment_id', 'x', '--device', 'cpu'])
    runner, policy = main_rl.build(args)
    assert isinstance(policy.base, SimpleCNNBase) and policy.image_kernel_shape() == (4, 512, False) and runner.actor_critic is policy
    assert runner.task.get_framebuffer_shape() == (32, 32, 12) and not runner.fused_serves_images()
    for other in ('--use-states', '--use-pretrained-model'):
        with pytest.raises(AssertionError):
            main_rl.parse_args(['--use-images', other])
    with pytest.raises(NotImplementedError, match='--use-images'):
        main_rl.build(main_rl.parse_args(['--experiment_id', 'x']))
    with pytest.raises(ValueError, match='--fused-update'):
        main_rl.build(main_rl.parse_args(['--use-images', '--fused-update', '--device', 'cpu']))
    grid = main_rl.build(main_rl.parse_args(['--use-images', '--use-grid', '--hidden-size', '8', '--device', 'cpu']))[1]
    assert grid.image_kernel_shape() is None and grid.base.main[0].in_channels == 14
    import model.rl.collect as mc
    import model.rl.runners as mu
    from stove_amd.rl import collect, runners
    assert mc.ImageForest is collect.ImageForest and mc.image_param_floats is collect.image_param_floats
    assert mu.PPORunner.run_batch is runners.PPORunner.run_batch and callable(mu.PPORunner.collect_images)


def _runner(B=2, S=3, H=8, device=None, greyscale=False, use_grid=False, F=4, **kw):
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    from stove_amd.rl.runners import PPORunner
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, num_stacked=F, greyscale=greyscale, action_force=.3)
    policy = Policy(task.get_framebuffer_shape(), 9, hidden_size=H, stacked_frames=F, use_grid=use_grid)
    agent = PPOAgent(policy, .1, 2, 2, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
    return PPORunner(env, task, None, device, agent, policy, num_steps=S, batch_size=B, discount=P.DISCOUNT, **kw)


def test_run_batch_trains_on_the_host():
    state = torch.get_rng_state()
    torch.manual_seed(1)
    runner = _runner()
    before = {k: v.clone() for k, v in runner.actor_critic.state_dict().items()}
    u = np.random.RandomState(3).random_sample((2, 3)).astype(np.float32)
    out = runner.run_batch(u=u)
    torch.set_rng_state(state)
    assert tuple(out['frames'].shape) == (2, 7, 3, 32, 32) and tuple(out['actions'].shape) == (2, 3) and not out['status'].any()
    assert len(out['losses']) == 3 and all(np.isfinite(float(l)) for l in out['losses'])
    after = runner.actor_critic.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before) and all(bool(torch.isfinite(v).all()) for v in after.values())
    assert runner.batch_counter == 1 and isinstance(runner._test_actorcritic_images(2, 2), float)
    # the first window is the reference's start: env.reset() and four steps with action 0, one environment after the other
    from stove_amd.envs import envs
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, num_stacked=4, action_force=.3)
    twin = _runner()
    twin.env, twin.task = env, task
    for b in range(2):
        buf = twin.reset(frame_buffer=True)[0]
        want = buf.transpose(2, 0, 1).reshape(4, 3, 32, 32)
        assert np.abs(out['frames'][b, :4].numpy() - want).max() <= 1e-7, b
    # the stacked observations: channel f * 3 + c, oldest frame first
    obs = runner.stacked(out['frames'], 4)
    assert tuple(obs.shape) == (2, 4, 12, 32, 32) and torch.equal(obs[1, 2, 7], out['frames'][1, 2 + 2, 1]) and torch.equal(obs[0, 0, 0], out['frames'][0, 0, 0])
    with pytest.raises(ValueError, match='fused=True'):
        runner.run_batch(fused=True)


@pytest.mark.parametrize('kw', [dict(greyscale=True), dict(use_grid=True), dict(F=2)])
def test_composed_loop_serves_what_the_launch_does_not(kw):
    state = torch.get_rng_state()
    torch.manual_seed(2)
    runner = _runner(**kw)
    out = runner.run_batch()
    torch.set_rng_state(state)
    F = kw.get('F', 4)
    assert tuple(out['frames'].shape) == (2, F + 3, 1 if kw.get('greyscale') else 3, 32, 32)
    assert all(np.isfinite(float(l)) for l in out['losses']) and not runner.fused_serves_images()


def test_main_runs_the_image_arm(tmp_path):
    from stove_amd.rl import main_rl
    state = torch.get_rng_state()
    runner = main_rl.main(['--use-images', '--experiment_id', 'img', '--device', 'cpu', '--num-steps', '2', '--batch-size', '2', '--num-ppo-mb', '2',
                           '--num-ppo-epochs', '1', '--num-env-steps', '8', '--hidden-size', '8', '--summary-dir', str(tmp_path / 's'),
                           '--model-dir', str(tmp_path / 'm')])
    torch.set_rng_state(state)
    assert runner.batch_counter == 2 and os.path.exists(tmp_path / 'm' / 'img' / 'model0.pt')


def test_collect_images_refuses_host_visible_nonsense():
    from stove_amd import _lib, build, ops
    build.build_library()
    fn = _lib.load().stove_ppo_collect_images
    Pv = ctypes.c_void_p
    good = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(good)
    call = lambda x=addr, B=1, S=1, N=3, F=4, H=64, warm=4, gran=5: fn(Pv(x), *([Pv(addr)] * 13), B, S, N, F, H, 0, warm, gran, 0, 1, 10.0, 1.0, 0.0,
                                                                      0.3, 0.95, None)
    assert call(x=None) == 1 and call(B=-1) == 1 and call(S=-1) == 1 and call(N=0) == 1 and call(N=7) == 1 and call(F=0) == 1 and call(F=5) == 1
    assert call(H=0) == 1 and call(H=513) == 1 and call(warm=0) == 1 and call(gran=0) == 1
    assert call(B=0) == 0
    b = P.envs('b5_s3_n3_f4_h16')
    cpu = [torch.from_numpy(np.array(a)) for a in (b.x, b.v, b.r, b.m)]
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_collect_images(*cpu, P.policy(4, 16, False).flat_image_params(), torch.from_numpy(np.array(P.table('b5_s3_n3_f4_h16'))), 4, 16,
                               False, 4, 2, 10.0)
    ret, params = control_harness.header_decl('stove_ppo_collect_images')
    assert ret == 'int' and len(params) == 30 and params[6] == 'float* frames' and params[-1] == 'void* stream'
