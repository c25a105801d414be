"""CPU-side checks (-m "not gpu") of whole-sequence data synthesis: stove_amd/csrc/env_step.h and env_gravity.h -- the text the kernel
of csrc/env_sequences.hip runs -- compiled host-only under sanitizers with contraction off (tests/abi/env_sequences_driver.cpp) and
held to the numpy specification (stove_amd/envs/synth.py: BatchedSequences) bit for bit; the specification held to envs.py
(synth_sequences, itself pinned to the reference by g0_envs.npz); draw_starts against what synth_sequences draws;
stove_env_sequences' host-side argument check; the data-file tool and the public surface.  (All fail before the feature: the header,
the module and the symbol do not exist.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import control_harness
import env_sequence_cases as C
from stove_amd.envs import envs, synth

ULP32 = 2.0 ** -23
# test_specification_against_envs_py: the largest |y| deviation between the numpy specification and envs.py over all cases, measured
# on the CPU this was written on, was 7.11e-15 (cases grav3 and res50, twelve steps of 50 substeps; 8.88e-16 on avoid3, at most 2.3e-16
# elsewhere); the smallest branch margin that is not an exact tie was 1.142e-4 (case avoid3; 1.14e-4 below).  The bar is 100 x the
# former, 7.11e-13, and stays below 1e-3 x the latter.
MEASURED_DEVIATION, SMALLEST_MARGIN = 7.11e-15, 1.14e-4
BAR = min(100 * MEASURED_DEVIATION, 1e-3 * SMALLEST_MARGIN)
GRAVITY = [n for n in C.CASES if n.startswith('grav') or n == 'res50']


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'env_sequences_driver')


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _drive(exe, tmp_path, name):
    st, T = C.starts(name), C.CASES[name][1]
    s = st['settings']
    B, N, res = st['x0'].shape[0], s['n'], s['res']
    outputs = [('y', (B, T, N, 4), np.float64), ('collisions', (B, T), np.int32), ('in_bounds', (B,), np.int32), ('status', (B,), np.int32),
               ('frames', (B, T, 3, res, res), np.float32)]
    arrays = [st[k] for k in ('x0', 'v0', 'r', 'm')] + ([st['actions']] if st['actions'] is not None else [])
    return control_harness.run_driver(exe, tmp_path, [B, N, T, s['granularity'], s['drift'], st['actions'] is not None, s['gravity'], res,
                                                      s['use_colors']], [s['hw'], s['t'], s['friction'], s['action_force']], arrays, outputs)


# ------------------------------------------------------------------------------------------------ 1. headers = specification, bit for bit
@pytest.mark.parametrize('name', list(C.CASES))
def test_headers_equal_the_specification_bit_for_bit(driver, tmp_path, name):
    """env_step.h / env_gravity.h on the CPU (sanitizers, -ffp-contract=off) against BatchedSequences: y bit for bit, collisions and
    in_bounds equal, every frame to one float32 ulp (exp is a library call on either side)."""
    out, host = _drive(driver, tmp_path, name), C.host_run(name)
    assert not out['status'].any() and not host['status'].any()
    assert np.array_equal(_bits(out['y']), _bits(host['y']))
    assert np.array_equal(out['collisions'], host['collisions']) and np.array_equal(out['in_bounds'], host['in_bounds'])
    err = float(np.abs(out['frames'].astype(np.float64) - host['X'].astype(np.float64)).max())
    print(f'{name}: header frames against numpy frames {err:.3g}')
    assert err <= ULP32
    assert host['X'].max() == 1.0 and host['X'].min() == 0.0


def test_validation_and_status_two_under_sanitizers(driver):
    """stove_env_sequences' host-side argument check (csrc/validate.h: env_sequences) through the driver: every documented bad argument
    returns hipErrorInvalidValue, an empty batch is accepted, nothing is dereferenced; and status 2: an action index of 9, -1 or 2^30 at
    step 0, in the middle or at step T - 1 of sequence 1 of 3 gives status [0, 2, 0], sequence 1's rows keep a poison pattern and its
    neighbours equal a clean run."""
    control_harness.run_modes(driver, ['validate', 'status'])


def test_status_two_on_the_specification():
    st = dict(C.starts('avoid3'))
    T = C.CASES['avoid3'][1]
    clean = synth.BatchedSequences(st).run(T)
    for bad in (9, -1, 1 << 30):
        for at in (0, T // 2, T - 1):
            acts = st['actions'].copy()
            acts[1, at] = bad
            got = synth.BatchedSequences(dict(st, actions=acts)).run(T)
            assert got['status'].tolist() == [0, 2, 0, 0]
            assert not got['y'][1].any() and not got['X'][1].any() and got['in_bounds'][1] == 0
            for k in ('y', 'X', 'collisions', 'in_bounds'):
                assert np.array_equal(got[k][[0, 2, 3]], clean[k][[0, 2, 3]]), k


# ------------------------------------------------------------------------------------------------ 2. specification against envs.py
@pytest.mark.parametrize('name', ['bill3', 'avoid3', 'grav3'])
def test_recording_classes_are_envs_py(name):
    """the instrumented classes compute what envs.py computes, bit for bit, and for a preset that is synth_sequences itself"""
    rec, plain = C.envs_run(name), C.envs_run(name, recording=False)
    preset, T, acting, res, seeds = C.CASES[name]
    for k in ('X', 'y') + (('action', 'reward') if acting else ()):
        assert np.array_equal(rec[k], plain[k]), k
        for row, seed in enumerate(seeds):
            assert np.array_equal(envs.synth_sequences(preset, 1, T, seed0=seed, res=res)[k][0], plain[k][row]), (k, seed)
    assert isinstance(rec['envs'][0], envs.GravityEnv if name == 'grav3' else envs.BillardsEnv)


@pytest.mark.parametrize('name', list(C.CASES))
def test_specification_against_envs_py(name):
    """The same sequences through envs.py in synth_sequences' loop.  The two differ only where BLAS norms / dots and pow differ from
    the plain forms in the last bit, amplified by collisions and by the gravity chain.  Every branch margin of the envs.py side (walls,
    pair gaps, the force clip, the box bounds of every recorded coordinate) is an exact tie that any arithmetic reproduces or >= 1e-6
    -- no case and no step is excluded -- so both sides take the same branches: actions, rewards, in_bounds and the accepted mask are
    equal, X agrees to one float32 ulp and y within BAR (the header of this file)."""
    ref, host = C.envs_run(name), C.host_run(name)
    T = C.CASES[name][1]
    margins = np.array([m for m, tie in ref['margins'] if not tie])
    ties = [m for m, tie in ref['margins'] if tie]
    assert all(m == 0.0 for m in ties)
    assert margins.min() >= 1e-6, margins.min()
    assert margins.min() >= SMALLEST_MARGIN, margins.min()              # (the figure the bar was set from)
    dev = float(np.abs(host['y'] - ref['y']).max())
    xerr = float(np.abs(host['X'].astype(np.float64) - ref['X'].astype(np.float64)).max())
    print(f'{name}: smallest margin {margins.min():.4g}, {len(ties)} exact ties, y deviation {dev:.3g} (bar {BAR:.3g}), X {xerr:.3g}')
    assert np.array_equal(host['in_bounds'], ref['in_bounds'])
    n = host['y'].shape[2]
    assert np.array_equal(synth.accepted(host['in_bounds'], T, n), synth.accepted(ref['in_bounds'], T, n))
    if 'action' in ref:
        preset, _, acting, res, seeds = C.CASES[name]
        for row, seed in enumerate(seeds):
            got = synth.synth_sequences_batched(preset, 1, T, seed0=seed, with_actions=acting, res=res)
            assert np.array_equal(got['action'][0], ref['action'][row]) and np.array_equal(got['reward'][0], ref['reward'][row])
            assert got['reward'].shape == (1, T, 1) and got['action'].shape == (1, T, 9)
            assert np.array_equal(got['y'][0], host['y'][row]) and np.array_equal(got['X'][0], host['X'][row])
        assert np.array_equal(-host['collisions'][:, :, None].astype(np.float64), ref['reward'])
    else:
        assert not host['collisions'].any()
    assert xerr <= ULP32
    assert dev <= BAR


def test_the_cases_exercise_every_branch():
    """wall bounces, free and controlled collisions (counted on the envs.py side), friction that slows the balls down, a drifting case
    without collisions; grav_clip: the clip engages, and every | |f| - 1 | is >= 1e-6; grav_out: at least one sequence is rejected and
    one accepted, every counted coordinate >= 1e-6 away from 0 and hw"""
    hits = {n: tuple(sum(getattr(e, k) for e in C.envs_run(n)['envs']) for k in ('wall_hits', 'free_hits', 'controlled_hits'))
            for n in ('bill3', 'bill6', 'avoid3', 'bill1', 'drift3', 'fric3')}
    print(hits)
    assert all(h >= 1 for h in hits['bill3'][:2]) and all(h >= 1 for h in hits['bill6'][:2]) and hits['bill3'][2] == 0
    assert all(h >= 1 for h in hits['avoid3']) and C.host_run('avoid3')['collisions'].any()
    assert hits['bill1'][0] >= 1 and hits['drift3'][0] >= 1 and hits['drift3'][1:] == (0, 0)
    speed = np.sqrt((C.host_run('fric3')['y'][:, :, :, 2:] ** 2).sum(-1))
    assert speed[:, -1].mean() < 0.7 * speed[:, 0].mean()               # (1 - 0.05 / 10) ^ (10 x 11) = 0.58 for a ball nothing hits
    clip = C.envs_run('grav_clip')
    assert clip['clipped'] >= 1 and min(clip['clip_margins']) >= 1e-6
    assert C.envs_run('grav3')['clipped'] == 0
    out = C.envs_run('grav_out')
    mask = synth.accepted(out['in_bounds'], C.CASES['grav_out'][1], 3)
    assert mask.tolist() == [True, False, True, False] and min(out['bound_margins']) >= 1e-6
    assert np.array_equal(synth.accepted(C.host_run('grav_out')['in_bounds'], 12, 3), mask)
    # the rule itself, on the integer: T = 100 steps of 3 balls tolerate no more than 5 of 600 coordinates outside
    assert synth.accepted(np.array([600, 595, 594, 0]), 100, 3).tolist() == [True, True, False, False]


# ------------------------------------------------------------------------------------------------ 3. draw_starts
@pytest.mark.parametrize('preset', ['billiards', 'avoidance', 'gravity'])
def test_draw_starts_draws_what_synth_sequences_draws(preset):
    T, B = 6, 3
    st = synth.draw_starts(preset, B, T, seed0=5)
    acting = preset == 'avoidance'
    assert st['x0'].shape == st['v0'].shape == (B, 3, 2) and st['r'].shape == st['m'].shape == (B, 3)
    for i in range(B):
        env = envs.make_env(preset, 5 + i)
        assert np.array_equal(st['x0'][i], env.x) and np.array_equal(st['v0'][i], env.v) and np.array_equal(st['r'][i], np.ravel(env.r))
        assert st['m'][i].tolist() == ([10000.0] if acting else [float(np.ravel(env.m)[0])]) + [float(np.ravel(env.m)[1])] * 2
    s = st['settings']
    cfg = envs.ENV_PRESETS[preset]
    assert (s['n'], s['res'], s['granularity'], s['hw'], s['gravity']) == (3, 32, cfg['granularity'], float(cfg['hw']), preset == 'gravity')
    assert synth.draw_starts(preset, B, T, seed0=5, res=50)['settings']['res'] == 50
    shifted = synth.draw_starts(preset, B, T, seed0=6)
    for k in ('x0', 'v0', 'r', 'm') + (('actions',) if acting else ()):
        assert np.array_equal(shifted[k][:-1], st[k][1:]), k
    if not acting:
        assert st['actions'] is None
        return
    assert st['actions'].dtype == np.int32 and st['actions'].shape == (B, T)
    ref = envs.synth_sequences(preset, B, T, seed0=5)['action']
    for i in range(B):
        rows = np.roll(ref[i], 1, axis=0)                  # row t of the file holds step t + 1's action, row T - 1 step 0's
        assert (rows.sum(1) == 1).all() and np.array_equal(rows.argmax(1), st['actions'][i])
    with pytest.raises(ValueError, match='no actions'):
        synth.draw_starts('gravity', 1, T, with_actions=True)


# ------------------------------------------------------------------------------------------------ 4. tool and surface
def test_make_data_writes_files_the_dataset_reads(tmp_path):
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.load_data import StoveDataset, load
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'make_data.py'), 'gravity', '--runs', '3', '2', '--res', '32', '--run-len', '12',
                        '--out', str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count('total amount of bad runs: 0') == 2
    ref = synth.synth_sequences_batched('gravity', 5, 12)
    for kind, rows in (('train', slice(0, 3)), ('test', slice(3, 5))):
        data = load(str(tmp_path / f'gravity_{kind}.pkl'))
        assert data['X'].shape == (rows.stop - rows.start, 12, 32, 32, 3) and data['X'].dtype == np.float64
        assert np.array_equal(data['y'], ref['y'][rows]) and np.array_equal(np.transpose(data['X'], (0, 1, 4, 2, 3)), ref['X'][rows])
        assert (data['coord_lim'], data['hw'], data['n'], data['granularity'], data['init_v_factor'], data['res']) == (30, 30, 3, 50, 0.55, 32)
        cfg = StoveConfig()
        cfg.num_episodes, cfg.num_visible, cfg.num_rollout, cfg.frame_step = 1000, 4, 4, 1
        ds = StoveDataset(cfg, data=data)
        assert ds.data_info['num_obj'] == 3 and ds.data_info['coord_lim'] == 30 and not ds.rl and len(ds) == (rows.stop - rows.start) * 5
        assert ds[0]['present_images'].shape == (4, 3, 32, 32)


def test_avoidance_file_and_the_acceptance_order(tmp_path):
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.load_data import StoveDataset, load
    paths = synth.generate_data('avoidance', str(tmp_path), runs=(2, 1), t_len=10, chunk=2)
    data = load(paths[0])
    ref = envs.synth_sequences('avoidance', 2, 10)
    assert set(data) >= {'X', 'y', 'action', 'reward', 'done', 'action_space', 'action_force', 'type', 'coord_lim', 'res', 'hw', 'n', 'r'}
    assert np.array_equal(data['action'], ref['action']) and np.array_equal(data['reward'], ref['reward']) and not data['done'].any()
    assert (data['action_space'], data['action_force'], data['type'], data['coord_lim']) == (9, 0.6, 'AvoidanceTask', 10)
    assert np.array_equal(load(paths[1])['action'], envs.synth_sequences('avoidance', 1, 10, seed0=2)['action'])
    cfg = StoveConfig()
    cfg.num_episodes, cfg.num_visible, cfg.num_rollout, cfg.frame_step = 1000, 4, 4, 1
    ds = StoveDataset(cfg, data=data)
    assert ds.rl and ds.data_info['action_space'] == 9 and ds[0]['present_actions'].shape == (4, 9)
    # the first accepted candidates in seed order: grav_out's consecutive seeds 4 .. 7 are accepted, rejected, accepted, rejected
    preset = C.CASES['grav_out'][0]
    for chunk in (1, 3, 256):
        part, seeds, bad = synth.generate_runs(preset, 2, 12, seed0=4, chunk=chunk)
        assert seeds.tolist() == [4, 6] and bad == 1
        assert np.array_equal(part['y'], C.host_run('grav_out')['y'][[0, 2]])
    part, seeds, bad = synth.generate_runs(preset, 3, 12, seed0=4, chunk=4, filtered=False)
    assert seeds.tolist() == [4, 5, 6] and bad == 0
    with pytest.raises(RuntimeError, match='accepted'):
        synth.generate_runs(preset, 3, 12, seed0=4, chunk=2, max_tries=4)
    with pytest.raises(ValueError, match='generate_data writes'):
        synth.generate_data('pong', str(tmp_path))


def test_env_sequences_refuses_host_visible_nonsense_and_public_surface():
    from stove_amd import _lib, build, ops
    build.build_library()
    assert _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.stove_abi_version() == 7
    fn = lib.stove_env_sequences
    assert callable(ops.env_sequences)
    ret, params = control_harness.header_decl('stove_env_sequences')
    assert ret == 'int' and len(params) == len(fn.argtypes) == 23
    # host-visible nonsense is refused before anything touches a device (this machine has none): hipErrorInvalidValue == 1
    P = ctypes.c_void_p
    good = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(good)

    def call(x0=addr, actions=None, y=addr, B=1, N=3, T=12, gran=10, res=32, kind=0):
        return fn(P(x0), P(addr), P(addr), P(addr), actions, P(y), None, P(addr), P(addr), P(addr), B, N, T, gran, res, 1, 0, kind,
                  10.0, 1.0, 0.0, 0.6, None)
    assert call(x0=None) == 1 and call(y=None) == 1 and call(B=-1) == 1 and call(N=0) == 1 and call(N=7) == 1 and call(T=0) == 1
    assert call(gran=0) == 1 and call(res=0) == 1 and call(kind=2) == 1 and call(kind=-1) == 1 and call(kind=1, actions=P(addr)) == 1
    assert call(B=0) == 0 and call(B=0, kind=1) == 0
    import torch
    st = C.starts('bill3')
    cpu = [torch.from_numpy(np.array(st[k])) for k in ('x0', 'v0', 'r', 'm')]
    with pytest.raises(RuntimeError, match='GPU'):
        ops.env_sequences(*cpu, None, 12, 10, 32, 10.0)
    # the public surface
    import model.envs.envs as menvs
    from stove_amd.envs.batched import BatchedAvoidance
    for name in ('BatchedSequences', 'accepted', 'draw_starts', 'generate_data', 'generate_runs', 'synth_sequences_batched'):
        assert getattr(menvs, name) is getattr(synth, name), name
    assert menvs.BatchedAvoidance is BatchedAvoidance and envs.SIMULATOR_VERSION == 2
    with pytest.raises(ValueError, match='stays on the host'):
        BatchedAvoidance.from_tasks([envs.AvoidanceTask(envs.GravityEnv(seed=0))])
    out = synth.synth_sequences_batched('billiards', 2, 3, device='cpu')
    assert isinstance(out['X'], np.ndarray) and set(out) == {'X', 'y', 'in_bounds'}
