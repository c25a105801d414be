"""GPU tests of whole-sequence data synthesis (stove_env_sequences, csrc/env_sequences.hip; ops.env_sequences;
synth_sequences_batched on a device): the kernel against the numpy specification BatchedSequences -- the same text, csrc/env_step.h and
csrc/env_gravity.h, is held to it on the CPU by tests/test_env_sequences_cpu.py -- bit for bit in y, equal in collisions and in_bounds,
EVERY frame to one float32 ulp (2^-23: exp is a library call on either side, everything else is the same IEEE operations before one
rounding).  Painting from the state one round early or late moves a ball by tenths of a unit, so the frame check at every step is what
catches a hand-off error between the stepping wave and the painting waves; the T = 1, 2, 3 cases localise it.  The sequences are those
of tests/env_sequence_cases.py."""
import numpy as np
import pytest
import torch

import env_sequence_cases as C
from control_harness import guarded, margins_intact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP32 = 2.0 ** -23
POISON_F, POISON_I = -7.5, -7


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))


def _launch(starts, T, render=True, actions='own'):
    """one ops.env_sequences call on guarded device copies, the outputs poisoned beforehand -> (host copies of the outputs, buffers)"""
    from stove_amd import ops
    s = starts['settings']
    B, N, res = starts['x0'].shape[0], s['n'], s['res']
    t, buffers = {}, {}
    for k in ('x0', 'v0', 'r', 'm'):
        t[k], buffers[k] = guarded(torch.from_numpy(np.array(starts[k])), float('nan'))
    acts = starts['actions'] if isinstance(actions, str) else actions
    if acts is not None:
        t['actions'], buffers['actions'] = guarded(torch.from_numpy(np.array(acts, dtype=np.int32)), -77)
    out = {}
    out['y'], buffers['y'] = guarded(torch.full((B, T, N, 4), POISON_F, dtype=torch.float64), float('nan'))
    if render:
        out['frames'], buffers['frames'] = guarded(torch.full((B, T, 3, res, res), POISON_F), float('nan'))
    for k, shape in (('collisions', (B, T)), ('in_bounds', (B,)), ('status', (B,))):
        out[k], buffers[k] = guarded(torch.full(shape, POISON_I, dtype=torch.int32), -77)
    got = ops.env_sequences(t['x0'], t['v0'], t['r'], t['m'], t.get('actions'), T, s['granularity'], res, s['hw'], s['t'], s['friction'],
                            s['action_force'], use_colors=s['use_colors'], drift=s['drift'], gravity=s['gravity'], render=render, out=out)
    torch.cuda.synchronize()
    margins_intact(buffers)
    for k in ('x0', 'v0', 'r', 'm'):                       # the starts are read only
        assert _same_bits(t[k].cpu().numpy(), starts[k]), k
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}


def _check(got, host, frames=True):
    assert not got['status'].any()
    assert _same_bits(got['y'], host['y'])
    assert np.array_equal(got['collisions'], host['collisions']) and np.array_equal(got['in_bounds'], host['in_bounds'])
    if frames:
        err = np.abs(got['frames'].astype(np.float64) - host['X'].astype(np.float64)).max(axis=(2, 3, 4))          # per (sequence, step)
        print('largest frame error per step', err.max(0))
        assert float(err.max()) <= ULP32


# ------------------------------------------------------------------------------------------------ 1. kernel = specification, every case
@pytest.mark.parametrize('name', list(C.CASES))
def test_kernel_equals_the_specification(name):
    got = _launch(C.starts(name), C.CASES[name][1])
    _check(got, C.host_run(name))


# ------------------------------------------------------------------------------------------------ 2. frames = NULL
@pytest.mark.parametrize('name', ['bill3', 'avoid3', 'grav3', 'bill3_T1', 'grav3_T2'])
def test_without_frames_the_states_are_the_same(name):
    got = _launch(C.starts(name), C.CASES[name][1], render=False)
    assert got['frames'] is None
    _check(got, C.host_run(name), frames=False)          # (an unwritten row would still hold the poison pattern)


# ------------------------------------------------------------------------------------------------ 3. status 2
@pytest.mark.parametrize('bad', [9, -1, 1 << 30])
def test_a_bad_action_index_refuses_the_whole_sequence(bad):
    st, T = C.starts('avoid3'), C.CASES['avoid3'][1]
    three = {k: (v[:3] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    clean = _launch(three, T)
    for at in (0, T // 2, T - 1):
        acts = three['actions'].copy()
        acts[1, at] = bad
        got = _launch(three, T, actions=acts)
        assert got['status'].tolist() == [0, 2, 0]
        assert (got['y'][1] == POISON_F).all() and (got['frames'][1] == POISON_F).all()
        assert (got['collisions'][1] == POISON_I).all() and got['in_bounds'][1] == POISON_I
        for k in ('y', 'frames', 'collisions', 'in_bounds'):
            assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]), k
    _check({k: (v[[0, 2]] if v is not None else None) for k, v in clean.items()},
           {k: v[[0, 2]] for k, v in C.host_run('avoid3').items()})


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize('name', ['bill6', 'res50'])
def test_two_calls_give_identical_bytes(name):
    a = _launch(C.starts(name), C.CASES[name][1])
    b = _launch(C.starts(name), C.CASES[name][1])
    for k in ('y', 'frames', 'collisions', 'in_bounds', 'status'):
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_synth_sequences_batched_on_the_device():
    from stove_amd.envs import synth
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.load_data import StoveDataset
    got = synth.synth_sequences_batched('billiards', 8, 8, device=DEV)
    want = synth.synth_sequences_batched('billiards', 8, 8)
    assert set(got) == set(want) == {'X', 'y', 'in_bounds'}
    assert all(got[k].is_cuda for k in ('X', 'y', 'in_bounds'))
    host = {k: v.cpu().numpy() for k, v in got.items()}
    assert _same_bits(host['y'], want['y']) and np.array_equal(host['in_bounds'], want['in_bounds'])
    assert host['X'].dtype == np.float32 and host['X'].shape == (8, 8, 3, 32, 32)
    assert float(np.abs(host['X'].astype(np.float64) - want['X'].astype(np.float64)).max()) <= ULP32
    cfg = StoveConfig()
    cfg.num_episodes, cfg.num_visible, cfg.num_rollout, cfg.frame_step = 1000, 4, 4, 1
    ds = StoveDataset(cfg, data=host)
    assert len(ds) == 8 and ds.data_info['num_obj'] == 3 and ds[0]['present_images'].shape == (4, 3, 32, 32)
    acting = synth.synth_sequences_batched('avoidance', 4, 6, device=DEV)
    ref = synth.synth_sequences_batched('avoidance', 4, 6)
    assert np.array_equal(acting['action'], ref['action']) and np.array_equal(acting['reward'], ref['reward'])
    assert _same_bits(acting['y'].cpu().numpy(), ref['y'])
