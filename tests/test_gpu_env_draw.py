"""GPU tests of the counter-based start stream (stove_env_draw_starts, csrc/env_draw.hip; ops.env_draw_starts;
synth_sequences_batched(starts='counter') on a device): the kernel against the numpy specification synth.draw_starts_counter -- the
same text, csrc/env_draw.h, is held to it on the CPU by tests/test_env_draw_cpu.py -- bit for bit on x0, v0, actions, tries and status.
Everything up to the uniform double is integer arithmetic and everything after it an uncontracted IEEE + - * / sqrt, so there is no
tolerance anywhere but on the frames of the end-to-end test, which keep env_sequences' one float32 ulp.  The cases are those of
tests/env_draw_cases.py: the four presets, N = 1 and 6, a sequence without a start, gravity's last attempt, and six-ball starts found in
the first round of 64 attempts, in the second and after dozens of rounds."""
import numpy as np
import pytest
import torch

import env_draw_cases as C
from control_harness import guarded, margins_intact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP32 = 2.0 ** -23
POISON_F, POISON_I = -7.5, -7
INVALID = 1          # hipErrorInvalidValue


def _buffers(want, B, T):
    """guarded device copies of the radii and poisoned, guarded outputs of a call on B sequences of T steps"""
    N = want['settings']['n']
    buffers = {}
    r, buffers['r'] = guarded(torch.from_numpy(np.array(want['r']).reshape(B, N)), float('nan'))
    out = {}
    for k in ('x0', 'v0'):
        out[k], buffers[k] = guarded(torch.full((B, N, 2), POISON_F, dtype=torch.float64), float('nan'))
    if want['actions'] is not None:
        out['actions'], buffers['actions'] = guarded(torch.full((B, T), POISON_I, dtype=torch.int32), -77)
    for k in ('tries', 'status'):
        out[k], buffers[k] = guarded(torch.full((B,), POISON_I, dtype=torch.int32), -77)
    return r, out, buffers


def _call(name, want, r, out, T):
    from stove_amd import ops
    _, _, _, seed0, max_tries, _ = C.CASES[name]
    s = want['settings']
    return ops.env_draw_starts(r, T, seed0, s['hw'], gravity=s['gravity'], v_factor=C.v_factor(name), max_tries=max_tries, out=out)


def _launch(name, B=None, T=None):
    """one ops.env_draw_starts call on the case (at another B or T if given) -> (host copies of the outputs, the specification's)"""
    want = C.spec_at(name, B, T)
    B, T = want['x0'].shape[0], (C.CASES[name][2] if T is None else T)
    r, out, buffers = _buffers(want, B, T)
    got = _call(name, want, r, out, T)
    torch.cuda.synchronize()
    margins_intact(buffers)
    assert np.array_equal(r.cpu().numpy(), want['r'])          # the radii are read only
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}, want


# ------------------------------------------------------------------------------------------------ 1. kernel = specification, bit for bit
@pytest.mark.parametrize('name', list(C.CASES))
def test_kernel_equals_the_specification_bit_for_bit(name):
    got, want = _launch(name)
    print(name, 'tries', got['tries'].tolist(), 'status', got['status'].tolist())
    C.assert_same_bits(got, want, name)          # (an unwritten element would still hold the poison pattern)


@pytest.mark.parametrize('name', ['avoidance', 'multi_second_round', 'gravity'])
@pytest.mark.parametrize('B', [1, 3, 4, 9])
def test_partly_filled_and_several_workgroups(name, B):
    """four sequences per workgroup: B = 1, 3 leave waves idle, 4 fills one, 5 (every case above) and 9 need a partly filled second
    and third"""
    got, want = _launch(name, B=B)
    C.assert_same_bits(got, want, (name, B))


@pytest.mark.parametrize('T', [0, 1, 63, 64, 65])
def test_action_rows_across_the_chunks_of_64_steps(T):
    got, want = _launch('avoidance', T=T)
    assert got['actions'].shape == (5, T)
    C.assert_same_bits(got, want, T)
    got, want = _launch('six_acting', B=3, T=T)
    C.assert_same_bits(got, want, ('six_acting', T))


def test_an_empty_batch_is_a_valid_call():
    from stove_amd import _lib, ops
    r = torch.zeros(0, 3, dtype=torch.float64, device=DEV)
    got = ops.env_draw_starts(r, 12, 7, 10.0, with_actions=True)
    torch.cuda.synchronize()
    assert got['x0'].shape == (0, 3, 2) and got['actions'].shape == (0, 12) and got['tries'].shape == (0,)
    assert _lib.load().stove_env_draw_starts(None, None, None, None, None, None, 7, 0, 0, 3, 12, 0, 64, 10.0, 0.0, None) == 0


# ------------------------------------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize('preset', ['billiards', 'multibilliards', 'gravity', 'avoidance'])
def test_synth_sequences_batched_draws_and_simulates_on_the_device(preset):
    from stove_amd.envs import synth
    got = synth.synth_sequences_batched(preset, 5, 12, starts='counter', device=DEV)
    want = synth.synth_sequences_batched(preset, 5, 12, starts='counter', device=None)
    assert set(got) == set(want)
    assert all(got[k].is_cuda for k in ('X', 'y', 'in_bounds'))
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    assert np.array_equal(host['y'].view(np.int64), want['y'].view(np.int64))
    err = float(np.abs(host['X'].astype(np.float64) - want['X'].astype(np.float64)).max())
    print(preset, 'frames against the specification', err)
    assert host['X'].dtype == np.float32 and err <= ULP32
    assert np.array_equal(host['in_bounds'], want['in_bounds'])
    if preset == 'avoidance':
        assert np.array_equal(host['action'], want['action']) and np.array_equal(host['reward'], want['reward'])


# ------------------------------------------------------------------------------------------------ 3. the refusals
def test_documented_refusals_launch_nothing():
    from stove_amd import _lib
    from stove_amd._lib import ptr
    lib = _lib.load()
    want = C.spec_at('avoidance')
    r, out, buffers = _buffers(want, 5, 12)
    good = dict(r=ptr(r), x0=ptr(out['x0']), v0=ptr(out['v0']), actions=ptr(out['actions']), tries=ptr(out['tries']), status=ptr(out['status']),
                B=5, N=3, T=12, kind=0, max_tries=64)

    def call(**change):
        a = dict(good, **change)
        return lib.stove_env_draw_starts(a['r'], a['x0'], a['v0'], a['actions'], a['tries'], a['status'], 7, 0, a['B'], a['N'], a['T'], a['kind'],
                                         a['max_tries'], 10.0, 0.0, None)
    for change in (dict(r=None), dict(x0=None), dict(v0=None), dict(tries=None), dict(status=None), dict(B=-1), dict(N=0), dict(N=7),
                   dict(T=-1), dict(max_tries=0), dict(max_tries=-3), dict(kind=2), dict(kind=-1)):
        assert call(**change) == INVALID, change
    torch.cuda.synchronize()
    margins_intact(buffers)
    for k in ('x0', 'v0'):
        assert bool((out[k] == POISON_F).all()), k
    for k in ('actions', 'tries', 'status'):
        assert bool((out[k] == POISON_I).all()), k
    assert call() == 0          # (the same arguments unchanged are accepted)
    torch.cuda.synchronize()
    assert bool((out['status'] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. determinism and capture
@pytest.mark.parametrize('name', ['avoidance', 'multi_many_rounds'])
def test_two_calls_and_a_replayed_capture_give_identical_bytes(name):
    a, _ = _launch(name)
    b, want = _launch(name)
    for k in C.OUTPUTS:
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k
    B, T = C.CASES[name][1], C.CASES[name][2]
    r, out, buffers = _buffers(want, B, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(name, want, r, out, T)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(name, want, r, out, T)
    for k, t in out.items():
        if t is not None:
            t.fill_(POISON_F if t.dtype == torch.float64 else POISON_I)          # (a capture runs nothing)
    graph.replay()
    torch.cuda.synchronize()
    margins_intact(buffers)
    for k in C.OUTPUTS:
        if a[k] is not None:
            assert out[k].cpu().numpy().tobytes() == a[k].tobytes(), k
