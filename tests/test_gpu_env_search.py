"""GPU tests of the search on the true environment (stove_env_search, csrc/env_search.hip; ops.env_search; plan_on_envs and
play(policy='env_mcts') on a device BatchedAvoidance): the kernel against the host forest EnvForest -- the same text, csrc/env_search.h,
is held to that forest and to the reference's recorded trees on the CPU by tests/test_env_search_cpu.py -- bit for bit in every tree
array, used, status and action.  The only library call is log, in the exploration term: every compared tree has a host decision gap
>= 1e-9 (asserted, no tree dropped), seven orders of magnitude above a last-bit difference in it, so both sides take the same
decisions and everything else is the same IEEE operations.  (All fail before the feature: the module and the symbol do not exist.)"""
import numpy as np
import pytest
import torch

import env_search_cases as E
from control_harness import guarded, margins_intact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MIN_GAP = 1e-9


def _device_search(b, draws, forest, R, graph=False):
    """ops.env_search on guarded device copies of the host batch `b`, the table and the arrays of `forest` -> (arrays, action, the state
    tensors, every guarded buffer)"""
    from stove_amd import ops
    buffers, state = {}, {}
    for k in ('x', 'v', 'r', 'm'):
        state[k], buffers[k] = guarded(torch.from_numpy(np.array(getattr(b, k))), float('nan'))
    table, buffers['draws'] = guarded(torch.from_numpy(np.array(draws, dtype=np.int32)), -77)
    arrays = {}
    for k, ten in forest.to_device('cpu').items():
        arrays[k], buffers[k] = guarded(ten, float('nan') if ten.dtype.is_floating_point else -77)
    call = lambda: ops.env_search(state['x'], state['v'], state['r'], state['m'], table, arrays, forest.D, b.granularity, b.hw, b.t, b.friction,
                                  b.action_force, b.drift, replicas=R)
    if not graph:
        action = call()
    else:
        fresh = {k: ten.clone() for k, ten in arrays.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        for k, ten in arrays.items():
            ten.copy_(fresh[k])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            action = call()
        for k, ten in arrays.items():
            ten.copy_(fresh[k])                             # (a capture runs nothing)
        g.replay()
    torch.cuda.synchronize()
    return arrays, action, state, buffers


def _assert_equal(arrays, action, forest, want_action, rows=None):
    """every tree array, used, status bit for bit (Qsa as bits) -- of all trees, or of `rows`"""
    rows = slice(None) if rows is None else rows
    for k in E.ARRAYS + ('used',):
        got, want = arrays[k].cpu().numpy()[rows], getattr(forest, k)[rows]
        if k == 'Qsa':
            assert np.array_equal(got.view(np.int64), np.ascontiguousarray(want).view(np.int64)), k
        else:
            assert np.array_equal(got, want), k
    assert np.array_equal(arrays['status'].cpu().numpy()[rows], forest.status[rows])
    if want_action is not None:
        assert action.dtype == torch.int32 and np.array_equal(action.cpu().numpy(), want_action)


# ------------------------------------------------------------------------------------------------ 1. kernel = host forest
@pytest.mark.parametrize('name', list(E.CASES))
def test_kernel_equals_the_host_forest_bit_for_bit(name):
    from stove_amd.mcts.mcts_env import EnvForest
    T, R, _, D, runs = E.shape(name)
    b, draws = E.start(name)
    host, want = E.host_search(name)
    print(f'{name}: T={T} R={R} smallest host decision gap {host.gap.min():.3g}')
    assert (host.gap >= MIN_GAP).all() and not host.status.any()                 # every tree, none dropped
    arrays, action, state, buffers = _device_search(b, draws, EnvForest(T, E.A, D, runs), R)
    _assert_equal(arrays, action, host, want)
    gaps = arrays['min_gap'].cpu().numpy()
    assert np.array_equal(np.isinf(gaps), np.isinf(host.gap)) and np.allclose(gaps[np.isfinite(gaps)], host.gap[np.isfinite(gaps)], rtol=0, atol=1e-12)
    for k in ('x', 'v', 'r', 'm'):                                               # the environment state is bit for bit untouched
        assert np.array_equal(state[k].cpu().numpy().view(np.int64), np.ascontiguousarray(getattr(b, k)).view(np.int64)), k
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 2. the reference's recorded trees
@pytest.mark.parametrize('case', range(4))
def test_kernel_reproduces_the_reference_trees(case):
    """the golden case on three trees of two environments (R = 1): every key's Nsa, Ns equal and Qsa bit for bit, the chosen action"""
    from stove_amd.mcts.mcts_env import EnvForest
    G = E.golden()[case]
    assert float(G['min_gap']) >= MIN_GAP
    D, runs = int(G['depth']), int(G['runs'])
    b = E.golden_envs(G, copies=3)
    draws = np.broadcast_to(G['draws'], (3, runs, D))
    f = EnvForest(3, E.A, D, runs)
    arrays, action, _, buffers = _device_search(b, draws, f, 1)
    f.from_device(arrays)
    assert not f.status.any() and action.tolist() == [int(G['action'])] * 3
    for t in range(3):
        E.assert_golden_tree(f, t, G)
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 3. frozen trees
@pytest.mark.parametrize('bad', [9, -1, 1 << 30])
def test_status_two_freezes_the_tree_and_spares_its_wave(bad):
    """a draw outside [0, 9) in column 0 of iteration 5 of tree 2 of 't65_n3_d10' (one wave and a lane): that tree is the clean tree after
    5 iterations with status 2, every other tree of the wave as in the clean run"""
    from stove_amd.mcts.mcts_env import EnvForest
    name = 't65_n3_d10'
    T, R, _, D, runs = E.shape(name)
    b, draws = E.start(name)
    host, _ = E.host_search(name)
    table = np.array(draws)
    table[2, 5, 0] = bad
    arrays, action, _, buffers = _device_search(b, table, EnvForest(T, E.A, D, runs), R)
    others = np.array([t for t in range(T) if t != 2])
    _assert_equal(arrays, None, host, None, rows=others)
    frozen = EnvForest(T, E.A, D, runs)
    want = frozen.search(b, table, R)
    assert frozen.status.tolist() == [2 if t == 2 else 0 for t in range(T)] and int(frozen.Ns[2, 0]) == 5
    _assert_equal(arrays, action, frozen, want)
    margins_intact(buffers)


def test_status_one_freezes_a_tree_out_of_slots():
    """'t4_n3_d10_runs12' with room for 5 expansions: every tree stops at its sixth expansion with status 1, as the host forest does"""
    from stove_amd.mcts.mcts_env import EnvForest
    name = 't4_n3_d10_runs12'
    T, R, _, D, runs = E.shape(name)
    b, draws = E.start(name)
    short, dev = EnvForest(T, E.A, D, 5), EnvForest(T, E.A, D, 5)
    want = short.search(b, draws, R)
    assert short.status.tolist() == [1] * T and (short.used == 1 + 5 * E.A).all()
    arrays, action, _, buffers = _device_search(b, draws, dev, R)
    _assert_equal(arrays, action, short, want)
    margins_intact(buffers)


def test_status_one_spares_the_wave_mates_of_a_full_tree():
    """'t4_n3_d3' uses 55, 55, 64 and 46 slots; with cap = 55 tree 2 alone stops at its seventh expansion with status 1, frozen as the
    host forest's, while trees 0, 1 and 3 of its wave are bit for bit those of the clean run"""
    from stove_amd.mcts.mcts_env import EnvForest
    name = 't4_n3_d3'
    T, R, _, D, runs = E.shape(name)
    b, draws = E.start(name)
    clean, clean_action = E.host_search(name)
    assert clean.used.tolist() == [55, 55, 64, 46]
    short = EnvForest(T, E.A, D, 6)
    want = short.search(b, draws, R)
    assert short.cap == 55 and short.status.tolist() == [0, 0, 1, 0] and int(short.used[2]) == 55 and int(short.Ns[2, 0]) < runs
    arrays, action, _, buffers = _device_search(b, draws, EnvForest(T, E.A, D, 6), R)
    _assert_equal(arrays, action, short, want)
    for k in E.ARRAYS + ('used',):                          # the neighbours against the CLEAN run (its slots from 55 on were never used)
        got, ref = arrays[k].cpu().numpy()[[0, 1, 3]], getattr(clean, k)[[0, 1, 3]]
        ref = ref[:, :55] if ref.ndim == 2 else ref
        assert np.array_equal(got.view(np.int64) if k == 'Qsa' else got, np.ascontiguousarray(ref).view(np.int64) if k == 'Qsa' else ref), k
        if ref.ndim == 2:
            rest = getattr(clean, k)[[0, 1, 3], 55:]
            assert (rest == (-1 if k in ('first', 'parent') else 0)).all(), k
    assert action.cpu().numpy()[[0, 1, 3]].tolist() == clean_action[[0, 1, 3]].tolist()
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 4. empty calls
def test_empty_searches_are_accepted():
    from stove_amd import _lib, ops
    from stove_amd.mcts.mcts_env import EnvForest
    b, _ = E.start('t4_n3_d3')
    f = EnvForest(4, E.A, 3, 0)
    arrays, action, _, buffers = _device_search(b, np.zeros((4, 0, 3), dtype=np.int32), f, 1)
    assert action.tolist() == [0] * 4 and arrays['used'].tolist() == [1] * 4 and arrays['status'].tolist() == [0] * 4
    assert bool((arrays['first'] == -1).all())
    margins_intact(buffers)
    assert _lib.load().stove_env_search(*([None] * 15), 0, 1, 3, 3, 12, 109, 5, 0, 10.0, 1.0, 0.0, 0.6, None) == 0
    e = torch.zeros(0, 3, 2, dtype=torch.float64, device=DEV)
    s = torch.zeros(0, 3, dtype=torch.float64, device=DEV)
    none = {k: torch.zeros((0, 10) if k in E.ARRAYS else (0,), dtype=torch.float64 if k in ('Qsa', 'min_gap') else torch.int32, device=DEV)
            for k in E.ARRAYS + ('used', 'status', 'min_gap')}
    out = ops.env_search(e, e, s, s, torch.zeros(0, 12, 3, dtype=torch.int32, device=DEV), none, 3, 5, 10.0)
    assert tuple(out.shape) == (0,)


# ------------------------------------------------------------------------------------------------ 5. graph capture
def test_captured_search_replays_bit_for_bit():
    from stove_amd.mcts.mcts_env import EnvForest
    name = 't130_r2_n3_d10'
    T, R, _, D, runs = E.shape(name)
    b, draws = E.start(name)
    host, want = E.host_search(name)
    arrays, action, _, buffers = _device_search(b, draws, EnvForest(T, E.A, D, runs), R, graph=True)
    _assert_equal(arrays, action, host, want)
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 6. the episode
def test_play_on_the_device_equals_the_host_episode():
    """no frame enters the decision, and x, v are bit for bit equal on both sides: the two episodes agree action for action"""
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.mcts.play import play
    seeds = (0, 1, 4, 8)
    np.random.seed(11)
    host = play(None, BatchedAvoidance(seeds), run_len=3, mcts_steps=12, max_rollout_depth=4, policy='env_mcts', replicas=2)
    np.random.seed(11)
    dev = play(None, BatchedAvoidance(seeds, device=DEV), run_len=3, mcts_steps=12, max_rollout_depth=4, policy='env_mcts', replicas=2)
    assert host['actions'].shape == (3, 4) and np.array_equal(host['actions'], dev['actions'])
    assert np.array_equal(host['rewards'], dev['rewards'])
    assert np.array_equal(host['states'].view(np.int64), dev['states'].view(np.int64))


def test_ops_env_search_checks_the_arrays_before_it_reads_them():
    """a missing or non-tensor entry of `arrays` is refused like every other argument, not with a KeyError / AttributeError"""
    from stove_amd import ops
    from stove_amd.mcts.mcts_env import EnvForest
    b, draws = E.start('t4_n3_d3')
    state = [torch.from_numpy(np.array(getattr(b, k))).to(DEV) for k in ('x', 'v', 'r', 'm')]
    table = torch.from_numpy(np.array(draws)).to(DEV)
    good = EnvForest(4, E.A, 3, 12).to_device(DEV)
    for broken in ({k: v for k, v in good.items() if k != 'first'}, dict(good, first=None), dict(good, first=good['first'].cpu().numpy()), None):
        with pytest.raises(RuntimeError, match='first must be'):
            ops.env_search(*state, table, broken, 3, 5, 10.0)
    with pytest.raises(ValueError, match='Qsa is'):
        ops.env_search(*state, table, dict(good, Qsa=good['Qsa'][:, :5].contiguous()), 3, 5, 10.0)
