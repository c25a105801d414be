"""CPU-side checks (-m "not gpu") of the device-resident tree search: the tree arithmetic of stove_amd/csrc/plan_tree.h -- the text the
kernels of csrc/plan_tree.hip run -- compiled host-only under sanitizers with contraction off (tests/abi/plan_tree_driver.cpp) and held
to the reference's recording (tests/golden/g21_mcts_tree.npz) and to the host Forest bit for bit; a tree that runs out of slots;
stove_plan_search's host-side argument check; the C ABI addition's workspace query.  (All fail before the feature: the
header, the symbols and the device_trees switch do not exist.)"""
import functools
import inspect

import numpy as np
import pytest
import torch

import control_harness
from helpers import load_golden

GOLD = load_golden('g21_mcts_tree')
A, ITERS, M = int(GOLD['actions']), int(GOLD['iters']), 3
INT_ARRAYS = ('first', 'parent', 'depth', 'Ns', 'Nsa')


def _key(row):
    return 'r' + ''.join(str(int(d)) for d in row if d >= 0)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'plan_tree_driver')


def _forest(D, used0=None, cap=0):
    from stove_amd.mcts.mcts_stove import Forest
    f = Forest(M, A, D, cap=cap)
    if used0 is not None:
        f.used = np.asarray(used0, dtype=np.int64).copy()
    return f


@functools.lru_cache(maxsize=None)
def _host_run(D, iters=ITERS, used0=None):
    """The forest of test_vectorised_forest_replays_the_reference (recording, other rewards, recording) searched on the host with q
    cast to float32 and widened, as the device hands it over -> (forest, q (iters, M, A) float32, leaf (iters, M), child (iters, M), used after
    every iteration (iters, M)).  Shared, never modified."""
    from stove_amd.mcts.mcts_stove import discounted_values
    rs, rr = GOLD[f'rs_d{D}'][..., 0, 0], GOLD[f'rr_d{D}'][..., 0]
    other = np.random.RandomState(5).rand(ITERS, A).astype(np.float32)
    f = _forest(D, used0)
    qs, leaves, childs, useds = [], [], [], []
    for i in range(iters):
        leaf = f.select()
        child = f.child_slots(leaf)
        len_s = f.depth[np.arange(M), leaf] + 1
        q = discounted_values(np.stack([rs[i], other[i], rs[i]]), np.stack([rr[i], rr[i][::-1], rr[i]]), len_s, D).astype(np.float32)
        f.backpropagate(leaf, child, q.astype(np.float64))
        qs.append(q)
        leaves.append(leaf)
        childs.append(child)
        useds.append(f.used.copy())
    return f, np.stack(qs), np.stack(leaves), np.stack(childs), np.stack(useds)


def _drive(exe, tmp_path, D, cap, q, used0=None):
    R = q.shape[0]
    used0 = np.ones(M, dtype=np.int32) if used0 is None else np.asarray(used0, dtype=np.int32)
    outputs = [('sel', (R, M), np.int32), ('child', (R, M), np.int32), ('status', (M,), np.int32), ('used', (M,), np.int32)] + \
        [(k, (M, cap), np.int32) for k in INT_ARRAYS] + [('action', (M,), np.int32), ('Qsa', (M, cap), np.float64), ('min_gap', (M,), np.float64)]
    return control_harness.run_driver(exe, tmp_path, [M, A, D, cap, R], used0, [np.asarray(q, dtype=np.float32)], outputs)


def _same_tree(out, f, m, cap=None):
    cap = f.cap if cap is None else cap
    for k in INT_ARRAYS:
        assert np.array_equal(out[k][m, :cap], getattr(f, k)[m, :cap]), (k, m)
    assert out['used'][m] == f.used[m], m
    assert np.array_equal(out['Qsa'][m, :cap].view(np.int64), f.Qsa[m, :cap].view(np.int64)), m              # bit for bit


@pytest.mark.parametrize('D', [3, 10])
def test_header_replays_the_recording_and_the_host_forest(driver, tmp_path, D):
    """plan_tree.h on the CPU against the reference's recording (the selected key of trees 0 and 2 at every iteration) and against
    Forest on the same float32 q: integer arrays and used equal, Qsa bit for bit, min_gap within 1e-12 (one log per candidate, each
    within a few ulp of values below 1e2)."""
    f, q, leaves, childs, _ = _host_run(D)
    out = _drive(driver, tmp_path, D, f.cap, q)
    assert not out['status'].any()
    for i in range(ITERS):
        for m in (0, 2):
            assert f.key_of(m, int(out['sel'][i, m])) == _key(GOLD[f'sel_d{D}'][i]), (D, i, m)
    assert np.array_equal(out['sel'], leaves) and np.array_equal(out['child'], childs)
    for m in range(M):
        _same_tree(out, f, m)
        fc = f.first[m, 0]
        assert out['action'][m] == int(np.argmax(f.Nsa[m, fc:fc + A]))
    assert abs(float(out['min_gap'].min()) - f.min_gap) <= 1e-12, (out['min_gap'], f.min_gap)
    if D == 3:
        # a final leaf reached again: its children overwritten in place, `used` not advanced
        again = [(i, m) for i in range(ITERS) for m in range(M) if (out['child'][:i, m] == out['child'][i, m]).any()]
        assert again, 'the D = 3 run never re-expanded a leaf'
        assert out['used'].max() < 1 + A * ITERS


def test_a_tree_out_of_slots_is_frozen_and_alone(driver, tmp_path):
    """Tree 1's slot cursor starts two expansions ahead (slots 1 .. 2 A left unused) and cap is one slot short of what it needs in the
    end, which still holds trees 0 and 2: tree 1 runs out at its last fresh expansion -> status 1, frozen at its state before that
    iteration (a host forest stopped there), trees 0 and 2 as in the run with room for all."""
    D = 10
    used0 = (1, 1 + 2 * A, 1)
    full, q, leaves, _, useds = _host_run(D, ITERS, used0)
    cap = int(full.used[1]) - 1
    assert cap >= max(full.used[0], full.used[2]) and cap >= 1 + A                               # the premise: only tree 1 is short
    stop = int(np.flatnonzero(np.diff(np.concatenate([[used0[1]], useds[:, 1]])) > 0)[-1])       # its last fresh expansion
    assert 0 < stop < ITERS - 1
    before = _host_run(D, stop, used0)[0]
    out = _drive(driver, tmp_path, D, cap, q, used0)
    assert out['status'].tolist() == [0, 1, 0]
    assert (out['sel'][stop:, 1] == -1).all() and np.array_equal(out['sel'][:stop, 1], leaves[:stop, 1])
    _same_tree(out, before, 1, min(cap, before.cap))
    assert (out['first'][1, before.cap:] == -1).all() and not out['Nsa'][1, before.cap:].any()
    for m in (0, 2):
        _same_tree(out, full, m, cap)
        assert np.array_equal(out['sel'][:, m], leaves[:, m])
    ample = _drive(driver, tmp_path, D, full.cap, q, used0)
    assert not ample['status'].any()
    for k in INT_ARRAYS + ('Qsa',):
        for m in (0, 2):
            assert np.array_equal(out[k][m], ample[k][m, :cap]), (k, m)


def test_plan_search_validation_under_sanitizers(driver):
    """stove_plan_search's host-side argument check (csrc/validate.h: plan_search) through the driver: every documented bad argument
    returns hipErrorInvalidValue, R == 0 is accepted, nothing is dereferenced."""
    control_harness.run_modes(driver, ['validate'])


def test_corrupt_trees_are_refused_untouched(driver):
    """status 2 on the CPU, under the sanitizers (the driver's `corrupt` case): children outside the arrays, a parent chain that never
    reaches the root or leaves the arrays, a descent that never ends, a slot cursor outside the arrays -> status 2 each, the tree
    exactly as handed over, nothing read out of bounds, the healthy tree as in a forest nobody damaged."""
    control_harness.run_modes(driver, ['corrupt'])


def test_plan_search_workspace_query_and_switches():
    from stove_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ws, ws_expand = lib.stove_plan_search_ws_bytes, lib.stove_plan_expand_ws_bytes
    assert ws(3, 9, 4, 3, 3) > ws_expand(3, 9, 4, 3, 3) > 0 and ws(4, 9, 4, 3, 3) > ws(3, 9, 4, 3, 3)
    for bad in ((0, 9, 4, 3, 3), (3, 0, 4, 3, 3), (3, 65, 4, 3, 3), (3, 9, 0, 3, 3), (3, 9, 4, 0, 3), (3, 9, 4, 9, 3), (3, 9, 4, 3, 13)):
        assert ws(*bad) == 0, bad
    from stove_amd import ops
    from stove_amd.mcts import mcts_stove as sm
    assert callable(ops.plan_search)
    # the switch: an attribute of the handler, off by default (run_mcts and run_mcts_model keep their parameter lists, which
    # tests/test_mcts_cpu.py pins), and a parameter of plan_on_model, off by default
    h = sm.BatchedMCTSHandler([sm.MCTS(None, torch.zeros(1, 3, 18))], None)
    assert h.device_trees is False
    p = inspect.signature(sm.plan_on_model).parameters
    assert list(p)[:6] == list(inspect.signature(sm.run_mcts_model).parameters)
    assert p['device_trees'].default is False and p['fused'].default is None
    assert sm.FUSED_WHERE_ELIGIBLE is False


def test_forest_round_trip_through_tensors():
    """Forest.to_device / from_device (on the CPU device here): int32 / float64 tensors and back, indistinguishable from the forest
    they came from; min_gap merged with min; key views read the restored arrays."""
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    src = _host_run(3)[0]
    trees = [MCTS(torch.zeros(1, 1, 3), torch.from_numpy(GOLD['z0_d3']), action_space=A, max_rollout_depth=3) for _ in range(M)]
    h = BatchedMCTSHandler(trees, torch.zeros(M, 1, 3), action_space=A, max_rollout_depth=3)
    f = h.forest
    f.reserve(src.cap)
    t = src.to_device('cpu')
    assert all(t[k].dtype == torch.int32 for k in INT_ARRAYS + ('used', 'status')) and t['Qsa'].dtype == t['min_gap'].dtype == torch.float64
    assert not t['status'].any() and bool(torch.isinf(t['min_gap']).all())
    t['min_gap'][1] = 0.25
    f.min_gap = 0.5
    f.from_device(t)
    for k in INT_ARRAYS + ('Qsa', 'used'):
        assert getattr(f, k).dtype == getattr(src, k).dtype and np.array_equal(getattr(f, k), getattr(src, k)), k
    assert f.min_gap == 0.25
    assert sorted(trees[2].Qsa.keys()) == sorted(src.keys(2)) and trees[0].Nsa['r' + str(int(GOLD['action_d3']))] >= 1
