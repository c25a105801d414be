"""CPU-side checks (-m "not gpu") of planning on the learned model (stove_amd.mcts, model.mcts): the host tree replays the reference's
MCTS class on tests/golden/g21_mcts_tree.npz (tools/make_mcts_goldens.py), the module surface is the reference's without its process
pool, and the workspace query rejects what the call rejects.  (All fail before the feature: the module and the symbols do not exist.)"""
import re
import sys

import numpy as np
import pytest
import torch

import control_harness
from helpers import load_golden

GOLD = load_golden('g21_mcts_tree')
A, ITERS = int(GOLD['actions']), int(GOLD['iters'])


def _key(row):
    return 'r' + ''.join(str(int(d)) for d in row if d >= 0)


def _check_tree(tree, D):
    g = {k: GOLD[f'{k}_d{D}'] for k in ('keys', 'nsa', 'qsa', 'ns', 'action')}
    keys = [_key(r) for r in g['keys']]
    assert sorted(tree.Qsa.keys()) == sorted(keys)
    for k, nsa, qsa, ns in zip(keys, g['nsa'], g['qsa'], g['ns']):
        assert tree.Nsa[k] == nsa and tree.Ns[k] == ns, k
        assert abs(tree.Qsa[k] - qsa) <= 1e-6 * abs(qsa), (k, tree.Qsa[k], qsa)
    counts = [tree.Nsa['r' + str(a)] for a in range(A)]
    assert int(np.argmax(counts)) == int(g['action'])


@pytest.mark.parametrize('D', [3, 10])
def test_single_tree_replays_the_reference(D):
    """MCTS.select / MCTS.backpropagate, one tree, the reference's own call sequence: the identical key at every iteration, identical
    Nsa / Ns and action, Qsa within 1e-6 relative (float32 summation order in the reference's value; the recorded smallest decision gap
    is far above it)."""
    from stove_amd.mcts.mcts_stove import MCTS
    assert float(GOLD[f'gap_d{D}']) >= 1e-4
    rs, rr, zs = (torch.from_numpy(GOLD[f'{k}_d{D}']) for k in ('rs', 'rr', 'zs'))
    tree = MCTS(torch.zeros(1, 1, 3), torch.from_numpy(GOLD[f'z0_d{D}']), action_space=A, max_rollout_depth=D)
    assert tree.Nsa['r'] == 0 and tree.Qsa['r'] == 0 and tree.Ns['r'] == 0
    for i in range(ITERS):
        s, z = tree.select('r', tree.Zstate['r'])
        assert s == _key(GOLD[f'sel_d{D}'][i]), i
        want_z = GOLD[f'z0_d{D}'] if s == 'r' else None
        if want_z is not None:
            assert np.array_equal(z.numpy(), want_z)
        tree.backpropagate(zs[i], rs[i], rr[i], s)
        assert np.array_equal(tree.Zstate[s + '4'].numpy(), zs[i, 4].numpy())
    _check_tree(tree, D)
    assert tree._f.min_gap == pytest.approx(float(GOLD[f'gap_d{D}']), rel=1e-5)


def test_vectorised_forest_replays_the_reference():
    """Each recorded run as a forest of three trees: two copies of the recording around a tree fed other rewards, selected and
    backpropagated together, one pass per tree level.  The copies must follow the recording key for key whatever their neighbour
    does (it descends to other depths at other times)."""
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler, discounted_values
    for D in (3, 10):
        rs, rr = GOLD[f'rs_d{D}'][..., 0, 0], GOLD[f'rr_d{D}'][..., 0]              # (iters, A), (iters, A, 2 D)
        trees = [MCTS(torch.zeros(1, 1, 3), torch.from_numpy(GOLD[f'z0_d{D}']), action_space=A, max_rollout_depth=D) for _ in range(3)]
        h = BatchedMCTSHandler(trees, torch.zeros(3, 1, 3), action_space=A, max_rollout_depth=D)
        f = h.forest
        other = np.random.RandomState(5).rand(ITERS, A).astype(np.float32)
        for i in range(ITERS):
            leaf = f.select()
            for m in (0, 2):
                assert f.key_of(m, leaf[m]) == _key(GOLD[f'sel_d{D}'][i]), (D, i, m)
            child = f.child_slots(leaf)
            len_s = f.depth[np.arange(3), leaf] + 1
            q = discounted_values(np.stack([rs[i], other[i], rs[i]]), np.stack([rr[i], rr[i][::-1], rr[i]]), len_s, D)
            f.backpropagate(leaf, child, q)
        for m in (0, 2):
            _check_tree(trees[m], D)
        assert trees[1].Qsa['r0'] != trees[0].Qsa['r0']
        with pytest.raises(RuntimeError):
            trees[0].select('r', None)                   # a tree of a batch is searched through its handler


def test_value_formula_quirks():
    """the reference's broadcast product, the clip of the counted rewards and the empty discount sum at len_s = D"""
    from stove_amd.mcts.mcts_stove import discounted_values
    D, L = 3, 6
    rng = np.random.RandomState(0)
    rs, rr = rng.rand(4, 2), rng.rand(4, 2, L)
    len_s = np.array([1, 2, 3, 3])
    q = discounted_values(rs, rr, len_s, D)
    for m in range(4):
        for a in range(2):
            n = min(2 * D - len_s[m] + 1, L)
            want = (rs[m, a] - 1) * 0.95 ** len_s[m] + sum(rr[m, a, :n] - 1) * sum(0.95 ** j for j in range(len_s[m], D))
            assert q[m, a] == pytest.approx(want, rel=1e-12)
    assert np.array_equal(q[2], (rs[2] - 1) * 0.95 ** 3)                       # len_s = D: the rollout term is exactly 0


def test_module_surface_without_the_process_pool():
    before = set(sys.modules)
    import model.mcts.mcts_stove as mm
    import stove_amd.mcts.mcts_stove as sm
    for name in ('multi_one_hot', 'encode_img', 'MCTS', 'BatchedMCTSHandler', 'run_mcts_model', 'initialize_img', 'update_buffer'):
        assert getattr(mm, name) is getattr(sm, name), name
    for banned in ('multiprocess', 'imageio', 'tqdm'):
        assert banned not in set(sys.modules) - before, banned
        assert not re.search(r'^\s*(import|from)\s+%s\b' % banned, open(sm.__file__).read(), flags=re.M), banned
    import inspect
    assert list(inspect.signature(sm.MCTS.__init__).parameters)[1:] == ['appearance', 'inferred_z', 'action_space', 'max_rollout_depth']
    assert inspect.signature(sm.MCTS.__init__).parameters['max_rollout_depth'].default == 20
    assert list(inspect.signature(sm.BatchedMCTSHandler.__init__).parameters)[1:] == ['trees', 'appearances', 'action_space', 'max_rollout_depth']
    assert list(inspect.signature(sm.BatchedMCTSHandler.run_mcts).parameters)[1:] == ['env', 'runs_per_round', 'fused', 'rollout_actions']
    p = inspect.signature(sm.run_mcts_model).parameters
    assert list(p) == ['img', 'model', 'actions', 'num_parallel_envs', 'mcts_steps', 'max_rollout_depth']
    assert (p['num_parallel_envs'].default, p['mcts_steps'].default, p['max_rollout_depth'].default) == (100, 100, 10)
    assert tuple(sm.multi_one_hot([2, 0], 3).shape) == (1, 2, 3) and sm.multi_one_hot([2, 0], 3)[0, 0, 2] == 1
    assert tuple(sm.encode_img(np.zeros((2, 3, 8, 8, 3))).shape) == (2, 3, 3, 8, 8)


def test_plan_expand_workspace_query():
    from stove_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    # the size query needs no GPU: 0 for what the call rejects, growing with every dimension otherwise
    ws = lib.stove_plan_expand_ws_bytes
    assert ws(3, 9, 4, 3, 3) > 0 and ws(3, 9, 5, 3, 3) > ws(3, 9, 4, 3, 3) and ws(4, 9, 4, 3, 3) > ws(3, 9, 4, 3, 3)
    for bad in ((0, 9, 4, 3, 3), (3, 0, 4, 3, 3), (3, 65, 4, 3, 3), (3, 9, 0, 3, 3), (3, 9, 4, 0, 3), (3, 9, 4, 9, 3), (3, 9, 4, 3, 13),
                (3, 9, 4, 3, -1)):
        assert ws(*bad) == 0, bad
    from stove_amd import ops
    assert callable(ops.plan_expand)


def test_plan_expand_validation_under_sanitizers(tmp_path_factory):
    """stove_plan_expand's host-side argument check (csrc/validate.h) compiled host-only with -fsanitize=address,undefined and driven
    by a stand-alone program (tests/abi/plan_validate_driver.cpp): every case returns the documented code, nothing is dereferenced."""
    control_harness.run_modes(control_harness.build_driver(tmp_path_factory, 'plan_validate_driver'), ['validate'])
