"""GPU tests of planning on the learned model: the fused tree expansion (stove_plan_expand, csrc/plan.hip; ops.plan_expand) against the
float64 oracle, against Stove.rollout bit for bit, under bad device indices and bad host arguments, under graph capture, and the batched
search (stove_amd.mcts) fused against composed and end to end.  Configuration 'ac3' (action-conditioned, appearance in the core:
23 inputs per node), M = 3 trees x A = 9 actions = 27 rows -- no multiple of the four waves of a reward-head workgroup."""
import functools

import numpy as np
import pytest
import torch

import plan_cases
from gpu_helpers import check, err, fill_analytic, regime_bar
from helpers import oracle_setup
from test_gpu_dynamics import CASES, make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INVALID = 1          # hipErrorInvalidValue
CFG = CASES['ac3']
M, A, N, APP = 3, 9, 3, 3
CAP = 22
LEAF, CHILD = (0, 5, 21), (1, 10, 3)             # child ranges 1..9, 10..18, 3..11: inside the pool, clear of the tree's leaf
GAMMA = 0.95


@functools.lru_cache(maxsize=None)
def _model(regime='analytic'):
    from stove_amd.video_prediction.stove import Stove
    return fill_analytic(Stove(make_cfg(**CFG)), '', regime).to(DEV)


@functools.lru_cache(maxsize=None)
def _oracle(regime, dtype):
    c, _, params = oracle_setup(dtype, requires_grad=False, regime=regime, **CFG)
    return c, params


def _weights(st):
    """what stove_plan_expand reads of the model: embedding, GNN image, reward-head block"""
    from stove_amd import ops
    dyn = st.dyn
    h0, h1 = dyn.reward_head0, dyn.reward_head1
    rh = torch.cat([p.detach().reshape(-1) for p in (h0[0].weight, h0[0].bias, h0[2].weight, h0[2].bias, h1[0].weight, h1[0].bias,
                                                     h1[2].weight, h1[2].bias, h1[4].weight, h1[4].bias)]).contiguous()
    gnn = ops.gnn_width(32).image(*[t.detach().float().contiguous() for t in dyn.param_image(0)])
    lay = dyn.action_embedding_layer
    return lay.weight.detach().contiguous(), lay.bias.detach().contiguous(), gnn, rh


@functools.lru_cache(maxsize=None)
def _inputs(L, trees=M, seed=11):
    """leaf states, appearances and random-rollout actions from a seeded CPU generator (shared, never modified)"""
    g = torch.Generator().manual_seed(seed + L)
    z = torch.cat([torch.rand(trees, N, 2, generator=g) * 0.2 + 0.1, torch.rand(trees, N, 16, generator=g) * 1.2 - 0.6], -1)
    app = torch.rand(trees, N, APP, generator=g)
    acts = torch.randint(0, A, (trees * A, L), generator=g, dtype=torch.int32)
    return z, app, acts


def _pool(z, leaf, cap=CAP):
    """NaN everywhere but the leaf slots"""
    pool = torch.full((z.shape[0], cap, N, 18), float('nan'))
    pool[torch.arange(z.shape[0]), torch.tensor(leaf)] = z
    return pool.to(DEV)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _expand(st, pool, leaf, child, len_s, app, acts, D):
    from stove_amd import ops
    emb_w, emb_b, gnn, rh = _weights(st)
    out = ops.plan_expand(pool, _i32(leaf), _i32(child), _i32(len_s), app.to(DEV), acts.to(DEV), emb_w, emb_b, gnn, rh, D, 2, st.dyn.use_elu,
                          st.dyn.loop_consts(), GAMMA, want_rewards=True)
    torch.cuda.synchronize()
    return out


def _one_hot_actions(acts, trees=M):
    return plan_cases.one_hot_actions(acts, A, trees)


def _oracle_rollout(regime, dtype, z, app, acts):
    c, params = _oracle(regime, dtype)
    return plan_cases.oracle_rollout(c, params, z, app, acts, A)


def _value(rew, len_s, D, dtype):
    return plan_cases.value(rew, len_s, D, dtype, M, A, GAMMA)


# ------------------------------------------------------------------------------------------------ 1. the float64 oracle
# len_s = 1 (every one of the L rewards counted: min(2 D - len_s + 1, L) = L), 1 < len_s < D, len_s = D (rollout term exactly 0);
# (5, 7): L < 2 D, so that the clip to L cuts below 2 D - len_s + 1 in every tree
@pytest.mark.parametrize('D,L,len_s', [(2, 4, (1, 2, 2)), (5, 10, (1, 3, 5)), (5, 7, (1, 3, 5))])
@pytest.mark.parametrize('regime', ['analytic', 'init'])
def test_plan_expand_against_the_oracle(regime, D, L, len_s):
    """q, r_first, r_roll and the child states against O.rollout in float64 given one-hot actions and the tiled appearance.  Bars as
    tests/test_gpu_rollout_sample.py section 2 builds them: the plain bars of the mean rollout there (z 3e-6, rewards 3e-6; q is a
    sum of rewards minus one, all of one sign, with positive weights, so it inherits the rewards' bar), regime_bar'ed with the float32
    ORACLE's own distance to the float64 oracle on the same inputs (6 x that gap where it is larger), printed next to the kernel's."""
    st = _model(regime)
    z, app, acts = _inputs(L)
    z_o, r_o = _oracle_rollout(regime, torch.float64, z, app, acts)
    z_f, r_f = _oracle_rollout(regime, torch.float32, z, app, acts)
    q_o, q_f = _value(r_o, len_s, D, np.float64), _value(r_f, len_s, D, np.float32)
    gaps = dict(z=err(z_f[:, 0], z_o[:, 0]), r_first=err(r_f[:, 0], r_o[:, 0]), r_roll=err(r_f[:, 1:], r_o[:, 1:]), q=err(q_f, q_o))
    pool = _pool(z, LEAF)
    q, r_first, r_roll = _expand(st, pool, LEAF, CHILD, len_s, app, acts, D)
    kids = torch.stack([pool[m, CHILD[m]:CHILD[m] + A] for m in range(M)]).flatten(0, 1)
    got = dict(z=err(kids, z_o[:, 0]), r_first=err(r_first.flatten(), r_o[:, 0]), r_roll=err(r_roll.flatten(0, 1), r_o[:, 1:]), q=err(q, q_o))
    print(f'plan.oracle {regime} D={D} L={L}: ' + '  '.join(f'{k} {got[k]:.3g} (oracle f32 gap {gaps[k]:.3g})' for k in got))
    for k in got:
        check(f'plan.oracle.{k}', got[k], regime_bar(3e-6, gaps[k]))
    for m in range(M):
        if len_s[m] == D:                    # the empty discount sum: exactly the first term
            want = (r_first[m] - 1.0) * torch.tensor(GAMMA, device=DEV) ** D
            assert float(((q[m] - want).abs() / want.abs()).max()) < 1e-6


# ------------------------------------------------------------------------------------------------ 2. child states, bit for bit
def test_child_states_are_the_rollouts_and_nothing_else_is_written():
    D, L, len_s = 5, 10, (1, 3, 5)
    st = _model()
    z, app, acts = _inputs(L)
    pool = _pool(z, LEAF)
    before = pool.clone()
    _expand(st, pool, LEAF, CHILD, len_s, app, acts, D)
    with torch.no_grad():
        want, _ = st.rollout(z.repeat_interleave(A, 0).to(DEV), num=1, actions=_one_hot_actions(acts)[:, :1].float().to(DEV),
                             appearance=app.repeat_interleave(A, 0).to(DEV))
    want = want.view(M, A, N, 18)
    written = torch.zeros(M, CAP, dtype=torch.bool, device=DEV)
    for m in range(M):
        assert torch.equal(pool[m, CHILD[m]:CHILD[m] + A], want[m]), m
        written[m, CHILD[m]:CHILD[m] + A] = True
    same = pool.view(torch.int32) == before.view(torch.int32)                       # (NaN slots compare by their bits)
    assert bool(same[~written].all())
    assert bool(torch.isfinite(pool[written]).all())


def test_plan_expand_is_reproducible_and_refuses_autograd():
    from stove_amd import ops
    D, L, len_s = 2, 4, (1, 2, 2)
    st = _model()
    z, app, acts = _inputs(L)
    a = _expand(st, _pool(z, LEAF), LEAF, CHILD, len_s, app, acts, D)
    b = _expand(st, _pool(z, LEAF), LEAF, CHILD, len_s, app, acts, D)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    emb_w, emb_b, gnn, rh = _weights(st)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.plan_expand(_pool(z, LEAF), _i32(LEAF), _i32(CHILD), _i32(len_s), app.to(DEV).requires_grad_(), acts.to(DEV), emb_w, emb_b, gnn,
                        rh, D, 2, st.dyn.use_elu, st.dyn.loop_consts())


# ------------------------------------------------------------------------------------------------ 3. fused against composed
SEARCH_SEED = 9


def _search(st, fused, seed):
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    z, app, _ = _inputs(6, trees=4, seed=42)
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=A, max_rollout_depth=3) for m in range(4)]
    h = BatchedMCTSHandler(trees, app, action_space=A, max_rollout_depth=3)
    np.random.seed(seed)
    actions = h.run_mcts(st, 12, fused=fused)
    counts = np.array([[t.Nsa['r' + str(a)] for a in range(A)] for t in trees])
    return actions, counts, h.forest.min_gap


def test_fused_search_equals_composed_search():
    """run_mcts(fused=True) against run_mcts(fused=False) under the same numpy seed: 4 trees, D = 3, 12 expansions -> identical root
    visit counts and actions.  The two differ in the rounding of q (float32 on the device against float64 on the host from the same
    float32 rewards, 1e-7 relative), so the run must keep every UCT decision at least 1e-4 apart: the forest reports the smallest gap
    and the test FAILS below that.  The 'init' weights: under the 'analytic' ones the rewards hardly depend on the action (root values
    1e-5 apart).  Root states of generator seed 42, numpy seed 9, chosen on the float64 oracle (smallest gap 1.9e-4, the widest of 75
    seed pairs tried there)."""
    st = _model('init')
    act_f, n_f, gap_f = _search(st, True, SEARCH_SEED)
    act_c, n_c, gap_c = _search(st, False, SEARCH_SEED)
    print(f'plan.search: smallest decision gap fused {gap_f:.3g} composed {gap_c:.3g}; actions {act_f}; root visits {n_f.tolist()}')
    assert min(gap_f, gap_c) >= 1e-4, (gap_f, gap_c)
    assert act_f == act_c and np.array_equal(n_f, n_c)
    assert n_f.sum(1).tolist() == [12 - 1 + 9] * 4               # nine first visits, then one more per later expansion


# ------------------------------------------------------------------------------------------------ 4. bad device indices
def test_bad_device_indices_poison_their_tree_only():
    """trees 0 and 5 valid; 1: leaf = cap; 2: child range one past the pool; 3: one action index = A; 4: len_s = D + 1"""
    D, L, T = 3, 6, 6
    st = _model()
    z, app, acts = _inputs(L, trees=T, seed=77)
    leaf, child, len_s = [0, 0, 0, 0, 0, 4], [1, 1, 1, 1, 1, 10], [1, 1, 1, 1, 1, 2]
    good_pool = _pool(z, leaf)
    q_ok, rf_ok, rr_ok = _expand(st, good_pool, leaf, child, len_s, app, acts, D)
    assert bool(torch.isfinite(q_ok).all())
    bad_leaf, bad_child, bad_len, bad_acts = list(leaf), list(child), list(len_s), acts.clone()
    bad_leaf[1] = CAP
    bad_child[2] = CAP - A + 1
    bad_acts[3 * A + 2, 1] = A
    bad_len[4] = D + 1
    pool = _pool(z, leaf)
    before = pool.clone()
    q, rf, rr = _expand(st, pool, bad_leaf, bad_child, bad_len, app, bad_acts, D)
    for m in (1, 2, 3, 4):
        assert bool(torch.isnan(q[m]).all()) and bool(torch.isnan(rf[m]).all()) and bool(torch.isnan(rr[m]).all()), m
        assert bool((pool[m].view(torch.int32) == before[m].view(torch.int32)).all()), m            # no slot of a bad tree written
    for m in (0, 5):
        assert torch.equal(q[m], q_ok[m]) and torch.equal(rf[m], rf_ok[m]) and torch.equal(rr[m], rr_ok[m]), m
        assert bool((pool[m].view(torch.int32) == good_pool[m].view(torch.int32)).all()), m


# ------------------------------------------------------------------------------------------------ 5. bad host arguments
def test_plan_expand_rejects_bad_host_arguments():
    from stove_amd import _lib
    lib = _lib.load()
    p = _lib.ptr
    D, L = 3, 6
    st = _model()
    z, app, acts = _inputs(L)
    emb_w, emb_b, gnn, rh = _weights(st)
    pool = _pool(z, LEAF)
    before = pool.clone()
    leaf, child, len_s = _i32(LEAF), _i32(CHILD), _i32((1, 2, 3))
    app, acts = app.to(DEV), acts.to(DEV)
    q = torch.full((M, A), 7.0, device=DEV)
    rf = torch.full((M, A), 7.0, device=DEV)
    rr = torch.full((M, A, L), 7.0, device=DEV)
    ws = torch.zeros(lib.stove_plan_expand_ws_bytes(M, A, L, N, APP) // 4 + 1, device=DEV)
    ptrs = dict(z_pool=p(pool), leaf=p(leaf), child=p(child), len_s=p(len_s), app=p(app), acts=p(acts), emb_w=p(emb_w), emb_b=p(emb_b),
                gnn=p(gnn), rh=p(rh), q=p(q), r_first=p(rf), r_roll=p(rr), ws=p(ws))
    dims = dict(M=M, cap=CAP, A=A, L=L, D=D, N=N, app_dim=APP)

    def call(**change):
        pp, dd = dict(ptrs), dict(dims)
        for k, v in change.items():
            (pp if k in pp else dd)[k] = v
        return lib.stove_plan_expand(*pp.values(), *dd.values(), 2, int(st.dyn.use_elu), *[float(c) for c in st.dyn.loop_consts()], GAMMA,
                                     _lib.stream())
    bad = [{k: None} for k in ptrs if k not in ('r_first', 'r_roll')]
    bad += [dict(M=0), dict(A=0), dict(L=0), dict(N=0), dict(D=0), dict(M=-1), dict(N=9), dict(A=65), dict(cap=A), dict(app_dim=13)]
    for change in bad:
        rc = call(**change)
        assert rc == INVALID, (change, rc)
        msg = lib.stove_error_string(rc)
        assert msg and b'invalid' in msg.lower()
    torch.cuda.synchronize()
    assert float(q.min()) == 7.0 and float(rf.min()) == 7.0 and float(rr.min()) == 7.0                 # nothing was written
    assert bool((pool.view(torch.int32) == before.view(torch.int32)).all())
    assert call() == 0 and call(r_first=None, r_roll=None) == 0                                         # and the stream still works
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all()) and float(rr.max()) < 1.0


# ------------------------------------------------------------------------------------------------ 6. graph capture
def test_plan_expand_replays_from_a_graph_bit_for_bit():
    from stove_amd import _lib
    lib = _lib.load()
    p = _lib.ptr
    D, L, len_s = 5, 10, (1, 3, 5)
    st = _model()
    z, app, acts = _inputs(L)
    want_pool = _pool(z, LEAF)
    want = _expand(st, want_pool, LEAF, CHILD, len_s, app, acts, D)
    emb_w, emb_b, gnn, rh = _weights(st)
    pool = _pool(z, LEAF)
    leaf, child, ls, app, acts = _i32(LEAF), _i32(CHILD), _i32(len_s), app.to(DEV), acts.to(DEV)
    q = torch.zeros(M, A, device=DEV)
    rf = torch.zeros(M, A, device=DEV)
    rr = torch.zeros(M, A, L, device=DEV)
    ws = torch.zeros(lib.stove_plan_expand_ws_bytes(M, A, L, N, APP) // 4 + 1, device=DEV)

    def call():
        rc = lib.stove_plan_expand(p(pool), p(leaf), p(child), p(ls), p(app), p(acts), p(emb_w), p(emb_b), p(gnn), p(rh), p(q), p(rf), p(rr),
                                   p(ws), M, CAP, A, L, D, N, APP, 2, int(st.dyn.use_elu), *[float(c) for c in st.dyn.loop_consts()], GAMMA,
                                   _lib.stream())
        assert rc == 0, rc
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in (q, rf, rr):
        t.zero_()
    pool.copy_(_pool(z, LEAF))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(q, want[0]) and torch.equal(rf, want[1]) and torch.equal(rr, want[2])
    assert bool((pool.view(torch.int32) == want_pool.view(torch.int32)).all())


# ------------------------------------------------------------------------------------------------ end to end
def test_run_mcts_model_end_to_end():
    """an untrained ac3 model, frames from initialize_img over four AvoidanceTasks -> four actions in [0, 9)"""
    from stove_amd.envs import envs
    from stove_amd.mcts.mcts_stove import initialize_img, run_mcts_model
    from stove_amd.video_prediction.stove import Stove
    torch.manual_seed(0)
    model = Stove(make_cfg(**CFG)).to(DEV)
    tasks = [envs.AvoidanceTask(envs.make_env('avoidance', 100 + i, 32), 4, greyscale=False, action_force=0.6) for i in range(4)]
    img, actions = initialize_img(tasks, steps=8, res=32)
    assert img.shape == (4, 8, 32, 32, 3) and tuple(actions.shape) == (4, 8, 9)
    np.random.seed(1)
    out = run_mcts_model(img, model, actions, num_parallel_envs=4, mcts_steps=6, max_rollout_depth=3)
    assert len(out) == 4 and all(isinstance(a, int) and 0 <= a < 9 for a in out), out
    from stove_amd.mcts import mcts_stove
    saved = mcts_stove.FUSED_WHERE_ELIGIBLE
    try:                                                  # the same through the other expansion path, whichever the default is
        mcts_stove.FUSED_WHERE_ELIGIBLE = not saved
        np.random.seed(1)
        other = run_mcts_model(img, model, actions, num_parallel_envs=4, mcts_steps=6, max_rollout_depth=3)
    finally:
        mcts_stove.FUSED_WHERE_ELIGIBLE = saved
    assert len(other) == 4 and all(isinstance(a, int) and 0 <= a < 9 for a in other), other
