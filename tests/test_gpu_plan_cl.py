"""GPU tests of planning at the state-code lengths cl = 16 and 64 (stove_plan_expand_cl / stove_plan_search_cl, csrc/plan.hip;
ops.plan_expand / ops.plan_search on pools 10 and 34 wide; BatchedMCTSHandler with fused_widths).  Cases, inputs and float64
references: tests/plan_cl_cases.py; the conditions on them: tests/test_plan_cl_cpu.py.

Bars: child states, r_first, r_roll and q at plan_cases.BAR_PLAN = 3e-6, or 6 x the float32 oracle's own gap to the float64 oracle on
the same inputs, measured here on the CPU, where that is larger (gpu_helpers.regime_bar).  The gap has a ceiling, asserted here before
the bar is formed: BAR_PLAN / 6, so that the bar is BAR_PLAN itself, everywhere but under the saturated 'analytic' fill at cl = 16, whose
gaps are held to the committed caps plan_cl_cases.GAP_CAPS_ANALYTIC16.  Everything else is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import plan_cases as P
import plan_cl_cases as C
from gpu_helpers import check_ratio, err, regime_bar
from test_gpu_dynamics import CASES, make_cfg
from test_gpu_plan_counts import _Env, _bits, _i32
from test_gpu_plan_search import _same_as_forest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
EVERY = (16, 32, 64)
MIN_GAP = 1e-9


@functools.lru_cache(maxsize=None)
def _env(cl, N, A, app, elu, regime):
    from stove_amd.video_prediction.dynamics import Dynamics
    return _Env(P.fill_module(Dynamics(make_cfg(**C.cl_cfg(cl, N, A, app, elu))), 'dyn.', regime).to(DEV))


def _case_env(case, fill):
    return _env(case.cl, case.N, case.A, case.app, case.elu, C.regime_of(case, fill))


def _weights(env):
    from stove_amd.mcts.mcts_stove import BatchedMCTSHandler
    return BatchedMCTSHandler._fused_weights(env)


def _pool(z, leaf, cap):
    """a pool out of NaN-filled memory: NaN everywhere but the leaf slots"""
    pool = torch.full((z.shape[0], cap) + tuple(z.shape[1:]), NAN)
    pool[torch.arange(z.shape[0]), torch.tensor(leaf)] = z.float()
    return pool.to(DEV)


def _expand(env, case, z, app, acts, leaf=None, child=None, len_s=None):
    """-> (pool before, pool after, q, r_first, r_roll)"""
    from stove_amd import ops
    leaf, child, len_s = (case.leaf if leaf is None else leaf), (case.child if child is None else child), (case.len_s if len_s is None else len_s)
    pool = _pool(z, case.leaf, case.cap)
    before = pool.clone()
    emb_w, emb_b, gnn, rh = _weights(env)
    assert rh.numel() == C.rh_floats(case.cl) and pool.shape[-1] == case.cl // 2 + 2
    q, rf, rr = ops.plan_expand(pool, _i32(leaf), _i32(child), _i32(len_s), app.float().to(DEV) if app is not None else None,
                                acts.to(torch.int32).to(DEV), emb_w, emb_b, gnn, rh, case.D, 2, env.dyn.use_elu, env.dyn.loop_consts(), C.GAMMA,
                                want_rewards=True)
    torch.cuda.synchronize()
    return before, pool, q, rf, rr


def _kids(pool, case):
    return torch.stack([pool[m, case.child[m]:case.child[m] + case.A] for m in range(case.M)]).flatten(0, 1)


def _written(case):
    w = torch.zeros(case.M, case.cap, dtype=torch.bool, device=DEV)
    for m in range(case.M):
        w[m, case.child[m]:case.child[m] + case.A] = True
    return w


def _named(cl, stem):
    case, = [c for c in C.expansion_cases(cl) if c.name.startswith('cl%d-%s' % (cl, stem))]
    return case


# ------------------------------------------------------------------------------------------------ 1 - 3. the expansion
@pytest.mark.parametrize('case', C.all_cases(), ids=C.case_id)
def test_plan_expand_against_the_oracle(case):
    """under every fill: child states, r_first, r_roll and q against O.rollout + the value formula in float64; the pool outside the
    child slots untouched bit for bit; two runs bit-equal; child states = Stove.rollout(num = 1) bit for bit (the same kernel)"""
    z, app, acts = C.inputs(case)
    for fill in C.FILLS:
        env = _case_env(case, fill)
        before, pool, q, rf, rr = _expand(env, case, z, app, acts)
        again = _expand(env, case, z, app, acts)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((pool, q, rf, rr), again[1:])), fill
        written = _written(case)
        assert bool((_bits(pool) == _bits(before))[~written].all()), 'a slot outside the child ranges was written'
        assert bool(torch.isfinite(pool[written]).all()) and bool(torch.isfinite(q).all())
        kids = _kids(pool, case)
        with torch.no_grad():
            first = P.one_hot_actions(acts, case.A, case.M)[:, :1].float().to(DEV)
            want, _ = env.rollout(z.float().repeat_interleave(case.A, 0).to(DEV), num=1, actions=first,
                                  appearance=app.float().repeat_interleave(case.A, 0).to(DEV) if app is not None else None)
        assert torch.equal(_bits(kids), _bits(want[:, 0])), 'child states differ from Stove.rollout(num = 1)'
        ref, gaps = C.expansion_reference(case, fill), C.float32_gaps(case, fill)
        got = {'z': err(kids, ref['z']), 'r_first': err(rf.flatten(), ref['r'][:, 0]), 'r_roll': err(rr.flatten(0, 1), ref['r'][:, 1:]),
               'q': err(q, ref['q'])}
        print('plan_cl.%s-%s: ' % (case.name, fill) + '  '.join('%s %.3g (f32 gap %.3g)' % (k, got[k], gaps[k]) for k in got))
        for k in got:
            assert gaps[k] < C.gap_cap(case, fill, k), (case.name, fill, k, gaps[k])          # the ceiling of the bar formed next
            check_ratio('plan_cl.expand.' + k, got[k], regime_bar(C.BAR_PLAN, gaps[k]))
        for m in range(case.M):
            if case.len_s[m] == case.D:                    # the empty discount sum: exactly the first term
                want_q = (rf[m] - 1.0) * torch.tensor(C.GAMMA, device=DEV) ** case.D
                assert float(((q[m] - want_q).abs() / want_q.abs()).max()) < 1e-6


# ------------------------------------------------------------------------------------------------ 4. bad device indices
@pytest.mark.parametrize('cl', C.WIDTHS)
def test_bad_device_indices_poison_their_tree_only(cl):
    """tree 1 with leaf = cap, a child range one past the pool, len_s = D + 1 or one action index = A: NaN rows, no slot written, the
    other trees bit for bit as in the clean run"""
    case = _named(cl, 'counts-N3')
    env = _case_env(case, 'scaled')
    z, app, acts = C.inputs(case)
    _, pool_ok, q_ok, rf_ok, rr_ok = _expand(env, case, z, app, acts)
    assert bool(torch.isfinite(q_ok).all())
    bad_acts = acts.clone()
    bad_acts[1 * case.A + 2, case.L - 1] = case.A
    swap = lambda v, x: tuple(x if m == 1 else y for m, y in enumerate(v))
    for bad in (dict(leaf=swap(case.leaf, case.cap)), dict(leaf=swap(case.leaf, -1)), dict(child=swap(case.child, case.cap - case.A + 1)),
                dict(len_s=swap(case.len_s, case.D + 1)), dict(len_s=swap(case.len_s, 0)), dict(acts=bad_acts)):
        before, pool, q, rf, rr = _expand(env, case, z, app, bad.pop('acts', acts), **bad)
        for m in range(case.M):
            if m == 1:
                assert bool(torch.isnan(q[m]).all()) and bool(torch.isnan(rf[m]).all()) and bool(torch.isnan(rr[m]).all()), bad
                assert torch.equal(_bits(pool[m]), _bits(before[m])), bad
            else:
                assert all(torch.equal(_bits(a[m]), _bits(b[m])) for a, b in ((q, q_ok), (rf, rf_ok), (rr, rr_ok))), bad
                assert torch.equal(_bits(pool[m]), _bits(pool_ok[m])), bad


# ------------------------------------------------------------------------------------------------ 5. fused against composed
def _handler(s, widths=EVERY, device_trees=False):
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    z, app, acts = C.search_inputs(s)
    z, app = z.float(), app.float()
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=s.A, max_rollout_depth=s.D) for m in range(s.M)]
    h = BatchedMCTSHandler(trees, app, action_space=s.A, max_rollout_depth=s.D)
    assert h.fused_widths == (32,) and h.device_trees is False                    # the defaults
    h.fused_widths, h.device_trees = widths, device_trees
    return h, acts


def _recorded(h):
    leaves, select = [], h.forest.select

    def recording_select():
        leaf = select()
        leaves.append(leaf.copy())
        return leaf
    h.forest.select = recording_select
    return leaves


def _search_env(s):
    return _env(s.cl, s.N, s.A, s.app, False, C.search_regime(s.cl))


@pytest.mark.parametrize('cl', C.WIDTHS)
def test_fused_search_equals_composed_search(cl):
    """run_mcts(fused=True) against run_mcts(fused=False) on the same random-rollout actions, N = 3, M = 3, D = 3, 12 iterations: the
    same leaf per iteration and the same actions.  The two differ in the rounding of the rewards and of q, so the inputs must keep
    every UCT decision SEARCH_GAP apart: asserted on the float64 oracle by the CPU test, and here on both host forests first."""
    s = C.search_case(cl, 3, 12)
    env = _search_env(s)
    out = {}
    for fused in (True, False):
        h, acts = _handler(s)
        leaves = _recorded(h)
        actions = h.run_mcts(env, s.R, fused=fused, rollout_actions=acts)
        out[fused] = (actions, np.stack(leaves), h.forest.min_gap, h.forest.Nsa.copy())
    print('plan_cl.search cl=%d: smallest decision gap fused %.3g composed %.3g; actions %s' % (cl, out[True][2], out[False][2], out[True][0]))
    assert min(out[True][2], out[False][2]) >= C.SEARCH_GAP
    assert np.array_equal(out[True][1], out[False][1]) and out[True][0] == out[False][0]
    assert np.array_equal(out[True][3], out[False][3])


# ------------------------------------------------------------------------------------------------ 6. device trees against the host search
@pytest.mark.parametrize('D,R', [(2, 12), (5, 40)])
@pytest.mark.parametrize('cl', C.WIDTHS)
def test_device_search_equals_host_search(cl, D, R):
    """handler.device_trees = True and ops.plan_search itself against the host forest searching on the same expansion kernel: the same
    leaf per iteration, integer arrays equal, Qsa and the whole pool bit for bit, min_gap equal, all statuses 0.  The host forest's
    smallest decision gap must be >= 1e-9 first (a condition on the inputs: one ulp of `log` moves a UCT value by far less)."""
    from stove_amd import ops
    from stove_amd.mcts.mcts_stove import Forest
    s = C.search_case(cl, D, R)
    env = _search_env(s)
    host, acts = _handler(s)
    leaves = _recorded(host)
    act_h = host.run_mcts(env, R, fused=True, rollout_actions=acts)
    assert host.forest.min_gap >= MIN_GAP, host.forest.min_gap
    dev, _ = _handler(s, device_trees=True)
    act_d = dev.run_mcts(env, R, rollout_actions=acts)
    assert act_d == act_h and dev.forest.cap == host.forest.cap
    _same_as_forest({k: getattr(dev.forest, k) for k in ('first', 'parent', 'depth', 'Ns', 'Nsa', 'Qsa', 'used')}, host.forest, pool=dev.forest.z)
    assert abs(dev.forest.min_gap - host.forest.min_gap) <= 1e-12
    # the op itself, with the leaves it selected
    z, app, _ = C.search_inputs(s)
    cap = host.forest.cap
    pool = torch.zeros(s.M, cap, s.N, cl // 2 + 2)
    pool[:, 0] = z.float()
    pool = pool.to(DEV)
    arrays = Forest(s.M, s.A, D, cap=cap).to_device(DEV)
    sel = torch.full((R, s.M), -5, dtype=torch.int32, device=DEV)
    emb_w, emb_b, gnn, rh = _weights(env)
    with torch.no_grad():
        action = ops.plan_search(pool, arrays, app.float().to(DEV), torch.from_numpy(acts.astype(np.int32)).to(DEV), emb_w, emb_b, gnn, rh, D, 2,
                                 env.dyn.use_elu, env.dyn.loop_consts(), C.GAMMA, sel_trace=sel)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in arrays.items()}
    assert not got['status'].any()
    assert np.array_equal(sel.cpu().numpy(), np.stack(leaves))
    _same_as_forest(got, host.forest, pool=pool)
    assert action.cpu().tolist() == act_h
    assert abs(float(got['min_gap'].min()) - host.forest.min_gap) <= 1e-12
    print('plan_cl.device_search cl=%d D=%d R=%d: smallest gap host %.3g device %.3g; actions %s' % (cl, D, R, host.forest.min_gap,
                                                                                                   float(got['min_gap'].min()), act_h))


@pytest.mark.parametrize('cl', C.WIDTHS)
def test_a_tree_out_of_slots_on_the_device(cl):
    """a pool with room for one expansion: the second iteration selects a fresh leaf, finds no slots and freezes every tree with
    status 1 -- arrays and pool as after the first iteration"""
    from stove_amd import ops
    from stove_amd.mcts.mcts_stove import Forest
    s = C.search_case(cl, 5, 40)
    env = _search_env(s)
    z, app, acts = C.search_inputs(s)
    emb_w, emb_b, gnn, rh = _weights(env)
    cap = 1 + s.A

    def run(R):
        pool = torch.zeros(s.M, cap, s.N, cl // 2 + 2)
        pool[:, 0] = z.float()
        pool = pool.to(DEV)
        arrays = Forest(s.M, s.A, s.D, cap=cap).to_device(DEV)
        with torch.no_grad():
            ops.plan_search(pool, arrays, app.float().to(DEV), torch.from_numpy(acts[:R].astype(np.int32)).to(DEV), emb_w, emb_b, gnn, rh, s.D, 2,
                            env.dyn.use_elu, env.dyn.loop_consts(), C.GAMMA)
        torch.cuda.synchronize()
        return pool, {k: v.cpu() for k, v in arrays.items()}
    pool1, one = run(1)
    pool3, three = run(3)
    assert one['status'].tolist() == [0] * s.M and three['status'].tolist() == [1] * s.M
    assert torch.equal(_bits(pool3), _bits(pool1))
    for k in ('first', 'parent', 'depth', 'Ns', 'Nsa', 'Qsa', 'used'):
        assert torch.equal(one[k], three[k]), k


# ------------------------------------------------------------------------------------------------ 7. graph replay
@pytest.mark.parametrize('cl', C.WIDTHS)
def test_plan_expand_cl_replays_from_a_graph_bit_for_bit(cl):
    from stove_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    case = _named(cl, 'counts-N3')
    env = _case_env(case, 'scaled')
    z, app, acts = C.inputs(case)
    _, want_pool, *want = _expand(env, case, z, app, acts)
    emb_w, emb_b, gnn, rh = _weights(env)
    M, A, L, N = case.M, case.A, case.L, case.N
    pool = _pool(z, case.leaf, case.cap)
    leaf, child, ls, appd, actsd = _i32(case.leaf), _i32(case.child), _i32(case.len_s), app.float().to(DEV), acts.to(torch.int32).to(DEV)
    q, rf, rr = torch.zeros(M, A, device=DEV), torch.zeros(M, A, device=DEV), torch.zeros(M, A, L, device=DEV)
    nbytes = lib.stove_plan_expand_ws_bytes_cl(cl, M, A, L, N, case.app)
    assert nbytes > 0
    ws = torch.zeros(nbytes // 4 + 1, device=DEV)

    def call():
        rc = lib.stove_plan_expand_cl(p(pool), p(leaf), p(child), p(ls), p(appd), p(actsd), p(emb_w), p(emb_b), p(gnn), p(rh), p(q), p(rf), p(rr),
                                      p(ws), cl, M, case.cap, A, L, case.D, N, case.app, 2, int(env.dyn.use_elu),
                                      *[float(c) for c in env.dyn.loop_consts()], C.GAMMA, _lib.stream())
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
    pool.copy_(_pool(z, case.leaf, case.cap))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((q, rf, rr), want))
    assert torch.equal(_bits(pool), _bits(want_pool))


# ------------------------------------------------------------------------------------------------ 8. defaults and refusals
def _roots_handler(cl, N, widths=None):
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    g = torch.Generator().manual_seed(5)
    z, app = C.draw_states(g, 3, N, cl, 3, 0.9)
    z, app = z.float(), app.float()
    h = BatchedMCTSHandler([MCTS(app[m:m + 1], z[m:m + 1], action_space=9, max_rollout_depth=3) for m in range(3)], app, action_space=9,
                           max_rollout_depth=3)
    h.device_trees = True
    if widths is not None:
        h.fused_widths = widths
    return h


def test_defaults_and_refusals():
    from stove_amd import ops
    from stove_amd.mcts import mcts_stove
    from stove_amd.video_prediction.dynamics import Dynamics
    assert mcts_stove.FUSED_WIDTHS == (32,)
    acts = np.zeros((2, 27, 6), dtype=np.int64)
    env16 = _env(16, 3, 9, 3, False, 'init')
    # the switch left alone: device_trees = True is refused as before the widths were served.  fused=True is refused with the same
    # reason, which is new for this path: it used to reach ops.plan_expand and fail there with 'do not fit'
    h = _roots_handler(16, 3)
    kept = h.forest.z.clone()
    with pytest.raises(ValueError, match='state code length is 16, not 32'):
        h.run_mcts(env16, 2, rollout_actions=acts)
    h.device_trees = False
    with pytest.raises(ValueError, match='state code length is 16, not 32'):
        h.run_mcts(env16, 2, fused=True, rollout_actions=acts)
    assert torch.equal(h.forest.z.cpu(), kept) and int(h.forest.used.max()) == 1
    # a handler that offers 16 and 64 only refuses a cl = 32 model both ways too
    env32 = _env(32, 3, 9, 3, False, 'init')
    for device_trees in (True, False):
        h = _roots_handler(32, 3, (16, 64))
        h.device_trees = device_trees
        with pytest.raises(ValueError, match='state code length is 32, not 16 or 64'):
            h.run_mcts(env32, 2, fused=True, rollout_actions=acts)
        assert int(h.forest.used.max()) == 1
    # switched on: what the width's kernels do not take is named
    crowded = _Env(Dynamics(make_cfg(**C.cl_cfg(16, 7, 9, 3, False))).to(DEV))
    h = _roots_handler(16, 7, EVERY)
    kept = h.forest.z.clone()
    with pytest.raises(ValueError, match='7 objects.*at most 6'):
        h.run_mcts(crowded, 2, rollout_actions=np.zeros((2, 27, 6), dtype=np.int64))
    assert torch.equal(h.forest.z.cpu(), kept)
    wide = _Env(Dynamics(make_cfg(**C.cl_cfg(16, 3, 9, 5, False))).to(DEV))
    h = _roots_handler(16, 3, EVERY)
    with pytest.raises(ValueError, match='5 appearance columns.*at most 4'):
        h.run_mcts(wide, 2, rollout_actions=acts)
    # ops: a pool of one width with the images of another, and a pool of no width
    case = _named(16, 'counts-N3')
    z, app, acts16 = C.inputs(case)
    emb_w, emb_b, gnn, rh = _weights(_case_env(case, 'init'))
    args = (_i32(case.leaf), _i32(case.child), _i32(case.len_s), app.float().to(DEV), acts16.to(torch.int32).to(DEV), emb_w, emb_b, gnn, rh,
            case.D, 2, env16.dyn.use_elu, env16.dyn.loop_consts(), C.GAMMA)
    for width in (18, 34, 12):
        pool = torch.full((case.M, case.cap, case.N, width), NAN, device=DEV)
        before = pool.clone()
        with pytest.raises(ValueError, match='do not fit'):
            ops.plan_expand(pool, *args)
        torch.cuda.synchronize()
        assert torch.equal(_bits(pool), _bits(before))
    pool = _pool(z, case.leaf, case.cap)
    before = pool.clone()
    with pytest.raises(ValueError, match='do not fit'):
        ops.plan_expand(pool, *args[:8], rh[:-1].contiguous(), *args[9:])
    with pytest.raises(ValueError, match='do not fit'):
        ops.plan_expand(pool, *args[:7], torch.zeros(gnn.numel() + 1, device=DEV), *args[8:])
    torch.cuda.synchronize()
    assert torch.equal(_bits(pool), _bits(before))
    assert ops.plan_expand(pool, *args).shape == (case.M, case.A)                 # and the valid call still runs


# ------------------------------------------------------------------------------------------------ 9. the closed loop
def test_play_on_device_environments_at_cl_16():
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.mcts.play import play
    from stove_amd.video_prediction.stove import Stove
    torch.manual_seed(0)
    model16 = Stove(make_cfg(**CASES['ac3'], cl=16, transition_lik_std=[0.01] * 8)).to(DEV)
    np.random.seed(3)
    with pytest.raises(ValueError, match='state code length is 16'):
        play(model16, BatchedAvoidance([0, 3, 4], device=DEV), run_len=1, mcts_steps=4, max_rollout_depth=2, device_trees=True)
    out = play(model16, BatchedAvoidance([0, 3, 4], device=DEV), run_len=2, mcts_steps=4, max_rollout_depth=2, device_trees=True,
               fused_widths=EVERY)
    assert out['actions'].shape == (2, 3) and ((out['actions'] >= 0) & (out['actions'] < 9)).all()
