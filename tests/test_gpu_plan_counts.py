"""The planning kernels against float64 references at every object and action count their entry points accept, and at the trip-count
edges of their loops (tests/plan_cases.py holds the cases, inputs and references; tests/test_plan_cases_cpu.py the conditions on them):

a. the reward head through the C ABI (stove_reward_head_fwd / _bwd, csrc/reward_head.hip) between guard bands, every output pre-filled
   with NaN, every call made twice: 1 .. 2 049 items, 1 .. 8 objects, the 'init', 'spread' and a saturated fill, three upstream gradients;
b. ops.plan_expand (stove_plan_expand, csrc/plan.hip) against O.rollout and the value formula: N = 1 .. 8, A = 1 .. 64, app_dim = 0 .. 12,
   up to 1 088 rows, L up to 70, under the 'analytic', 'init' and 'spread' fills; child states bit for bit against Stove.rollout;
   poisoned trees; refusals of the C entry;
c. ops.plan_search (stove_plan_search, csrc/plan_tree.hip) against the host forest on the same expansion kernel, 'spread' weights.

Bars: what each quantity holds elsewhere (plan_cases.BAR_*), or 6 x the reference's own float32-vs-float64 gap on the same inputs where
that is larger (gpu_helpers.regime_bar); every gap is measured here on the CPU and must stay below its cap (plan_cases.GAP_CAPS).
Achieved errors: profiles/plan_counts_parity.json."""
import functools

import numpy as np
import pytest
import torch

import plan_cases as P
from control_harness import guarded, margins_intact
from gpu_helpers import check_ratio, err, err_l2, err_small, regime_bar
from test_gpu_dynamics import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
INVALID = 1          # hipErrorInvalidValue
GUARD = 1024         # floats: 4 KiB in front of and behind every buffer of the reward-head calls


def _lib():
    from stove_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _held(key, quantity, got, want, low, bar, fn=err):
    """check `got` against the float64 reference `want` at regime_bar(bar, gap), gap = what the reference's float32 run `low` differs
    from `want` by -- which must stay below the cap the CPU test asserts"""
    e, gap = fn(got, want), fn(low, want)
    assert gap <= P.GAP_CAPS[quantity], (key, quantity, gap)
    check_ratio('plan_counts.' + key + '.' + quantity.split('.', 1)[1], e, regime_bar(bar, gap))
    return e, gap


# ------------------------------------------------------------------------------------------------ a. the reward head, C ABI
def _nan(n):
    return guarded(torch.full((n,), NAN), NAN, GUARD)


def _rh_forward(lib, p, stream, pred, flat, items, N):
    reward, reward_buf = _nan(items)
    saved, saved_buf = _nan(lib.stove_reward_head_saved_floats(items, N))
    assert lib.stove_reward_head_fwd(p(pred), p(flat), p(reward), p(saved), items, N, stream()) == 0
    torch.cuda.synchronize()
    margins_intact({'reward': reward_buf, 'saved': saved_buf}, GUARD)
    assert not torch.isnan(reward).any() and not torch.isnan(saved).any(), 'elements the kernel did not write'
    return reward, saved


def _rh_backward(lib, p, stream, pred, flat, reward, saved, d_reward, items, N):
    d_pred, d_pred_buf = _nan(items * N * 32)
    g, g_buf = _nan(lib.stove_reward_head_param_floats())
    ws, ws_buf = _nan(lib.stove_reward_head_bwd_ws_floats(items))
    assert lib.stove_reward_head_bwd(p(pred), p(flat), p(reward), p(saved), p(d_reward), p(d_pred), p(g), p(ws), items, N, stream()) == 0
    torch.cuda.synchronize()
    margins_intact({'d_pred': d_pred_buf, 'g': g_buf, 'ws': ws_buf}, GUARD)
    assert not torch.isnan(d_pred).any() and not torch.isnan(g).any(), 'elements the kernel did not write'
    return d_pred, g


@pytest.mark.parametrize('items,N', P.RH_SHAPES, ids=lambda v: str(v))
def test_reward_head_against_the_restatement(items, N):
    lib, p, stream = _lib()
    assert lib.stove_reward_head_param_floats() == 2785
    x = P.rh_inputs(items, N)[0]
    pred = x.float().to(DEV).contiguous()
    for fill in P.rh_fills(items):
        key = 'reward_head.i%d-n%d-%s' % (items, N, fill)
        flat = P.rh_packed(P.rh_params(N, fill)).float().to(DEV).contiguous()
        reward, saved = _rh_forward(lib, p, stream, pred, flat, items, N)
        again = _rh_forward(lib, p, stream, pred, flat, items, N)
        assert torch.equal(_bits(reward), _bits(again[0])) and torch.equal(_bits(saved), _bits(again[1]))
        ref, low = P.rh_case_reference(items, N, fill, 'drawn'), P.rh_case_reference(items, N, fill, 'drawn', torch.float32)
        cuts = np.cumsum([0, items * N * 32, items * 32, items * 16, items * 8])
        got = {'reward': reward, **{k: saved[a:b].view(ref[k].shape) for k, a, b in zip(('H0', 'Q', 'A1', 'A2'), cuts[:-1], cuts[1:])}}
        for k, v in got.items():
            _held(key, 'rh.' + k, v, ref[k], low[k], P.BAR_VALUE)
        for variant in P.RH_GRADS:
            d = P.rh_d_reward(items, N, variant).float().to(DEV)
            d_pred, g = _rh_backward(lib, p, stream, pred, flat, reward, saved, d, items, N)
            again = _rh_backward(lib, p, stream, pred, flat, reward, saved, d, items, N)
            assert torch.equal(_bits(d_pred), _bits(again[0])) and torch.equal(_bits(g), _bits(again[1]))
            if variant == 'zero':
                assert bool((d_pred == 0).all()) and bool((g == 0).all())
                continue
            ref, low = P.rh_case_reference(items, N, fill, variant), P.rh_case_reference(items, N, fill, variant, torch.float32)
            kv = key + '-' + variant
            _held(kv, 'rh.d_pred', d_pred.view(items, N, 32), ref['d_pred'], low['d_pred'], P.BAR_GRAD[0])
            grads = P.rh_unpack(g)
            for sfx, fn, bar in zip(('', '.l2', '.small'), (err, err_l2, err_small), P.BAR_GRAD):
                for name in P.RH_PACKED:
                    _held(kv, 'rh.grad' + sfx, grads[name], ref['grads'][name], low['grads'][name], bar, fn)


def test_reward_head_empty_call():
    """items = 0: g_params comes back zeroed and nothing else is touched"""
    lib, p, stream = _lib()
    bufs = {k: _nan(n) for k, n in (('pred', 96), ('reward', 1), ('saved', 184), ('d_reward', 1), ('d_pred', 96), ('g', 2785), ('ws', 2785 * 4))}
    flat = P.rh_packed(P.rh_params(3, 'init')).float().to(DEV).contiguous()
    v = {k: b[0] for k, b in bufs.items()}
    assert lib.stove_reward_head_fwd(p(v['pred']), p(flat), p(v['reward']), p(v['saved']), 0, 3, stream()) == 0
    assert lib.stove_reward_head_bwd(p(v['pred']), p(flat), p(v['reward']), p(v['saved']), p(v['d_reward']), p(v['d_pred']), p(v['g']), p(v['ws']),
                                     0, 3, stream()) == 0
    torch.cuda.synchronize()
    assert bool((v['g'] == 0).all()) and not bool(torch.signbit(v['g']).any())
    for k, (view, buf) in bufs.items():
        if k != 'g':
            assert bool(torch.isnan(buf).all()), k
    margins_intact({'g': bufs['g'][1]}, GUARD)


# ------------------------------------------------------------------------------------------------ b. the expansion
class _Env(torch.nn.Module):
    """the part of a Stove that planning uses: the dynamics module and Stove.rollout on it (the method itself, not a restatement)"""

    def __init__(self, dyn):
        super().__init__()
        self.dyn, self.c, self.noise_fn = dyn, dyn.c, None

    def rollout(self, *args, **kw):
        from stove_amd.video_prediction.stove import Stove
        return Stove.rollout(self, *args, **kw)


@functools.lru_cache(maxsize=None)
def _env(N, A, app, elu, regime):
    from stove_amd.video_prediction.dynamics import Dynamics
    return _Env(P.fill_module(Dynamics(make_cfg(**P.plan_cfg(N, A, app, elu))), 'dyn.', regime).to(DEV))


def _weights(env):
    from stove_amd.mcts.mcts_stove import BatchedMCTSHandler
    return BatchedMCTSHandler._fused_weights(env)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _pool(z, leaf, cap):
    """NaN everywhere but the leaf slots"""
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
    q, rf, rr = ops.plan_expand(pool, _i32(leaf), _i32(child), _i32(len_s), app.float().to(DEV) if app is not None else None,
                                acts.to(torch.int32).to(DEV), emb_w, emb_b, gnn, rh, case.D, 2, env.dyn.use_elu, env.dyn.loop_consts(), P.GAMMA,
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


@pytest.mark.parametrize('regime', P.REGIMES)
@pytest.mark.parametrize('case', P.expansion_cases(), ids=P.case_id)
def test_plan_expand_against_the_oracle(case, regime):
    """child states, r_first, r_roll and q against O.rollout + the value formula in float64 at 3e-6 (the bars of tests/test_gpu_plan.py)
    or 6 x the float32 oracle's gap; the pool outside the child slots untouched bit for bit; two runs bit-equal; child states =
    Stove.rollout(num = 1) bit for bit"""
    env = _env(case.N, case.A, case.app, case.elu, P.case_regime(case, regime))
    z, app, acts = P.load_inputs(case, regime)
    before, pool, q, rf, rr = _expand(env, case, z, app, acts)
    again = _expand(env, case, z, app, acts)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((pool, q, rf, rr), again[1:]))
    written = _written(case)
    assert bool((_bits(pool) == _bits(before))[~written].all()), 'a slot outside the child ranges was written'
    assert bool(torch.isfinite(pool[written]).all())
    kids = _kids(pool, case)
    with torch.no_grad():
        first = P.one_hot_actions(acts, case.A, case.M)[:, :1].float().to(DEV)
        want, _ = env.rollout(z.float().repeat_interleave(case.A, 0).to(DEV), num=1, actions=first,
                              appearance=app.float().repeat_interleave(case.A, 0).to(DEV) if app is not None else None)
    assert torch.equal(_bits(kids), _bits(want[:, 0])), 'child states differ from Stove.rollout(num = 1)'
    ref, low = P.expansion_reference(case, regime), P.expansion_reference(case, regime, torch.float32)
    key = 'expand.%s-%s' % (case.name, regime)
    out = [_held(key, 'expand.z', kids, ref['z'], low['z'], P.BAR_PLAN),
           _held(key, 'expand.r_first', rf.flatten(), ref['r'][:, 0], low['r'][:, 0], P.BAR_PLAN),
           _held(key, 'expand.r_roll', rr.flatten(0, 1), ref['r'][:, 1:], low['r'][:, 1:], P.BAR_PLAN),
           _held(key, 'expand.q', q, ref['q'], low['q'], P.BAR_PLAN)]
    print(key + ': ' + '  '.join('%s %.3g (f32 gap %.3g)' % (k, e, g) for k, (e, g) in zip(('z', 'r_first', 'r_roll', 'q'), out)))
    for m in range(case.M):
        if case.len_s[m] == case.D:                    # the empty discount sum: exactly the first term
            want_q = (rf[m] - 1.0) * torch.tensor(P.GAMMA, device=DEV) ** case.D
            assert float(((q[m] - want_q).abs() / want_q.abs()).max()) < 1e-6


def _poisoned(case, regime, tree, **bad):
    """the case with one tree poisoned: that tree all NaN and no slot written, the others bit-equal to the clean run"""
    env = _env(case.N, case.A, case.app, case.elu, P.case_regime(case, regime))
    z, app, acts = P.load_inputs(case, regime)
    _, pool_ok, q_ok, rf_ok, rr_ok = _expand(env, case, z, app, acts)
    assert bool(torch.isfinite(q_ok).all())
    before, pool, q, rf, rr = _expand(env, case, z, app, bad.pop('acts', acts), **bad)
    for m in range(case.M):
        if m == tree:
            assert bool(torch.isnan(q[m]).all()) and bool(torch.isnan(rf[m]).all()) and bool(torch.isnan(rr[m]).all())
            assert torch.equal(_bits(pool[m]), _bits(before[m]))
        else:
            assert torch.equal(_bits(q[m]), _bits(q_ok[m])) and torch.equal(_bits(rf[m]), _bits(rf_ok[m])) and torch.equal(_bits(rr[m]), _bits(rr_ok[m]))
            assert torch.equal(_bits(pool[m]), _bits(pool_ok[m]))


def _named(prefix):
    case, = [c for c in P.expansion_cases() if c.name.startswith(prefix)]
    return case


def test_the_last_of_320_actions_poisons_its_tree():
    """A = 64, L = 5: the one bad action is the last of tree 0's A L = 320, behind the first 256-thread trip of the index check"""
    case = _named('limit-N4-A64-app12')
    assert case.A * case.L == 320
    acts = P.load_inputs(case, 'init')[2].clone()
    acts[case.A - 1, case.L - 1] = case.A
    _poisoned(case, 'init', 0, acts=acts)


def test_a_poisoned_tree_at_seventy_steps():
    """L = 70: the NaN fill of r_roll takes a second trip of its 64-lane loop"""
    case = _named('long-N2-A2')
    assert case.L == 70 and case.M == 2
    len_s = list(case.len_s)
    len_s[1] = case.D + 1
    _poisoned(case, 'spread', 1, len_s=len_s)


def test_plan_expand_c_entry_and_refusals():
    """the C entry at N = 8, app_dim = 12 with workspace of exactly the queried size: app_dim = 13, A = 65, N = 9 and cap = A are refused
    with the outputs untouched, the valid call equals ops.plan_expand bit for bit"""
    lib, p, stream = _lib()
    case, regime = _named('wide-N8'), 'init'
    env = _env(case.N, case.A, case.app, case.elu, regime)
    z, app, acts = P.load_inputs(case, regime)
    _, pool_ok, q_ok, rf_ok, rr_ok = _expand(env, case, z, app, acts)
    emb_w, emb_b, gnn, rh = _weights(env)
    pool = _pool(z, case.leaf, case.cap)
    before = pool.clone()
    M, A, L, N = case.M, case.A, case.L, case.N
    leaf, child, len_s, appd, actsd = _i32(case.leaf), _i32(case.child), _i32(case.len_s), app.float().to(DEV), acts.to(torch.int32).to(DEV)
    q, rf, rr = (torch.full(s, 7.0, device=DEV) for s in ((M, A), (M, A), (M, A, L)))
    nbytes = lib.stove_plan_expand_ws_bytes(M, A, L, N, case.app)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, ws_buf = guarded(torch.zeros(nbytes // 4), NAN, GUARD)
    dims = dict(M=M, cap=case.cap, A=A, L=L, D=case.D, N=N, app_dim=case.app)

    def call(**change):
        d = dict(dims, **change)
        return lib.stove_plan_expand(p(pool), p(leaf), p(child), p(len_s), p(appd), p(actsd), p(emb_w), p(emb_b), p(gnn), p(rh), p(q), p(rf), p(rr),
                                     p(ws), *d.values(), 2, int(env.dyn.use_elu), *[float(c) for c in env.dyn.loop_consts()], P.GAMMA, stream())
    for change in (dict(app_dim=13), dict(A=65), dict(N=9), dict(cap=A)):
        assert call(**change) == INVALID, change
    assert lib.stove_plan_expand_ws_bytes(M, A, L, N, 13) == 0 and lib.stove_plan_expand_ws_bytes(M, 65, L, N, case.app) == 0
    torch.cuda.synchronize()
    assert float(q.min()) == 7.0 and float(rf.min()) == 7.0 and float(rr.min()) == 7.0
    assert torch.equal(_bits(pool), _bits(before))
    assert call() == 0
    torch.cuda.synchronize()
    margins_intact({'ws': ws_buf}, GUARD)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((pool, q, rf, rr), (pool_ok, q_ok, rf_ok, rr_ok)))


# ------------------------------------------------------------------------------------------------ c. the search
MIN_GAP = 1e-9


@pytest.mark.parametrize('s', P.SEARCH_CASES, ids=P.search_id)
def test_device_search_equals_host_search(s):
    """ops.plan_search against the host forest searching on ops.plan_expand, 'spread' weights: the same leaf per iteration, integer
    arrays equal, Qsa and the pool bit for bit, all statuses 0 (tests/test_gpu_plan_search.py's comparison at other counts).  The
    seeds keep every decision of the float64 oracle's search 1e-4 apart (tests/test_plan_cases_cpu.py); here the host forest's and
    every device tree's smallest gap must be >= 1e-9, far above what one ulp of `log` moves a UCT value by."""
    from stove_amd import ops
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler, Forest
    from test_gpu_plan_search import _same_as_forest
    env = _env(s.N, s.A, s.app, False, ('scaled', P.SEARCH_SPREAD_K[P.search_id(s)]))
    z, app, acts = P.search_inputs(s)
    z, app = z.float(), app.float()
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=s.A, max_rollout_depth=s.D) for m in range(s.M)]
    h = BatchedMCTSHandler(trees, app, action_space=s.A, max_rollout_depth=s.D)
    leaves, select = [], h.forest.select

    def recording_select():
        leaf = select()
        leaves.append(leaf.copy())
        return leaf
    h.forest.select = recording_select
    act_h = h.run_mcts(env, s.R, fused=True, rollout_actions=acts)
    assert h.forest.min_gap >= MIN_GAP, h.forest.min_gap
    cap = h.forest.cap
    f = Forest(s.M, s.A, s.D, cap=cap)
    pool = torch.zeros(s.M, cap, s.N, 18)
    pool[:, 0] = z
    pool = pool.to(DEV)
    arrays = f.to_device(DEV)
    sel = torch.full((s.R, s.M), -5, dtype=torch.int32, device=DEV)
    emb_w, emb_b, gnn, rh = _weights(env)
    with torch.no_grad():
        action = ops.plan_search(pool, arrays, app.to(DEV), torch.from_numpy(acts.astype(np.int32)).to(DEV), emb_w, emb_b, gnn, rh, s.D, 2,
                                 env.dyn.use_elu, env.dyn.loop_consts(), P.GAMMA, sel_trace=sel)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in arrays.items()}
    assert not out['status'].any()
    assert np.array_equal(sel.cpu().numpy(), np.stack(leaves))
    _same_as_forest(out, h.forest, pool=pool)
    assert action.cpu().tolist() == act_h
    assert (out['min_gap'] >= MIN_GAP).all(), out['min_gap']
    assert float(out['min_gap'].min()) == h.forest.min_gap or abs(float(out['min_gap'].min()) - h.forest.min_gap) <= 1e-12       # (inf at A = 1)
    print('plan_search %s: smallest gap host %.3g, per tree on the device >= %.3g; actions %s' % (P.search_id(s), h.forest.min_gap,
                                                                                                 float(out['min_gap'].min()), act_h[:8]))
