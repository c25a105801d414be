"""The input conditions of tests/test_gpu_plan_counts.py, asserted on the CPU for every case of tests/plan_cases.py (no case is skipped
or filtered: a condition that does not hold fails here): the 'spread' fill moves the rewards and the ReLU units, no ReLU pre-activation
lies where float32 could take the other branch, the value formula is the reference's, the search cases keep their decisions 1e-4 apart,
the case lists reach every trip-count edge of the kernels' loops, and the reference's own float32 run stays inside the caps the GPU
tests give it."""
import numpy as np
import pytest
import torch

import plan_cases as P
import stove_oracle as O
from gpu_helpers import err, err_l2, err_small

CASES = P.expansion_cases()


# ------------------------------------------------------------------------------------------------ the 'spread' fill
@pytest.mark.parametrize('case', CASES, ids=P.case_id)
def test_spread_moves_the_rewards_of_every_expansion_case(case):
    ok, fig = P.spread_conditions(*P.expansion_preacts(case, 'spread'))
    print('spread %s: k = %r, seed %d  %s' % (case.name, P.SPREAD_K[case.name], P.INPUT_SEEDS.get((case.name, 'spread'), 0), fig))
    assert fig['q90'] - fig['q10'] >= 0.1 and 0.02 < fig['min'] and fig['max'] < 0.98 and min(fig['use']) >= 0.25, fig
    assert ok


@pytest.mark.parametrize('s', P.SEARCH_CASES, ids=P.search_id)
def test_spread_moves_the_rewards_of_every_search_case(s):
    ok, fig = P.spread_conditions(*P.search_root_expansion(s))
    print('spread search %s: k = %r  %s' % (P.search_id(s), P.SEARCH_SPREAD_K[P.search_id(s)], fig))
    assert ok, fig


@pytest.mark.parametrize('N', range(1, 9))
def test_spread_moves_the_rewards_of_the_reward_head_cases(N):
    ok, fig = P.rh_spread_conditions(N)
    print('spread reward head N = %d: k = %r  %s' % (N, P.RH_SPREAD_K[N], fig))
    assert ok, fig


def test_the_saturated_fill_saturates():
    """some float32 rewards are exactly 1.0f or below 1e-7, and most items are not saturated (the gradients' scale is theirs)"""
    for items, N in P.RH_SHAPES:
        if items < 1000:
            continue
        r = P.rh_case_reference(items, N, 'saturated', 'drawn', torch.float32)['reward']
        sat = (r == 1.0) | (r < 1e-7)
        assert bool(sat.any()), (items, N)
        assert float(sat.float().mean()) < 0.9, (items, N)


# ------------------------------------------------------------------------------------------------ ReLU pre-activations
def _clear_of_zero(pre, what):
    for layer, p in enumerate(pre):
        m = float(p.abs().min() / p.abs().max())
        assert m > P.RELU_MARGIN, (what, layer, m)


@pytest.mark.parametrize('regime', P.REGIMES)
@pytest.mark.parametrize('case', CASES, ids=P.case_id)
def test_no_expansion_preactivation_near_zero(case, regime):
    """Every ReLU pre-activation of the reward head over all rows and steps keeps 1e-4 of its layer's largest away from zero."""
    _clear_of_zero(P.expansion_preacts(case, regime)[1], (case.name, regime))


@pytest.mark.parametrize('items,N', P.RH_SHAPES, ids=lambda v: str(v))
def test_no_reward_head_preactivation_near_zero(items, N):
    pred, _, passed = P.rh_inputs(items, N)
    assert pred.shape == (items, N, 32) and torch.equal(pred, pred.float().double())
    assert bool((pred.abs() == 30).any()) or items * N * 32 < 2
    for fill in P.RH_FILLS:
        _clear_of_zero(P.rh_preacts(P.rh_params(N, fill), pred), (items, N, fill))
    print('reward head inputs %d x %d: %d items passed over' % (items, N, passed))


def test_the_fixture_is_what_make_inputs_draws():
    """two small cases and the long rollout drawn again: the committed inputs are make_inputs' (and its margin is the tighter one)"""
    long, = [c for c in CASES if c.L > P.PILOT_STEPS]
    for case, regime in ((P.expansion_cases()[0], 'spread'), (P.expansion_cases()[12], 'init'), (long, 'analytic')):
        z, app, acts, _ = P.make_inputs(case, regime)
        zf, appf, actsf = P.load_inputs(case, regime)
        assert torch.equal(z.float().double(), zf) and torch.equal(acts, actsf)
        assert (app is None and appf is None) or torch.equal(app.float().double(), appf)


def test_rollout_preds_is_the_oracles_rollout():
    case = CASES[3]
    c, params = P.plan_oracle(case.N, case.A, case.app, case.elu, 'init')
    z, app, acts = P.load_inputs(case, 'init')
    zs, rew = P.oracle_rollout(c, params, z, app, acts, case.A)
    zs2, rew2, preds = P.rollout_preds(c, params, z.repeat_interleave(case.A, 0), P.one_hot_actions(acts, case.A, case.M).double(),
                                       app.repeat_interleave(case.A, 0))
    assert torch.equal(zs, zs2) and torch.equal(rew, rew2)
    assert torch.equal(O.reward_head(params, preds[:, 2])[:, 0], rew[:, 2])


def test_parameter_block_round_trip():
    params = P.rh_params(3, 'init')
    flat = P.rh_packed(params)
    assert flat.numel() == 2785
    back = P.rh_unpack(flat)
    assert all(torch.equal(back[k], params[k]) for k in P.RH_PACKED)
    k = P.RH_SPREAD_K[3]
    spread = P.rh_params(3, 'spread')
    for name in P.RH_PACKED:
        assert torch.equal(spread[name], params[name] * (k if name.endswith('.weight') else 1.0)), name


# ------------------------------------------------------------------------------------------------ the value formula
def test_value_formula():
    from stove_amd.mcts.mcts_stove import discounted_values
    g = np.random.default_rng(3)
    for M, A, L, D in ((3, 9, 5, 3), (2, 2, 70, 40), (3, 1, 1, 1), (4, 64, 2, 3)):
        rew = torch.from_numpy(g.uniform(0.05, 0.95, (M * A, 1 + L)))
        len_s = [1 + m % D for m in range(M)]
        q = P.value(rew, len_s, D, np.float64, M, A)
        r = rew.numpy().reshape(M, A, 1 + L)
        want = discounted_values(r[..., 0], r[..., 1:], len_s, D, P.GAMMA)
        assert np.abs(q - want).max() <= 1e-12
        for m in range(M):
            if len_s[m] == D:               # the empty discount sum: exactly the first term, whatever the rollout rewards
                assert np.array_equal(q[m], (r[m, :, 0] - 1.0) * P.GAMMA ** float(D))
            counted = min(2 * D - len_s[m] + 1, L)
            moved = rew.clone()
            moved[m * A:(m + 1) * A, 1 + counted:] = 0.5          # rewards past the clip do not count
            assert np.array_equal(P.value(moved, len_s, D, np.float64, M, A)[m], q[m])
    clipped = [c for c in CASES for m in range(c.M) if c.L < 2 * c.D - c.len_s[m] + 1]
    unclipped = [c for c in CASES for m in range(c.M) if c.L > 2 * c.D - c.len_s[m] + 1]
    assert clipped and unclipped


# ------------------------------------------------------------------------------------------------ the search cases
@pytest.mark.parametrize('s', P.SEARCH_CASES, ids=P.search_id)
def test_search_decisions_are_far_apart(s):
    f, leaves = P.search_on_oracle(s)
    print('search %s: seed %d, smallest decision gap %.3g; seeds passed over %s' % (P.search_id(s), s.seed, f.min_gap,
                                                                                  P.SEARCH_SEEDS_PASSED.get(P.search_id(s), [])))
    assert f.min_gap >= P.SEARCH_GAP
    assert leaves.shape == (s.R, s.M)
    assert s.seed not in P.SEARCH_SEEDS_PASSED.get(P.search_id(s), [])


def test_search_cases_are_the_issues():
    assert [tuple(s[:5]) for s in P.SEARCH_CASES] == [(1, 1, 2, 2, 6), (2, 64, 3, 2, 8), (6, 2, 70, 4, 16), (8, 9, 3, 5, 12)]
    blocks = {P.search_id(s): (s.M + 63) // 64 for s in P.SEARCH_CASES}                 # plan_tree_action_k: 64 trees per block
    assert blocks['N6-A2-M70-D4-R16'] == 2 and {s.A for s in P.SEARCH_CASES} >= {1, 64}


# ------------------------------------------------------------------------------------------------ geometry
def _one(prefix):
    case, = [c for c in CASES if c.name.startswith(prefix)]
    return case, P.geometry(case)


def test_every_trip_count_edge_is_hit_by_a_named_case():
    geo = {c.name: P.geometry(c) for c in CASES}
    assert {c.N for c in CASES} == set(range(1, 9))
    for n in range(1, 9):               # both nonlinearities are not asked of every count, ELU is
        assert any(c.elu for c in CASES if c.N == n), n
    # plan_finish_k's scatter loop over N 18 floats, 64 per trip
    assert {n: P.geometry(c)['scatter_trips'] for n in range(1, 9) for c in CASES if c.N == n} == {1: 1, 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 7: 2, 8: 3}
    # the row loops: a second trip from 1 025 rows on (256 blocks of four waves)
    for prefix, rows in (('limit-N2', 1088), ('limit-N5', 1088), ('rows-N3', 1026)):
        case, g = _one(prefix)
        assert g['rows'] == rows and g['blocks'] == 256 and g['row_trips'] == 2
    assert _one('rows-N3')[0].A == 9
    assert all(g['row_trips'] == 1 for name, g in geo.items() if g['rows'] <= 1024)
    trips = {items: -(-items // 1024) for items, _ in P.RH_SHAPES}
    assert trips[1024] == 1 and trips[1025] == 2 and trips[2049] == 3 and {n for items, n in P.RH_SHAPES if items == 1025} == set(range(1, 9))
    assert set(P.RH_ITEMS_N3) == {1, 3, 4, 5, 1023, 1024, 1025, 2049}
    # plan_prep_k
    assert {c.N for c in CASES if c.app == 0} >= {1, 4, 7}                                   # app == NULL
    assert {c.N for c in CASES if P.geometry(c)['sin_dim'] == 32} >= {3, 8}                  # the full input width
    assert {c.N for c in CASES if c.A == 1} == {2, 5} and {c.N for c in CASES if c.A == 2} >= {2, 5}
    case, g = _one('limit-N4-A64-app12')
    assert case.elu and g['AL'] == 320 and g['index_trips'] == 2 and g['embed_trips'] == 64 and g['sin_dim'] == 32
    assert _one('limit-N2')[1]['AL'] == 128
    case, g = _one('long-N2')
    assert case.L == 70 and case.D == 40 and g['nan_fill_trips'] == 2
    case, g = _one('onestep')
    assert case.L == 1 and case.D == 1 and case.len_s == (1, 1, 1)
    # the rollout behind the expansion: gnn.hip at one object and at seven and eight
    assert {c.N for c in CASES if not P.geometry(c)['gnn_small']} == {1, 7, 8}
    # slots: few actions at cap = 1 + A; the last legal slots, alone and together
    for c in CASES:
        assert c.cap >= 1 + c.A and all(0 <= lf < c.cap and 0 <= ch <= c.cap - c.A for lf, ch in zip(c.leaf, c.child))
        if c.name.startswith('few'):
            assert c.cap == 1 + c.A
    last = [c for c in CASES if c.cap - 1 in c.leaf and c.cap - c.A in c.child]
    assert len(last) >= 2
    assert len(CASES) == len({c.name for c in CASES})


# ------------------------------------------------------------------------------------------------ float32 gaps
def test_float32_gaps_of_the_expansion_stay_below_their_caps():
    worst = {}
    for case in CASES:
        for regime in P.REGIMES:
            ref, low = P.expansion_reference(case, regime), P.expansion_reference(case, regime, torch.float32)
            gaps = {'expand.z': err(low['z'], ref['z']), 'expand.r_first': err(low['r'][:, 0], ref['r'][:, 0]),
                    'expand.r_roll': err(low['r'][:, 1:], ref['r'][:, 1:]), 'expand.q': err(low['q'], ref['q'])}
            for k, v in gaps.items():
                if v > worst.get(k, (0, ''))[0]:
                    worst[k] = (v, case.name + '/' + regime)
    print('largest float32 gaps:', worst)
    for k, (v, where) in worst.items():
        assert v <= P.GAP_CAPS[k], (k, v, where)
        assert P.GAP_CAPS[k] <= 4 * v, (k, v, 'the cap is twice the largest gap measured; it was not measured on these cases')


def test_float32_gaps_of_the_reward_head_stay_below_their_caps():
    worst = {}
    for items, N in P.RH_SHAPES:
        for fill in P.rh_fills(items):
            for variant in ('drawn', 'third_zero'):
                ref, low = P.rh_case_reference(items, N, fill, variant), P.rh_case_reference(items, N, fill, variant, torch.float32)
                gaps = {'rh.' + k: err(low[k], ref[k]) for k in ('reward', 'H0', 'Q', 'A1', 'A2', 'd_pred')}
                for sfx, fn in (('', err), ('.l2', err_l2), ('.small', err_small)):
                    gaps['rh.grad' + sfx] = max(fn(low['grads'][n], ref['grads'][n]) for n in P.RH_PACKED)
                for k, v in gaps.items():
                    if v > worst.get(k, (0, ''))[0]:
                        worst[k] = (v, (items, N, fill, variant))
    print('largest float32 gaps:', worst)
    for k, (v, where) in worst.items():
        assert v <= P.GAP_CAPS[k], (k, v, where)
        assert P.GAP_CAPS[k] <= 4 * v, (k, v)
