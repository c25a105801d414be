"""CPU side of planning at the state-code lengths 16 and 64 (stove_plan_expand_cl, stove_plan_search_cl): the conditions on the cases
of tests/plan_cl_cases.py that tests/test_gpu_plan_cl.py relies on, the new entry points in header, library and binding table, their
argument checks under the sanitizers (tests/abi/plan_cl_validate_driver.cpp), and the handler's width switch on a stub model."""
import ctypes
import types

import numpy as np
import pytest
import torch

import control_harness
import plan_cl_cases as C

ENTRY_POINTS = {
    'stove_reward_head_param_floats_cl': ('size_t', 1),
    'stove_plan_expand_ws_bytes_cl': ('size_t', 6),
    'stove_plan_expand_cl': ('int', 29),
    'stove_plan_search_ws_bytes_cl': ('size_t', 6),
    'stove_plan_search_cl': ('int', 35),
}


# ------------------------------------------------------------------------------------------------ the cases
def test_the_case_list_covers_what_it_has_to():
    for cl in C.WIDTHS:
        cases = C.expansion_cases(cl)
        counts = [c for c in cases if '-counts-' in c.name]
        assert [c.N for c in counts] == list(range(1, C.MAX_OBJECTS + 1))
        assert {c.elu for c in counts} == {True, False}
        for c in counts:
            assert (c.A, c.app, c.M, c.L, c.D) == (9, 3, 3, 5, 3)
            tight = c.N in (1, C.MAX_OBJECTS)
            assert (max(c.leaf) == c.cap - 1 and max(c.child) == c.cap - c.A) == tight
        assert sorted(c.A for c in cases if '-few-' in c.name) == [1, 2]
        big, = [c for c in cases if c.A == 64]
        assert C.geometry(big)['rows'] == 1088 and C.geometry(big)['row_trips'] == 2
        assert any(c.app == 0 for c in cases)
        wide, = [c for c in cases if c.app == C.app_limit(cl)]
        assert C.geometry(wide)['sin_dim'] == cl
        assert any(c.L == 1 and c.D == 1 for c in cases)
        assert len({c.name for c in cases}) == len(cases) and all(c.name in C.SCALED for c in cases)
    assert C.app_limit(16) == 4 and C.app_limit(64) == 28


@pytest.mark.parametrize('case', C.all_cases(), ids=C.case_id)
def test_the_scaled_fill_spreads_the_rewards(case):
    """q90 - q10 >= 0.1 and every reward inside (0.02, 0.98), over all rows and steps on the float64 oracle; (k, seed, span) lie on the
    grid the search was given.  The fraction of ReLU units that change state is printed, not required (four units in the last hidden
    layer at cl = 16)."""
    k, seed, span = C.SCALED[case.name]
    assert k in C.K_GRID and seed in C.SEEDS and span in C.SPANS
    ok, fig = C.scaled_figures(case)
    print('%s: k %.4f seed %d span %.1f  q10 %.3f q90 %.3f min %.3f max %.3f  units in both states %s' % (
        case.name, k, seed, span, fig['q10'], fig['q90'], fig['min'], fig['max'], ' '.join('%.2f' % u for u in fig['use'])))
    assert ok, fig
    z, app, acts = C.inputs(case)
    assert tuple(z.shape) == (case.M, case.N, case.cl // 2 + 2) and tuple(acts.shape) == (case.M * case.A, case.L)
    assert float(z[..., :2].min()) >= 0.1 and float(z[..., :2].max()) <= 0.3 and float(z[..., 2:].abs().max()) <= span
    assert (app is None) == (case.app == 0)


@pytest.mark.parametrize('case', C.all_cases(), ids=C.case_id)
def test_the_float32_oracle_stays_close_to_the_float64_oracle(case):
    """per quantity (child state, r_first, r_roll, q) and fill, the float32 oracle's gap to the float64 oracle stays below
    BAR_PLAN / 6 = 5e-7: the bar the kernels are held to on the GPU is then BAR_PLAN.  Measured: 0.8 .. 3.7e-7 for the states, 0.3 ..
    2.4e-7 for the rewards, 0.3 .. 3.5e-7 for q.  Under the scaled fill this holds by selection as well: plan_cl_cases.search_scaled
    passes over a draw whose float32 gap under any capped fill is above 0.75 x the bar, so the committed draws keep a quarter of the bar
    in hand (the largest gap measured is 3.7e-7 against 5e-7) for a CPU whose float32 sums round differently.
    A deviation from BAR_PLAN / 6, in one place: the 'analytic' fill at cl = 16 (plan_cl_cases.gap_is_capped: saturated, rewards down
    to 1e-58; gaps of 0.7 .. 6.6e-6 in the states, up to 1.5e-5 in r_first, 1.1e-3 in the rollout's rewards, 3.1e-5 in q, whatever the
    span or seed of the inputs) cannot meet it.  Its gaps are held to the committed caps plan_cl_cases.GAP_CAPS_ANALYTIC16 instead, twice
    the largest gap measured, as plan_cases.GAP_CAPS are at cl = 32; the GPU test asserts the same caps before it forms 6 x the gap."""
    for fill in C.FILLS:
        gaps = C.float32_gaps(case, fill)
        print('%s %s: ' % (case.name, fill) + '  '.join('%s %.3g' % kv for kv in gaps.items()))
        for quantity, gap in gaps.items():
            cap = C.gap_cap(case, fill, quantity)
            assert gap < cap, (case.name, fill, quantity, gap, cap)
    assert C.GAP_BAR == C.BAR_PLAN / 6 and all(C.gap_is_capped(case, fill) for fill in ('init', 'scaled'))
    assert C.gap_is_capped(case, 'analytic') == (case.cl != 16)
    for fill in ('init', 'scaled'):
        assert all(C.gap_cap(case, fill, quantity) == C.GAP_BAR for quantity in ('z', 'r_first', 'r_roll', 'q'))


def test_the_caps_of_the_saturated_model_are_the_gaps_measured():
    """GAP_CAPS_ANALYTIC16 against the largest float32 gap per quantity over the twelve cl = 16 cases under the 'analytic' fill: every
    gap below its cap, and no cap above four times the largest gap (the caps are twice it: they were measured on these cases and do
    not leave the bar on the GPU, 6 x the gap, room to grow)"""
    worst = {}
    for case in C.expansion_cases(16):
        assert not C.gap_is_capped(case, 'analytic')
        for quantity, gap in C.float32_gaps(case, 'analytic').items():
            if gap > worst.get(quantity, (0, ''))[0]:
                worst[quantity] = (gap, case.name)
    print('largest float32 gaps, analytic fill at cl = 16:', worst)
    assert set(worst) == set(C.GAP_CAPS_ANALYTIC16)
    for quantity, (gap, where) in worst.items():
        assert gap <= C.GAP_CAPS_ANALYTIC16[quantity], (quantity, gap, where)
        assert C.GAP_CAPS_ANALYTIC16[quantity] <= 4 * gap, (quantity, gap, where)


@pytest.mark.parametrize('cl', C.WIDTHS)
@pytest.mark.parametrize('D,R', C.SEARCH_SHAPES)
def test_the_search_seeds_keep_the_decisions_apart(cl, D, R):
    s = C.search_case(cl, D, R)
    forest, leaves = C.search_on_oracle(s)
    print('%s: seed %d, smallest decision gap %.3g' % (C.search_id(s), s.seed, forest.min_gap))
    assert forest.min_gap >= C.SEARCH_GAP
    assert leaves.shape == (R, s.M)


# ------------------------------------------------------------------------------------------------ header, library, binding table
def test_the_new_entry_points_in_header_library_and_binding():
    from stove_amd import _lib, build
    build.build_library()
    raw = ctypes.CDLL(_lib.LIB_PATH)

    class Recorder:
        def __init__(self):
            self.bound = {}

        def __getattr__(self, name):
            return self.bound.setdefault(name, types.SimpleNamespace())
    rec = Recorder()
    _lib._declare(rec)
    for name, (ret, count) in ENTRY_POINTS.items():
        got_ret, params = control_harness.header_decl(name)
        assert got_ret == ret and len(params) == count, (name, got_ret, len(params))
        assert hasattr(raw, name), name
        assert name in rec.bound and len(rec.bound[name].argtypes) == count, name
        # the `_cl` convention: the cl = 32 call's parameters with `int cl` between the pointers and the first size
        base = control_harness.header_decl(name[:-3])[1]
        lead = next((k for k, p in enumerate(base) if '*' not in p), len(base))            # the leading pointers
        assert params == base[:lead] + ['int cl'] + base[lead:], name
    assert _lib.ABI_VERSION == 7 and _lib.load().stove_abi_version() == 7


def test_sizes_and_workspace_queries():
    from stove_amd import _lib
    lib = _lib.load()
    assert lib.stove_reward_head_param_floats_cl(16) == 721 == C.rh_floats(16)
    assert lib.stove_reward_head_param_floats_cl(64) == 10945 == C.rh_floats(64)
    assert lib.stove_reward_head_param_floats() == 2785 == C.rh_floats(32)
    assert lib.stove_reward_head_param_floats_cl(32) == 0 and lib.stove_reward_head_param_floats_cl(48) == 0
    for query in (lib.stove_plan_expand_ws_bytes_cl, lib.stove_plan_search_ws_bytes_cl):
        for cl in C.WIDTHS:
            assert query(cl, 3, 9, 4, 6, C.app_limit(cl)) > 0
            assert query(cl, 3, 9, 4, 1, 0) > 0
            assert query(cl, 3, 9, 4, 7, 3) == 0
            assert query(cl, 3, 9, 4, 3, C.app_limit(cl) + 1) == 0
            assert query(cl, 3, 65, 4, 3, 3) == 0
            assert query(cl, 1 << 20, 9, 1 << 20, 3, 3) == 0
        assert query(32, 3, 9, 4, 3, 3) == 0 and query(48, 3, 9, 4, 3, 3) == 0
    # the rollout's rows are what the workspace holds: states, extras, predicted states, pred, one flag per tree
    M, A, L, N, app = 3, 9, 5, 3, 3
    for cl in C.WIDTHS:
        rows, steps, zw = M * A, 1 + L, cl // 2 + 2
        least = 4 * (rows * N * zw + rows * steps * N * (4 + app) + rows * steps * N * zw + rows * steps * N * cl + M)
        got = lib.stove_plan_expand_ws_bytes_cl(cl, M, A, L, N, app)
        assert least <= got <= least + 5 * 64
        assert lib.stove_plan_search_ws_bytes_cl(cl, M, A, L, N, app) >= got + 4 * rows + 3 * 4 * M + 8 * M
    assert lib.stove_plan_expand_ws_bytes(M, A, L, N, app) > lib.stove_plan_expand_ws_bytes_cl(16, M, A, L, N, app)


def test_argument_checks_under_the_sanitizers(tmp_path_factory):
    """the width-aware checks of csrc/validate.h compiled host-only with -fsanitize=address,undefined and driven by a stand-alone
    program (tests/abi/plan_cl_validate_driver.cpp): every case returns the documented code, nothing is dereferenced"""
    control_harness.run_modes(control_harness.build_driver(tmp_path_factory, 'plan_cl_validate_driver'), ['validate'])


# ------------------------------------------------------------------------------------------------ the handler's switch
def _stub(cl, num_obj=3, app_dim=3, core_app=True, cuda=True, dtype=torch.float32):
    """what _fused_unserved looks at: the configuration and the first parameter's device and dtype"""
    c = types.SimpleNamespace(cl=cl, num_obj=num_obj, debug_core_appearance=core_app, debug_appearance_dim=app_dim, action_conditioned=True)
    p = types.SimpleNamespace(is_cuda=cuda, dtype=dtype)
    return types.SimpleNamespace(c=c, parameters=lambda: iter([p]))


def test_the_width_switch_on_a_stub_model():
    from stove_amd.mcts import mcts_stove
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    assert mcts_stove.FUSED_WIDTHS == (32,) and mcts_stove.FUSED_WHERE_ELIGIBLE is False
    unserved = BatchedMCTSHandler._fused_unserved
    z = torch.zeros(1, 3, 10)
    h = BatchedMCTSHandler([MCTS(None, z, max_rollout_depth=2)], None, action_space=9, max_rollout_depth=2)
    assert h.fused_widths == (32,) and h.device_trees is False
    # the default: today's answers
    assert unserved(_stub(32)) == '' and unserved(_stub(32), h.fused_widths) == ''
    for cl in (16, 64):
        assert unserved(_stub(cl)) == 'its state code length is %d, not 32' % cl
        assert unserved(_stub(cl), h.fused_widths) == 'its state code length is %d, not 32' % cl
    assert unserved(_stub(16, cuda=False), (16, 32, 64)) == 'it is not on the GPU'
    assert 'float64' in unserved(_stub(16, dtype=torch.float64), (16, 32, 64))
    # switched on
    every = (16, 32, 64)
    for cl in every:
        assert unserved(_stub(cl), every) == ''
    assert unserved(_stub(16, num_obj=6, app_dim=4), every) == '' and unserved(_stub(64, num_obj=6, app_dim=28), every) == ''
    assert unserved(_stub(64, app_dim=99, core_app=False), every) == ''          # appearance that does not reach the core
    for cl, limit in ((16, 4), (64, 28)):
        why = unserved(_stub(cl, num_obj=7), every)
        assert '7 objects' in why and 'at most 6' in why, why
        why = unserved(_stub(cl, app_dim=limit + 1), every)
        assert '%d appearance columns' % (limit + 1) in why and 'at most %d' % limit in why, why
    assert unserved(_stub(48), every).startswith('its state code length is 48')
    assert unserved(_stub(32), (16, 64)) == 'its state code length is 32, not 16 or 64'
    assert unserved(_stub(16), (32, 64)) == 'its state code length is 16, not 32 or 64'
    # the keyword reaches the handler; run_mcts and run_mcts_model keep their parameter lists
    import inspect
    from stove_amd.mcts.play import play
    for fn in (mcts_stove.plan_on_model, mcts_stove.plan_on_frames, play):
        assert inspect.signature(fn).parameters['fused_widths'].default is None
    assert list(inspect.signature(BatchedMCTSHandler.run_mcts).parameters) == ['self', 'env', 'runs_per_round', 'fused', 'rollout_actions']
    assert list(inspect.signature(mcts_stove.run_mcts_model).parameters) == ['img', 'model', 'actions', 'num_parallel_envs', 'mcts_steps',
                                                                             'max_rollout_depth']


def test_the_handlers_limits_are_the_librarys():
    """mcts_stove._FUSED_LIMITS (what _fused_unserved names in its refusals) against the library's own answers: per width, the largest
    object count and the largest app_dim whose workspace query is not 0 (csrc/validate.h: plan_dims_bad)"""
    from stove_amd import _lib
    from stove_amd.mcts import mcts_stove
    lib = _lib.load()
    assert set(mcts_stove._FUSED_LIMITS) == {16, 32, 64}
    for cl, (max_obj, max_app) in mcts_stove._FUSED_LIMITS.items():
        for query in (lib.stove_plan_expand_ws_bytes, lib.stove_plan_search_ws_bytes) if cl == 32 else \
                (lambda *a, q=lib.stove_plan_expand_ws_bytes_cl, cl=cl: q(cl, *a), lambda *a, q=lib.stove_plan_search_ws_bytes_cl, cl=cl: q(cl, *a)):
            assert [n for n in range(1, 17) if query(3, 9, 4, n, 0) > 0] == list(range(1, max_obj + 1)), cl
            assert [a for a in range(0, 65) if query(3, 9, 4, max_obj, a) > 0] == list(range(0, max_app + 1)), cl
            assert [a for a in range(0, 65) if query(3, 9, 4, 1, a) > 0] == list(range(0, max_app + 1)), cl


def test_ops_refuses_other_widths_before_anything_else():
    """a pool whose last dimension is no cl/2 + 2 of a served width never reaches the library"""
    from stove_amd import ops
    for width, cl in ((10, 16), (18, 32), (34, 64)):
        assert ops._plan_width(torch.zeros(1, 2, 3, width)).cl == cl
    for width in (9, 17, 26, 66):
        assert ops._plan_width(torch.zeros(1, 2, 3, width)) is None
    assert ops._plan_width(torch.zeros(2, 3, 18)) is None
    assert np.isclose(C.GAMMA, 0.95)
