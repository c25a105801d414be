"""The float64 restatement of the state pipeline, the z assembly and the ELBO (helpers.state_chain / zall_chain / elbo_chain) that
tests/test_gpu_state_counts.py holds csrc/state.hip to -- pinned here, without a GPU, to the reference's recorded results (the g6
fixtures), to a symmetry the chain must have, and to the input conditions its cases state: no |jump| of the matched track within
1e-4 of fix_supair's 0.095 threshold, every matcher decision won by more than 1e-5 -- for EVERY case of the grid, by the seeded choice
of the inputs (helpers.state_inputs), none left out."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from helpers import (FIX_CLEARANCE, FIX_THRESHOLD, STATE_COUNTS, STATE_IDX_FORMS, STATE_SHAPES, assert_state_conditions,
                     assert_state_coverage, draw_codes, elbo_chain, elbo_inputs, gather_slots, given_idx_inputs, load_golden, match_walk,
                     state_case_id, state_cases, state_chain, state_config, state_coverage, state_inputs, state_last_stage,
                     state_reference, state_span_low, t_, zall_chain)

CASES = state_cases()


def test_grid_holds_every_count_shape_mode_and_both_fix_settings():
    assert len(CASES) == len(set(CASES)) == 2 * 8 * 8 + 8
    assert {c[0] for c in CASES} == set(STATE_COUNTS) == set(range(1, 9)) and {c[1:4] for c in CASES} == set(STATE_SHAPES)
    assert all(c[4] != '3_only' or c[0] == 3 for c in CASES)
    for o in STATE_COUNTS:
        for mode in ('greedy', 'volatile'):
            assert {c[1:4] for c in CASES if c[0] == o and c[4] == mode} == set(STATE_SHAPES)
        assert {c[5] for c in CASES if c[0] == o} == {True, False}
    for shape in STATE_SHAPES:
        assert {c[5] for c in CASES if c[1:4] == shape} == {True, False}
    assert {c[5] for c in CASES if c[4] == '3_only'} == {True, False}


def test_last_stage_reproduces_the_reference_fix_supair_fixture():
    g = load_golden('g6_fix_supair')
    z, zs, zf = t_(g['z']), t_(g['zstd']), t_(g['z_fixed'])
    out = state_last_stage(torch.cat([z, zs], -1), 2, True)
    assert torch.equal(out['zfix'][..., :4], zf) and torch.equal(out['zfix'][..., 4:], t_(g['zstd_fixed']))
    # the two-bit mask: bit a = dims a, a + 2, ... were replaced
    for a in (0, 1):
        fired = (zf[..., a::2] != z[..., a::2]).any(-1)
        assert torch.equal((out['hits'] >> a & 1).bool(), fired)
    assert int((out['hits'] > 0).sum()) >= 2
    full = O.v_from_state(zf)
    assert torch.equal(out['zl'], full[:, 2:]) and torch.equal(out['init'], full[:, 1])
    off = state_last_stage(torch.cat([z, zs], -1), 2, False)
    assert torch.equal(off['zfix'][..., :4], z) and not off['hits'].any()


@pytest.mark.parametrize('mode,name', [('3_only', 'g6_match_3only'), ('greedy', 'g6_match_greedy'), ('volatile', 'g6_match_volatile')])
def test_match_walk_reproduces_the_reference_match_fixtures(mode, name):
    g = load_golden(name)
    z = t_(g['z'])
    idx, _ = match_walk(z[..., 2:4], mode)
    want = g['idx'] if 'idx' in g else g['perm'].argmax(-1)
    assert np.array_equal(idx.numpy(), want)
    assert float((gather_slots(z, idx) - t_(g['z_matched'])).abs().max()) < 1e-15
    assert torch.equal(gather_slots(t_(g['zstd']), idx), t_(g['zstd_matched']))


def test_match_walk_margins_are_the_decisions_margins():
    """two slots, one frame pair, by hand: slots at x = 0 and 0.5, current objects at x = 0.1 and 0.45 (features (x + 1) / 2)"""
    pos = torch.tensor([[[[0.0, 0.0], [0.5, 0.0]], [[0.1, 0.0], [0.45, 0.0]]]], dtype=torch.float64)
    e = lambda a, b: ((a - b) / 2) ** 2          # noqa: E731
    idx, m = match_walk(pos, 'volatile')
    assert idx[0, 1].tolist() == [0, 1]
    assert abs(float(m) - min(e(0, .45) - e(0, .1), e(.5, .1) - e(.5, .45))) < 1e-15
    idx, m = match_walk(pos, 'greedy')
    assert idx[0, 1].tolist() == [0, 1] and abs(float(m) - (e(0, .1) - e(.5, .45))) < 1e-15      # smallest entry against the second smallest


@pytest.mark.parametrize('case', CASES, ids=state_case_id)
def test_input_conditions_hold(case):
    """the stated conditions on the float64 reference of every case; the inputs are float32 values; with the stencil off nothing is
    replaced; the chain's hit mask says where fix_supair replaced something"""
    o, n, T, skip, mode, fix = case
    codes = state_inputs(case)
    assert codes.shape == (n, T, o, 8) and torch.equal(codes, codes.float().double())
    ref = state_reference(case)
    assert_state_conditions(ref, mode)
    zm = gather_slots(ref['zc'], ref['idx'])
    changed = (ref['zfix'] - zm).abs() > 1e-12          # (the matchers hand the means through (z + 1) / 2 and back: one rounding)
    assert torch.equal(changed.any(-1), ref['hits'] > 0) if fix else not changed.any()
    assert not ref['hits'][:, 0].any() and not ref['hits'][:, -1].any()
    if skip == 1:
        assert not ref['init'].any()                       # the zero row of v_from_state


def test_grid_coverage():
    assert_state_coverage(state_coverage(CASES))


@pytest.mark.parametrize('o', STATE_COUNTS)
def test_chain_is_equivariant_under_a_permutation_of_frame_zero(o):
    """'greedy': listing the objects of frame 0 in another order relabels the slots and changes nothing else"""
    case = next(c for c in CASES if c[0] == o and c[1:5] == (6, 11, 2, 'greedy'))
    _, n, T, skip, mode, _ = case
    codes = state_inputs(case)
    p = torch.randperm(o, generator=torch.Generator().manual_seed(o))
    moved = codes.clone()
    moved[:, 0] = codes[:, 0, p]
    c = state_config(o, skip)
    noise = torch.randn(n, o, 12, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a = state_chain(c, codes.reshape(-1, 8), n, T, o, skip, True, mode, noise)
    b = state_chain(c, moved.reshape(-1, 8), n, T, o, skip, True, mode, noise[:, p])
    for k in ('zfix', 'hits', 'zl', 'sl'):
        assert torch.equal(b[k], a[k][:, :, p]), k
    assert torch.equal(b['init'], a['init'][:, p])
    assert torch.equal(b['idx'][:, 1:], a['idx'][:, 1:, p]) and torch.equal(b['idx'][:, 0], torch.argsort(p)[a['idx'][:, 0, p]])


@pytest.mark.parametrize('form', STATE_IDX_FORMS)
@pytest.mark.parametrize('o', STATE_COUNTS)
def test_given_matchings(o, form):
    if form == 'volatile' and o == 1:
        with pytest.raises(AssertionError):
            given_idx_inputs(o, 2, 5, form, 0)
        return
    zc, idx = given_idx_inputs(o, 4, 9, form, 5000 + o)
    assert zc.shape == (4, 9, o, 8) and idx.shape == (4, 9, o) and idx.dtype == torch.int64 and torch.equal(zc, zc.float().double())
    srt = idx.sort(-1).values
    if form == 'volatile':          # every frame: one object twice, one never
        assert bool((srt[..., 1:] == srt[..., :-1]).any(-1).all()) and bool((srt != torch.arange(o)).any(-1).all())
    else:
        assert torch.equal(srt, torch.arange(o).expand_as(srt))
        assert (form == 'identity') == torch.equal(idx, torch.arange(o).expand_as(idx)) or o == 1
    jump = state_last_stage(gather_slots(zc, idx), 2, True)['jump']
    assert float((jump - FIX_THRESHOLD).abs().min()) > FIX_CLEARANCE


def test_span_low_and_constrain_zp_agree():
    c = state_config(3)
    sl = torch.tensor(state_span_low(c), dtype=torch.float64)
    codes = draw_codes(torch.Generator().manual_seed(0), 2, 3, 3).reshape(-1, 8)
    mean, std = O.constrain_zp(c, codes)
    assert float((torch.cat([mean, std], -1) - (sl[8:] + sl[:8] * torch.sigmoid(codes))).abs().max()) < 1e-15


@pytest.mark.parametrize('skip', [1, 2, 4])
def test_elbo_chain_against_torch_distributions(skip):
    n, T, o = 3, 6, 2
    tstd = [0.01] * 4 + [0.02] * 12
    zs, mean, std, zdyn, lik = elbo_inputs(torch.Generator().manual_seed(skip), n, T, o, skip, tstd)
    elbo, trans, logq = elbo_chain(zs, mean, std, zdyn, lik, tstd, skip)
    N = torch.distributions.Normal
    lq = N(mean, std).log_prob(zs).sum((-2, -1))
    tr = N(zdyn, torch.tensor(tstd, dtype=torch.float64)).log_prob(zs[..., 2:]).sum((-2, -1))
    want = (tr + lik[:, skip - 1:] - lq).mean() + (lik[:, :skip - 1].mean() if skip > 1 else 0.0)
    assert torch.isfinite(elbo) and abs(float(elbo - want)) < 1e-12 * abs(float(want))
    assert abs(float(trans - tr.mean())) < 1e-12 * abs(float(tr.mean())) and abs(float(logq - lq.mean())) < 1e-12 * abs(float(lq.mean()))
    assert float(std.min()) < 0.06


def test_zall_chain_rows():
    n, T, o, skip = 2, 5, 3, 3
    g = torch.Generator().manual_seed(0)
    zfix, zs = torch.rand(n, T, o, 8, generator=g, dtype=torch.float64), torch.rand(n, T - skip, o, 18, generator=g, dtype=torch.float64)
    z = zall_chain(zfix, zs, skip).view(n, T - 1, o, 4)
    assert torch.equal(z[:, 1, 2], torch.stack([zfix[:, 2, 2, 0], zfix[:, 2, 2, 0] * zfix[:, 2, 2, 1], zfix[:, 2, 2, 2], zfix[:, 2, 2, 3]], -1))
    assert torch.equal(z[:, 2, 0, 1], zs[:, 0, 0, 0] * zs[:, 0, 0, 1]) and torch.equal(z[:, 3, 1, 2:], zs[:, 1, 1, 2:4])
    assert zall_chain(zfix, torch.rand(n, T - 1, o, 18, generator=g, dtype=torch.float64), 1).shape == (n * (T - 1) * o, 4)
