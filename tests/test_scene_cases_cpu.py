"""The conditions tests/scene_cases.py states for the inputs of tests/test_gpu_scene_counts.py, checked from the float64 oracle and its
own float32 run alone (no kernel, no GPU): which gradient tensors underflow float32 and where they lie, the caps on every float32
gap, finiteness, that everything held relatively has a scale, and that exchanging two objects moves the oracle's log p far beyond
the bar.  A case that breaks a condition gets another seed (scene_cases.SEED_SHIFT); the conditions stay.

`pytest -s tests/test_scene_cases_cpu.py` prints the table of gaps and underflow counts."""
import pytest
import torch

import scene_cases as S
from gpu_helpers import err

KEYS = ('log_p', 'part', 'dz', 'dz.l2', 'dz.small', 'grad', 'grad.l2', 'grad.small')


def _row(case, regime):
    """the largest gap per quantity of a (case, regime)"""
    g = S.gaps(case, regime)
    row = {k: g[k] for k in ('log_p', 'dz', 'dz.l2', 'dz.small')}
    row['part'] = max(g['part.bg'], g['part.patch'], g['part.overlap'])
    for sfx in S.ERR_FN:
        row['grad' + sfx] = max(g['grad' + sfx].values())
    return row


@pytest.mark.parametrize('case,regime', S.pairs() + S.degenerate_pairs(), ids=lambda v: v)
def test_conditions_of_a_case(case, regime):
    hi, lo = S.reference(case, regime), S.reference(case, regime, torch.float32)
    compared, under, zero = S.classify(case, regime)
    for ref in (hi, lo):
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ('log_p', 'parts', 'dz'))
        assert all(bool(torch.isfinite(g).all()) for g in ref['grads'].values())
    assert set(hi['grads']) == set(lo['grads']) and len(compared) >= 6
    # a tensor without a float32 scale is a leaf tensor of the background SPN: at most four underflow; only the saturated weights
    # take any below float64's range altogether, and then at most two of the three replicas (four leaf tensors each)
    assert len(under) <= S.MAX_UNDERFLOWING_TENSORS, under
    assert all(k.startswith(S.UNDERFLOW_PREFIX) for k in under + zero), (under, zero)
    assert len(zero) <= 8 and (regime == 'stress' or not zero), zero
    for k in compared:
        assert float(hi['grads'][k].abs().max()) >= S.UNDERFLOW and float(lo['grads'][k].abs().max()) > 0, k
    assert float(hi['dz'].abs().max()) > 0
    row = _row(case, regime)
    print(f'{case:16s} {regime:9s} underflowing {len(under)} zero {len(zero)}  ' + '  '.join(f'{k} {row[k]:.3g}' for k in KEYS))
    for k in KEYS:
        assert row[k] <= S.cap(k), (k, row[k], S.cap(k))


def test_few_pairs_have_underflowing_tensors():
    have = [(case, regime) for case, regime in S.pairs() if S.classify(case, regime)[1]]
    print('underflowing:', have)
    assert len(S.pairs()) == 39 and len(have) <= S.MAX_UNDERFLOWING_PAIRS, have


def test_the_largest_gaps_lie_within_their_caps():
    """prints the largest gap per quantity over all pairs: what scene_cases.MEASURED records for the quantities whose caps are twice
    the measurement (a float32 run rounds differently from one CPU to the next, so the record is not asserted digit for digit)"""
    worst = {k: max(_row(case, regime)[k] for case, regime in S.pairs() + S.degenerate_pairs()) for k in KEYS}
    print('largest gaps:', {k: f'{v:.3g}' for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= S.cap(k), (k, v, S.cap(k))


@pytest.mark.parametrize('case', S.ORDER_CASES)
def test_exchanging_two_objects_moves_the_oracle_far_beyond_the_bar(case):
    ref, gap = S.reference(case, 'analytic')['log_p'], S.gaps(case, 'analytic')['log_p']
    moved, bar = err(S.swapped_log_p(case, 'analytic'), ref), S.bar('log_p', gap)
    print(f'{case}: log p moves by {moved:.3g} = {moved / bar:.3g} x the bar {bar:.3g}')
    assert moved > 100 * bar
