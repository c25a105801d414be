"""The float64 oracle's dynamics core and inference recursion at every object count the kernels accept (1 .. 8), not only at the three
and six objects the reference-generated fixtures hold (tests/test_oracle_goldens.py): tests/test_gpu_dynamics_counts.py measures the
kernels against it there, so it must not be an oracle that only works where it is pinned."""
import pytest
import torch

import stove_oracle as O
from helpers import (DYN_VARIANTS, dyn_actions, dyn_appearance, dyn_oracle, dyn_recursion_inputs, dyn_state, embed_actions, rel_err)

EPS64 = 2.0 ** -52
COUNTS = list(range(1, 9))
VARIANT_OF = {n: list(DYN_VARIANTS)[n % 3] for n in COUNTS}          # every variant at two or three counts
WIDTH_OF = {1: 16, 2: 32, 3: 64, 4: 16, 5: 64, 6: 32, 7: 32, 8: 32}   # cl = 16 / 64 take up to six objects


def _extra(params, n_obj, actions, app):
    """[action embedding | appearance] per object, the rows dynamics_forward appends to the state, or None"""
    rows = ([embed_actions(params, actions, n_obj)] if actions is not None else []) + ([app] if app is not None else [])
    return torch.cat(rows, -1) if rows else None


def _step_case(n_obj, B=3):
    cl, variant = WIDTH_OF[n_obj], VARIANT_OF[n_obj]
    c, params = dyn_oracle(cl, n_obj, variant)
    g = torch.Generator().manual_seed(40 + n_obj)
    return c, params, dyn_state(g, B, n_obj, cl), dyn_actions(g, variant, B), dyn_appearance(g, variant, B, n_obj)


def _recursion_case(n_obj, B=3, Ts=3):
    cl, variant = WIDTH_OF[n_obj], VARIANT_OF[n_obj]
    c, params = dyn_oracle(cl, n_obj, variant)
    g = torch.Generator().manual_seed(60 + n_obj)
    return (c, params) + dyn_recursion_inputs(g, B, Ts, n_obj, cl) + (dyn_actions(g, variant, B, Ts), dyn_appearance(g, variant, B, Ts, n_obj))


@pytest.mark.parametrize('n_obj', COUNTS)
def test_actions_enter_as_embedded_rows(n_obj):
    """dynamics_forward / recursion with `actions` equal the same calls with the embedded rows handed over next to the appearance:
    how the GPU tests hand the recursion kernels their `extra` input, and how the permutation test below permutes the embedding."""
    c, params, s, actions, app = _step_case(n_obj)
    with torch.no_grad():
        a = O.dynamics_forward(c, params, s, actions, app, with_pred=True)
        b = O.dynamics_forward(c, params, s, None, _extra(params, n_obj, actions, app), with_pred=True)
        for u, v in zip(a, b):
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        c, params, z1, zsup, zsstd, eps, actions, app = _recursion_case(n_obj)
        ra = O.recursion(c, params, z1, zsup, zsstd, eps.unbind(1), actions, app)
        rb = O.recursion(c, params, z1, zsup, zsstd, eps.unbind(1), None, _extra(params, n_obj, actions, app))
        for k in ('z', 'z_dyn', 'z_dyn_std', 'mean', 'std', 'log_q', 'dynamic_pred'):
            assert torch.equal(ra[k], rb[k]), k


@pytest.mark.parametrize('n_obj', COUNTS)
def test_object_permutation_equivariance(n_obj):
    """Objects permuted in -> the permuted result out, the reward (a sum over the objects) unchanged.  In float64 only the ORDER of
    sums changes: the relational sum over the N - 1 partners, and the order in which a library GEMM meets the rows.  One such
    reordering costs a few ulps of the largest entry; a step runs eleven layers in sequence behind it and the recursion feeds each
    step's state into the next, so the bars are 16 ulps for one step and 16 ulps per step for the recursion -- nine orders of
    magnitude below what a wrong pairing of the objects would show (the far-object test below: 1e-3 and more)."""
    perm = torch.tensor([k for k in (3, 1, 4, 0, 7, 2, 6, 5) if k < n_obj])          # no identity for N > 1: 1 comes before 0
    with torch.no_grad():
        c, params, s, actions, app = _step_case(n_obj)
        ex = _extra(params, n_obj, actions, app)
        res, rew, pred = O.dynamics_forward(c, params, s, None, ex, with_pred=True)
        res_p, rew_p, pred_p = O.dynamics_forward(c, params, s[:, perm], None, ex[:, perm] if ex is not None else None, with_pred=True)
        assert rel_err(res_p, res[:, perm]) < 16 * EPS64 and rel_err(pred_p, pred[:, perm]) < 16 * EPS64
        if c.action_conditioned:
            assert rel_err(rew_p, rew) < 16 * EPS64
        c, params, z1, zsup, zsstd, eps, actions, app = _recursion_case(n_obj)
        ex = _extra(params, n_obj, actions, app)
        Ts = zsup.shape[1]
        r = O.recursion(c, params, z1, zsup, zsstd, eps.unbind(1), None, ex)
        rp = O.recursion(c, params, z1[:, perm], zsup[:, :, perm], zsstd[:, :, perm], eps[:, :, perm].unbind(1), None,
                         ex[:, :, perm] if ex is not None else None)
        for k in ('z', 'z_dyn', 'z_dyn_std', 'mean', 'std', 'log_q', 'dynamic_pred'):
            assert rel_err(rp[k], r[k][:, :, perm]) < 16 * Ts * EPS64, k
        if c.action_conditioned:
            assert rel_err(torch.stack(rp['rewards'], 1), torch.stack(r['rewards'], 1)) < 16 * Ts * EPS64


@pytest.mark.parametrize('n_obj', COUNTS[:-1])
def test_one_more_object_far_away_changes_the_others(n_obj):
    """N -> N + 1 objects, the new one two units away from every other: the relational term is a sum over ALL partners weighted by a
    learned attention, not cut off by distance, so the predictions of the first N objects must move -- by far more than rounding
    (an oracle whose relational term silently vanished, or ignored the last object, would return them unchanged).  The threshold: 1e-4
    of the largest prediction, twelve orders of magnitude above float64 rounding; the plain core's parameters do not depend on N."""
    cl = 32 if n_obj + 1 > 6 else WIDTH_OF[n_obj]
    c, params = dyn_oracle(cl, n_obj, 'plain')
    c1, params1 = dyn_oracle(cl, n_obj + 1, 'plain')
    assert all(torch.equal(params[k], params1[k]) for k in params)
    g = torch.Generator().manual_seed(80 + n_obj)
    B, Ts = 3, 2
    with torch.no_grad():
        s = dyn_state(g, B, n_obj + 1, cl)
        s[:, -1, :2] = 2.8 + 0.1 * s[:, -1, :2]
        few, _, pred_few = O.dynamics_forward(c, params, s[:, :-1], with_pred=True)
        more, _, pred_more = O.dynamics_forward(c1, params1, s, with_pred=True)
        assert rel_err(more[:, :-1], few) > 1e-4 and rel_err(pred_more[:, :-1], pred_few) > 1e-4
        z1, zsup, zsstd, eps = dyn_recursion_inputs(g, B, Ts, n_obj + 1, cl)
        z1[:, -1, 2:4] += 3.0
        zsup[:, :, -1, 2:4] += 3.0
        r_few = O.recursion(c, params, z1[:, :-1], zsup[:, :, :-1], zsstd[:, :, :-1], eps[:, :, :-1].unbind(1))
        r_more = O.recursion(c1, params1, z1, zsup, zsstd, eps.unbind(1))
        for k in ('z', 'z_dyn', 'dynamic_pred'):
            assert rel_err(r_more[k][:, :, :-1], r_few[k]) > 1e-4, k
        # ... while what does not pass through the relational term stays: the SuPAIR scale columns of the fused mean
        assert torch.equal(r_more['mean'][:, :, :-1, :2], r_few['mean'][..., :2])
