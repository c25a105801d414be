"""Stove.forward + backward against the float64 oracle at EVERY object count the kernels accept (1 .. 8), where the full-model tests
run three and six (and five in colour): the seams between the pieces that each claim 1 .. 8 -- the workspace layouts by
nmax_of / nmax_ch, the n_obj <= 3 / <= 6 / else ladders of the background SPN, the small-graph recursion kernels (2 .. 6) against
the block-wise ones, the matcher dispatch -- at (B, T) = (3, 5) and at one sequence with one recursion step, (1, 3), with the fused
dynamics / state / ELBO kernels and with the op-by-op chain, the parameter arena on, under the 'analytic' weights at every count
and the 'init' weights at 1, 4 and 8 objects.

Frames: helpers.paint_discs, every object its own radius and track; noise: O.draw_eps through noise_fn.  The frames are chosen on the
CPU (helpers.model_inputs) such that the oracle's own float32 run takes the matching and the fix_supair hits of its float64 run; that
is asserted again here before anything is compared.

Bars: those of test_gpu_dynamics.full_model_against_golden -- relative ELBO 1.5e-6, z and z_dyn 3e-6, z_sup 8e-6, every parameter
gradient 3e-4 / 3.5e-4 / 4e-3 (largest entry, L2, entry-wise) -- or 6 x the oracle's own float32 gap on the same inputs where that is
larger (gpu_helpers.regime_bar); the gap is printed next to every achieved error."""
import pytest
import torch

from gpu_helpers import check_ratio, err, err_l2, err_small, fill_analytic, regime_bar
from helpers import model_case_id, model_cases, model_cfg, model_decisions, model_inputs, oracle_stove
from test_gpu_dynamics import DEV, make_cfg

pytestmark = pytest.mark.gpu
_REFS = {}


def _reference(N, B, T, regime):
    """the oracle's step in float64 and in float32 on the case's inputs: once per (N, B, T, regime), shared by the switch settings"""
    key = (N, B, T, regime)
    if key not in _REFS:
        x, eps = model_inputs(N, B, T, regime)
        i64, h64 = model_decisions(N, regime, x, torch.float64)
        i32, h32 = model_decisions(N, regime, x, torch.float32)
        assert torch.equal(i64, i32) and torch.equal(h64, h32), 'the input condition does not hold'
        _REFS[key] = (oracle_stove(model_cfg(N), x, eps, regime=regime), oracle_stove(model_cfg(N), x, eps, regime=regime, dtype=torch.float32))
    return _REFS[key]


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize('case', model_cases(), ids=model_case_id)
def test_model_at_every_object_count(case):
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    N, B, T, regime, fused = case
    ref, low = _reference(N, B, T, regime)
    x, eps = model_inputs(N, B, T, regime)
    st = fill_analytic(Stove(make_cfg(fused_dynamics=fused, fused_state=fused, fused_elbo=fused, **model_cfg(N))), '', regime).to(DEV)
    ar = ParamArena(st)
    assert ar.has_spn and ar.has_gnn
    table = {'latent': eps['latent'][..., 0].float().to(DEV), 'std': eps['std'][..., 0].float().to(DEV),
             'steps': torch.stack(eps['steps'], 1).float().to(DEV)}
    st.noise_fn = lambda kind, shape: table[kind].reshape(shape)
    elbo, prop, _ = st(x.float().to(DEV), 0, None)
    (-elbo).backward()
    torch.cuda.synchronize()
    ar.check()
    tag = f'model_counts.N{N}' + ('' if regime == 'analytic' else '.' + regime)
    gap = _rel(low['elbo'], ref['elbo'])
    e = _rel(elbo, ref['elbo'])
    print(f'{tag}.elbo_rel {model_case_id(case)}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {regime_bar(1.5e-6, gap):.3g})')
    check_ratio(tag + '.elbo_rel', e, regime_bar(1.5e-6, gap))
    for k in ('z', 'z_dyn', 'z_sup'):
        assert prop[k].shape == ref['info'][k].shape == (B, T - 2, N, ref['info'][k].shape[-1])
        e, gap = err(prop[k], ref['info'][k]), err(low['info'][k], ref['info'][k])
        bar = regime_bar(8e-6 if k == 'z_sup' else 3e-6, gap)
        print(f'{tag}.{k} {model_case_id(case)}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {bar:.3g})')
        check_ratio(tag + '.' + k, e, bar)
    n = 0
    for k, p in st.named_parameters():
        want = ref['grads'].get(k)
        if want is None:
            continue
        assert p.grad is not None, k
        lo = low['grads'][k]
        if not bool(want.any()):
            # what the float64 oracle leaves exactly zero (the relational nets at one object, W_hh at one LSTM step) has no scale for a
            # relative error: it must be exactly zero here as well
            assert not bool(p.grad.any()), (k, float(p.grad.abs().max()))
        else:
            for sfx, fn, bar in (('', err, 3e-4), ('.l2', err_l2, 3.5e-4), ('.small', err_small, 4e-3)):
                e, gap = fn(p.grad, want), fn(lo, want)
                if gap > bar / 6:
                    print(f'{tag}.grad{sfx} {model_case_id(case)} {k}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {regime_bar(bar, gap):.3g})')
                check_ratio(tag + '.grad' + sfx, e, regime_bar(bar, gap))
        n += 1
    assert n == len(ref['grads']) and n > 100
