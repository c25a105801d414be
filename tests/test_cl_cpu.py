"""CPU-side checks (-m "not gpu") of the state-code lengths 16 and 64: the float64 oracle against the reference's g20 fixtures
(tools/make_goldens_cl.py), the host side of `Dynamics` at those widths, and the parameter-image sizes the width-generic kernels report.
Regimes 'analytic' and 'init'; the 'stress' regime is out of scope here (its bars depend on the equal-codes machinery)."""
import ctypes
import os

import pytest
import torch

import stove_oracle as O
from helpers import load_golden, oracle_setup, rel_err, t_
from test_oracle_goldens import _full_model_against

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 64)
REGIMES = ('analytic', 'init')
DYN_VARIANTS = {
    'plain3': dict(num_obj=3), 'plain6': dict(num_obj=6),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
}
STOVE_CASES = {
    'n3': dict(num_obj=3),
    'n6': dict(num_obj=6, debug_match_objects='greedy', overlap_beta=100.0, max_obj_scale=0.22),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
}


def width_cfg(cl):
    return dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


def gname(stem, regime):
    return f'{stem}_f64' if regime == 'analytic' else f'{stem}_{regime}_f64'


@pytest.mark.parametrize('name', list(DYN_VARIANTS))
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('cl', WIDTHS)
def test_oracle_dynamics_step(cl, regime, name):
    tol = 1e-10
    g = load_golden(gname(f'g20_dynamics_cl{cl}_{name}', regime))
    c, structs, params = oracle_setup(torch.float64, regime=regime, **DYN_VARIANTS[name], **width_cfg(cl))
    s = t_(g['s'], torch.float64).requires_grad_()
    assert s.shape[-1] == cl // 2
    act = t_(g['actions'], torch.float64) if 'actions' in g else None
    app = t_(g['app'], torch.float64).requires_grad_() if 'app' in g else None
    res, rew = O.dynamics_forward(c, params, s, act, app, lim_enc=int(g['lim_enc']))
    assert rel_err(res.detach(), g['result']) < tol
    loss = (res * t_(g['w'], torch.float64)).sum()
    if c.action_conditioned:
        assert rel_err(rew.detach(), g['reward']) < tol
        loss = loss + (rew * torch.linspace(1, 2, s.shape[0], dtype=torch.float64).view(-1, 1)).sum()
    loss.backward()
    assert rel_err(s.grad, g['gs']) < tol * 10
    if app is not None:
        assert rel_err(app.grad, g['gapp']) < tol * 10
    n = 0
    for k, v in g.items():
        if k.startswith('g_'):
            assert rel_err(params['dyn.' + k[2:]].grad, v) < tol * 10, k
            n += 1
    assert n >= 26


@pytest.mark.parametrize('name', list(STOVE_CASES))
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('cl', WIDTHS)
def test_oracle_full_model(cl, regime, name):
    g = load_golden(gname(f'g20_stove_cl{cl}_{name}', regime))
    assert g['eps_steps'].shape[-1] == cl // 2 + 2 and g['roll_z'].shape[1] == 8
    _full_model_against(g, name, regime, torch.float64, cfg=dict(STOVE_CASES[name], **width_cfg(cl)))


def _cfg(cl, **kw):
    from stove_amd.video_prediction.config import StoveConfig
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = torch.device('cpu'), torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    cfg.cl = cl
    cfg.transition_lik_std = [0.01] * (cl // 2)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize('name', list(DYN_VARIANTS))
@pytest.mark.parametrize('cl', WIDTHS)
def test_dynamics_constructs_at_the_new_widths(cl, name):
    """`Dynamics` at cl = 16 / 64: the state dict is the reference's (names, shapes, order), the parameter image has the size the
    width-generic kernels read.  (Fails before this width support: the constructor raised NotImplementedError.)"""
    from stove_amd import _lib, build
    from stove_amd.video_prediction.dynamics import Dynamics
    build.build_library()
    g = load_golden(f'g20_dynamics_cl{cl}_{name}_f64')
    dyn = Dynamics(_cfg(cl, **DYN_VARIANTS[name]))
    sd = dyn.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['sd_names']]
    for (k, v), shp in zip(sd.items(), g['sd_shapes']):
        assert tuple(v.shape) == tuple(int(d) for d in shp[:v.dim()]), k
    w, v, wt = dyn.param_image(0)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for fn in ('stove_gnn_param_floats_cl', 'stove_gnn_grad_floats_cl'):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert w.numel() + v.numel() + wt.numel() == lib.stove_gnn_param_floats_cl(cl) == 44 * cl * cl + 21 * cl
    assert w.numel() + v.numel() == lib.stove_gnn_grad_floats_cl(cl)
    assert lib.stove_gnn_param_floats_cl(24) == 0


def test_unsupported_width_and_short_transition_std_raise():
    from stove_amd.video_prediction.dynamics import Dynamics
    with pytest.raises(NotImplementedError, match='16, 32, 64'):
        Dynamics(_cfg(24))
    with pytest.raises(ValueError, match='transition_lik_std'):
        Dynamics(_cfg(16, transition_lik_std=[0.01, 0.01, 0.01, 0.01]))
    Dynamics(_cfg(32, transition_lik_std=[0.01, 0.01, 0.01, 0.01]))      # the reference's default still pads to 16 entries at cl = 32


def test_float32_gap_records_cover_every_case():
    """tests/golden/g20_reference_fp32_gap.json (tools/make_goldens_cl.py gap) has a finite record for every g20 fixture and for every
    shape of the ragged-batch and T = 100 GPU tests: the bars of tests/test_gpu_cl.py read them, and a missing record must not pass for a zero."""
    import json
    import math
    with open(os.path.join(ROOT, 'tests', 'golden', 'g20_reference_fp32_gap.json')) as f:
        gaps = json.load(f)['gaps']
    want = [f'g20_dynamics_cl{cl}_{n}_{r}' for cl in WIDTHS for r in REGIMES for n in DYN_VARIANTS]
    want += [f'g20_stove_cl{cl}_{n}_{r}' for cl in WIDTHS for r in REGIMES for n in STOVE_CASES]
    want += [f'ragged_cl{cl}_n{n}_B{B}' for cl in WIDTHS for n in (3, 6) for B in (1, 5, 64, 257)]
    want += [f'T100_cl{cl}_{n}' for cl in WIDTHS for n in ('n3', 'n6')]
    assert sorted(want) == sorted(gaps)

    def leaves(v):
        if isinstance(v, dict):
            for x in v.values():
                yield from leaves(x)
        else:
            yield v
    for k, v in gaps.items():
        assert all(isinstance(x, float) and math.isfinite(x) for x in leaves(v)), k
        if k.startswith('g20_stove'):
            assert v['grad_tensor']['max'] < 1e-4 and v['elbo_rel'] < 1e-6, k
