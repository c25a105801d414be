"""The state-supervised baseline on the GPU (csrc/gnn_sup.hip, ops.sup_rollout / sup_loss, stove_amd/supairvised) against its
specification: the composed loop of core steps bit for bit, and tests/sup_ref.py in float64.

Cases and inputs: tests/sup_cases.py (tests/test_sup_cpu.py holds their conditioning).  Bars: pred at regime_bar(2e-6 one step /
3e-6 otherwise, gap), gradients at regime_bar((3e-4, 3.5e-4, 4e-3), gap) on check_grad's three scales, gap = what sup_ref's float32
run differs from its float64 run by on the same inputs, measured inside the test and printed next to the achieved error."""
import ctypes
import pickle
import types

import numpy as np
import pytest
import torch

import sup_cases as C
import sup_ref as S
from gpu_helpers import check, check_grad, err, err_l2, err_small, regime_bar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INVALID = 1          # hipErrorInvalidValue


def _config(cl, n_obj, nl='relu', **kw):
    from stove_amd.supairvised.config import SupStoveConfig
    c = SupStoveConfig()
    c.cl, c.num_obj, c.debug_nonlinear = cl, n_obj, nl
    c.device, c.dtype = torch.device(DEV), torch.float32
    c.action_conditioned, c.action_space = False, None
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _model(cl, n_obj, nl, fill):
    """SupStove on the device, every Linear filled by its name's rule (cores 1 and 2 too: nothing reads them)"""
    from stove_amd.supairvised.supstove import SupStove
    st = SupStove(_config(cl, n_obj, nl))
    with torch.no_grad():
        for name, p in st.named_parameters():
            fan_in = dict(st.named_parameters())[name[:-4] + 'weight'].shape[-1] if name.endswith('.bias') else None
            p.copy_(S.regime_tensor(name, p.shape, fill, torch.float64, fan_in).float())
    return st.to(DEV)


def _dev(t, grad=False):
    return t.float().to(DEV).requires_grad_(grad)


def _loss_stub(cfg):
    return types.SimpleNamespace(c=cfg)


def _device_case(st, d, R, fused, which):
    """forward + backward of one loss -> pred, codes, losses, {name: gradient} (parameters with a gradient, and latent0)"""
    from stove_amd.supairvised.train import SupTrainer
    st.zero_grad(set_to_none=True)
    x, lat, fut = _dev(d['x']), _dev(d['latent0'], True), _dev(d['future'])
    pred, recon, codes = st.dyn(x, num_rollout=R, fused=fused, latent=lat, return_codes=True)
    assert recon is x and pred.grad_fn is not None
    if which == 'total':
        total, pred_loss, recon_loss = SupTrainer.compute_loss(_loss_stub(st.c), x, fut, recon, pred)
        assert float(recon_loss) == 0.0
        losses = (total.detach(), pred_loss.detach())
    else:
        total, losses = (pred * _dev(d['w'])).sum(), None
    total.backward()
    grads = {'dyn.' + k: p.grad.clone() for k, p in st.dyn.named_parameters() if p.grad is not None}
    grads['latent0'] = lat.grad.clone()
    return {'pred': pred.detach(), 'codes': codes.detach(), 'losses': losses, 'grads': grads}


# ------------------------------------------------------------------------------------------------ 1. fused == composed, bit for bit
@pytest.mark.parametrize('case', C.cases(), ids=C.case_id)
def test_fused_forward_equals_the_composed_loop_bit_for_bit(case):
    """pred and every step's input code of the one-launch kernel against the loop of ops.gnn_step calls: both run cl_forward<CL> on the
    same rows in the same workgroups, and a row's arithmetic does not depend on its neighbours in the tile"""
    cl, N, B, V, R, fill, nl = case
    d = C.inputs(case)
    st = _model(cl, N, nl, fill)
    with torch.no_grad():
        x, lat = _dev(d['x']), _dev(d['latent0'])
        pf, _, cf = st.dyn(x, num_rollout=R, fused=True, latent=lat, return_codes=True)
        pc, _, cc = st.dyn(x, num_rollout=R, fused=False, latent=lat, return_codes=True)
    assert pf.shape == (B, R, N, 4) and cf.shape == (B, V - 1 + R, N, cl)
    assert torch.equal(cf, cc), float((cf - cc).abs().max())
    assert torch.equal(pf, pc), float((pf - pc).abs().max())
    assert torch.equal(cf[:, :V, :, :4], x) and torch.equal(cf[:, 0, :, 4:], lat)          # the labels are teacher-forced as they are


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize('case', C.cases(), ids=C.case_id)
def test_fused_rollout_and_gradients_against_float64(case):
    """SupervisedDynamics.forward(fused=True) + SupTrainer.compute_loss, and a second loss with random weights on pred, against
    sup_ref: pred, the losses, d latent0 and the gradient of exactly the reference's 28 tensors (the encoder and core 0).  The losses
    are held at 10 x pred's bar: d loss / loss <= 2 max|d pred| / rms|pred - future|, and max|pred| / rms|pred - future| stays below
    5 on these inputs (positions in [0, 2] against independent draws from the same range)."""
    cl, N, B, V, R, fill, nl = case
    key = 'sup.' + ('step' if C.one_step(case) else 'rollout')
    d = C.inputs(case)
    hi, lo = C.ref_case(case, torch.float64, d), C.ref_case(case, torch.float32, d)
    st = _model(cl, N, nl, fill)
    got = _device_case(st, d, R, True, 'total')
    e, gap = err(got['pred'], hi['pred']), err(lo['pred'], hi['pred'])
    bar = regime_bar(C.PRED_BAR_STEP if C.one_step(case) else C.PRED_BAR_ROLLOUT, gap)
    print(f'{C.case_id(case)}.pred: {e:.3g} (sup_ref f32 gap {gap:.3g}, bar {bar:.3g})')
    check(key + '.pred', e, bar)
    for i, name in enumerate(('total', 'pred_loss')):
        check(key + '.' + name, abs(float(got['losses'][i]) - float(hi['losses'][i])) / abs(float(hi['losses'][i])), 10 * bar)
    for which, got_w in (('g_total', got), ('g_w', _device_case(st, d, R, True, 'w'))):
        want, low = hi[which], lo[which]
        assert set(got_w['grads']) == set(want) and len(want) == 29, sorted(set(got_w['grads']) ^ set(want))
        gaps = [max(f(low[k], want[k]) for k in want) for f in (err, err_l2, err_small)]
        worst = [max(f(got_w['grads'][k], want[k]) for k in want) for f in (err, err_l2, err_small)]
        print(f'{C.case_id(case)}.{which}: max {worst[0]:.3g} ({gaps[0]:.3g})  l2 {worst[1]:.3g} ({gaps[1]:.3g})  small {worst[2]:.3g} '
              f'({gaps[2]:.3g})  [achieved (sup_ref f32 gap)]')
        bars = [regime_bar(b, g) for b, g in zip(C.GRAD_BARS, gaps)]
        assert all(bar <= C.CAP * b for bar, b in zip(bars, C.GRAD_BARS)), gaps
        for k in want:
            check_grad(key + '.' + which, got_w['grads'][k], want[k], *bars)


# ------------------------------------------------------------------------------------------------ 3. the loss kernel
@pytest.mark.parametrize('shape', [(11, 4, 3), (256, 8, 3), (5, 1, 6), (1, 2, 1)], ids=lambda s: 'B%d-R%d-N%d' % s)
@pytest.mark.parametrize('end', [2, 4])
@pytest.mark.parametrize('with_delta', [True, False], ids=['delta', 'nodelta'])
def test_loss_kernel_against_float64(shape, end, with_delta):
    from stove_amd import ops
    B, R, N = shape
    g = torch.Generator().manual_seed(100 * B + 10 * R + N)
    fut = torch.rand(B, R, N, 4, generator=g, dtype=torch.float64).float().double()
    pred = (fut + 0.3 * torch.randn(B, R, N, 4, generator=g, dtype=torch.float64)).float().double().requires_grad_()
    want = S.sup_loss_ref(pred, fut, C.DISCOUNT, end, with_delta)
    (2.5 * want[0]).backward()
    p = _dev(pred.detach(), True)
    got = ops.sup_loss(p, _dev(fut), C.DISCOUNT, end, with_delta)
    (2.5 * got[0]).backward()
    for name, a, b in zip(('total', 'pred', 'delta'), got, want):
        if float(b.detach()) == 0.0:
            assert float(a) == 0.0, name
        else:
            check('sup.loss.' + name, abs(float(a) - float(b)) / abs(float(b)), 1e-6)
    assert (float(want[2]) == 0.0) == (R == 1 or not with_delta)
    check_grad('sup.loss.d_pred', p.grad, pred.grad, 2.5e-5, 2e-5, 1e-3)          # the step's gradient bars (tests/test_gpu_dynamics_counts.py)
    assert float(p.grad[..., end:].abs().max()) == 0.0 if end < 4 else True
    assert not got[1].requires_grad and not got[2].requires_grad


# ------------------------------------------------------------------------------------------------ 4. reproducibility and edges
def test_two_calls_agree_bit_for_bit():
    case = (16, 3, 11, 3, 4, 'init', 'relu')
    d = C.inputs(case)
    st = _model(16, 3, 'relu', 'init')
    a, b = _device_case(st, d, 4, True, 'total'), _device_case(st, d, 4, True, 'total')
    assert torch.equal(a['pred'], b['pred'])
    assert set(a['grads']) == set(b['grads'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k


@pytest.mark.parametrize('cl', [16, 64])
def test_rollout_without_codes_and_long_rollout_prefix(cl):
    """a no-grad call passes codes = NULL: the same pred bits; 40 steps are the first 40 of 60"""
    case = (cl, 3, 7, 3, 4, 'init', 'relu')
    d = C.inputs(case)
    st = _model(cl, 3, 'relu', 'init')
    x, lat = _dev(d['x']), _dev(d['latent0'])
    with torch.no_grad():
        plain, _ = st.dyn(x, num_rollout=4, fused=True, latent=lat)
        long40, _ = st.dyn(x, num_rollout=40, fused=True, latent=lat)
        long60, _ = st.dyn(x, num_rollout=60, fused=True, latent=lat)
    with_codes, _, codes = st.dyn(x, num_rollout=4, fused=True, latent=lat.clone().requires_grad_(), return_codes=True)
    assert codes.shape == (7, 6, 3, cl) and torch.equal(plain, with_codes.detach())
    assert torch.equal(long40, long60[:, :40]) and torch.equal(long40[:, :4], plain)
    assert bool(torch.isfinite(long60).all())


def test_empty_batch():
    st = _model(16, 3, 'relu', 'init')
    x, lat = torch.zeros(0, 3, 3, 4, device=DEV), torch.zeros(0, 3, 12, device=DEV, requires_grad=True)
    pred, _ = st.dyn(x, num_rollout=4, fused=True, latent=lat)
    assert pred.shape == (0, 4, 3, 4)
    pred.sum().backward()
    assert lat.grad.shape == (0, 3, 12)
    grads = [p.grad for k, p in st.dyn.named_parameters() if p.grad is not None]
    assert len(grads) == 28 and all(float(g.abs().max()) == 0.0 for g in grads)


def test_arena_gradient_equals_the_per_parameter_path():
    from stove_amd.arena import ParamArena
    case = (16, 3, 11, 3, 4, 'half', 'relu')
    d = C.inputs(case)
    plain, flat = _model(16, 3, 'relu', 'half'), _model(16, 3, 'relu', 'half')
    arena = ParamArena(flat)
    assert arena.has_gnn
    want = _device_case(plain, d, 4, True, 'total')
    arena.zero_grad()
    x, lat, fut = _dev(d['x']), _dev(d['latent0'], True), _dev(d['future'])
    from stove_amd.supairvised.train import SupTrainer
    pred, recon = flat.dyn(x, num_rollout=4, fused=True, latent=lat)
    SupTrainer.compute_loss(_loss_stub(flat.c), x, fut, recon, pred)[0].backward()
    assert torch.equal(pred.detach(), want['pred']) and torch.equal(lat.grad, want['grads']['latent0'])
    seen = 0
    for k, p in flat.dyn.named_parameters():
        g = arena.view_of(p, arena.grad)
        if 'dyn.' + k in want['grads']:
            assert torch.equal(g, want['grads']['dyn.' + k]), k
            seen += 1
        else:
            assert float(g.abs().max()) == 0.0, k
    assert seen == 28


# ------------------------------------------------------------------------------------------------ 5. C ABI
def test_rejections_leave_the_outputs_untouched():
    from stove_amd import _lib
    lib = _lib.load()
    cl, B, V, R, N = 16, 4, 3, 4, 3
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)          # noqa: E731
    z = lambda *s: torch.zeros(*s, device=DEV)          # noqa: E731
    x, lat, params = z(B, V, N, 4), z(B, N, cl - 4), z(lib.stove_gnn_param_floats_cl(cl))
    pred, codes, dlat, g = nan(B, R, N, 4), nan(B, V - 1 + R, N, cl), nan(B, N, cl - 4), nan(lib.stove_gnn_grad_floats_cl(cl))
    ws, dp, losses = nan(lib.stove_sup_rollout_bwd_ws_bytes(cl, B, N) // 4), z(B, R, N, 4), nan(3)
    P = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def fwd(x=x, lat=lat, params=params, pred=pred, cl=cl, B=B, V=V, R=R, N=N):
        return lib.stove_sup_rollout_fwd(P(x), P(lat), P(params), P(pred), P(codes), cl, B, V, R, N, 0, st)

    def bwd(x=x, params=params, codes=codes, dp=dp, g=g, ws=ws, cl=cl, B=B, V=V, R=R, N=N):
        return lib.stove_sup_rollout_bwd(P(x), P(params), P(codes), P(dp), P(dlat), P(g), P(ws), cl, B, V, R, N, 0, st)

    def loss(pred=dp, fut=dp, losses=losses, d=dlat, B=B, R=R, N=N, end=4):
        return lib.stove_sup_loss(P(pred), P(fut), P(losses), P(d), B, R, N, end, 1, ctypes.c_double(0.98), st)
    for kw in (dict(x=None), dict(lat=None), dict(params=None), dict(pred=None), dict(cl=32), dict(cl=48), dict(N=0), dict(N=7), dict(V=0),
               dict(R=0), dict(B=-1)):
        assert fwd(**kw) == INVALID, kw
    for kw in (dict(x=None), dict(params=None), dict(codes=None), dict(dp=None), dict(g=None), dict(ws=None), dict(cl=32), dict(N=0),
               dict(N=7), dict(V=0), dict(R=0)):
        assert bwd(**kw) == INVALID, kw
    for kw in (dict(pred=None), dict(fut=None), dict(losses=None), dict(d=None), dict(end=3), dict(end=0), dict(B=0), dict(R=0), dict(N=7)):
        assert loss(**kw) == INVALID, kw
    torch.cuda.synchronize()
    for name, t in (('pred', pred), ('codes', codes), ('d_latent0', dlat), ('g_params', g), ('ws', ws), ('losses', losses)):
        assert bool(torch.isnan(t).all()), name
    assert fwd() == 0 and bwd() == 0                                  # the same buffers pass with the arguments in order
    torch.cuda.synchronize()
    assert not bool(torch.isnan(pred).any()) and not bool(torch.isnan(g).any()) and not bool(torch.isnan(dlat).any())


# ------------------------------------------------------------------------------------------------ 6. the trainer
def _write(tmp_path):
    from stove_amd.envs import envs
    d = envs.synth_sequences('billiards', 8, 20)
    data = {'X': np.transpose(d['X'], (0, 1, 3, 4, 2)).astype(np.float64), 'y': d['y'], 'coord_lim': 10, 'r': 1.2}
    path = str(tmp_path / 'billiards.pkl')
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    return path


def _trainer(tmp_path, **extra):
    import model.main as M
    path = _write(tmp_path)
    args = {'supairvised': 'True', 'traindata': path, 'testdata': path, 'experiment_dir': str(tmp_path), 'batch_size': '4',
            'num_visible': '3', 'num_rollout': '4', 'num_workers': '0', 'dtype': 'torch.float', 'random_seed': '42', 'print_every': '1',
            'num_epochs': '1', 'long_rollout_every': '1000000', 'save_every': '1000000'}
    args.update(extra)
    return M.main(sh_args=args)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_three_optimiser_steps_track_the_float64_chain(tmp_path, fused):
    """Three Adam steps (the config's amsgrad setting, no clipping, fixed learning rate) on one batch with a fed latent, against
    sup_ref + torch.optim.Adam in float64 started from the same parameters.  Held: the loss of every step.  Bar: the float32 forward's
    3e-6, plus what the parameter differences can move the loss by -- an entry whose gradient g carries a relative float32 error of up
    to 3e-4 max|g| (the gradient bar) takes an Adam step that is off by at most lr 3e-4 max|g| / |g|, which changes the loss by at most
    lr 3e-4 max|g| per entry and per step, over the P entries of the encoder and core 0."""
    from stove_amd.supairvised import dynamics as SD
    from stove_amd.supairvised.train import SupTrainer
    tr = _trainer(tmp_path, nolog='True')
    assert isinstance(tr, SupTrainer) and tr.c.cl == 16 and tr.c.num_obj == 3
    data = next(iter(tr.dataloader))
    assert data['present_labels'].shape == (4, 3, 3, 4) and data['future_labels'].shape == (4, 4, 3, 4)
    assert float(data['present_labels'][..., :2].min()) >= 0.0 and float(data['present_labels'][..., :2].max()) <= 2.0
    shapes = S.core0_shapes(16)
    params = {'dyn.' + k: p.detach().double().cpu().clone().requires_grad_() for k, p in tr.stove.dyn.named_parameters() if 'dyn.' + k in shapes}
    assert len(params) == 28
    start = {k: p.detach().cpu().clone() for k, p in tr.stove.dyn.named_parameters()}
    opt = torch.optim.Adam(list(params.values()), lr=tr.c.learning_rate, amsgrad=tr.c.debug_amsgrad)
    lat = torch.randn(4, 3, 12, generator=torch.Generator().manual_seed(5), dtype=torch.float64).float()
    x, fut = data['present_labels'].double().cpu(), data['future_labels'].double().cpu()
    c = S.sup_config(16, tr.c.debug_nonlinear, num_obj=3)
    P = sum(p.numel() for p in params.values())
    SD.FUSED_DEFAULT, keep = fused, SD.FUSED_DEFAULT
    try:
        slack = 0.0
        for step in range(3):
            opt.zero_grad()
            want = S.sup_loss_ref(S.sup_rollout_ref(c, params, x, lat.double(), 4), fut, tr.c.discount_factor)
            want[0].backward()
            gmax = max(float(p.grad.abs().max()) for p in params.values())
            opt.step()
            total, pred_loss, recon_loss = tr.train_step(data, latent=lat.to(DEV))
            bar = 3e-6 + slack / float(want[0])
            e = abs(float(total) - float(want[0])) / float(want[0])
            print(f'step {step}: loss {float(total):.6g} against {float(want[0]):.6g}: {e:.3g} (bar {bar:.3g})')
            check('sup.trainer.loss', e, bar)
            assert float(recon_loss) == 0.0 and abs(float(pred_loss) - float(want[1])) / float(want[1]) < bar
            slack += tr.c.learning_rate * 3e-4 * gmax * P
    finally:
        SD.FUSED_DEFAULT = keep
    for k, p in tr.stove.dyn.named_parameters():
        if 'dyn.' + k in params:
            assert not torch.equal(p.detach().cpu(), start[k]), k          # every tensor of the encoder and core 0 moved
    for k, p in tr.stove.dyn.named_parameters():                      # cores 1 and 2 never move
        if 'dyn.' + k not in params:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


def test_trainer_logs_rolls_out_and_restores(tmp_path):
    import os
    tr = _trainer(tmp_path)
    data = next(iter(tr.dataloader))
    tr.train_step(data)
    tr.test(1, 0.0)
    rows = open(tr.logger.performance_file).read().strip().split('\n')
    assert rows[0] == 'step,time,error,type,frame,test'
    assert len(rows) == 1 + 3 * min(len(tr.test_dataloader), 9) and [r.split(',')[4] for r in rows[1:4]] == ['total', 'pred', 'recon']
    assert all(r.split(',')[3] == 'vin_true' and r.split(',')[5] == 'True' and np.isfinite(float(r.split(',')[2])) for r in rows[1:])
    tr.long_rollout(idx=[0, 1], step_counter=1, num=30)
    for name in ('error.csv', 'std_error.csv'):
        line, = open(os.path.join(tr.logger.exp_dir, name)).read().strip().split('\n')
        vals = [float(v) for v in line.split(',')]
        assert len(vals) == 20 and all(np.isfinite(vals))             # 3 visible + the 17 frames the 20-frame test set has left
        assert name != 'error.csv' or vals[:3] == [0.0, 0.0, 0.0]    # the observed frames come back as they went in
    states = np.load(os.path.join(tr.logger.rollout_states_dir, 'rollout_states_00001.npy'))
    assert states.shape == (8, 33, 3, 4) and np.isfinite(states).all()
    assert np.load(os.path.join(tr.logger.rollout_states_dir, 'real_states.npy')).shape == (8, 20, 3, 4)
    tr.save(0, 1)
    ckpt = os.path.join(tr.logger.checkpoint_dir, 'ckpt')
    other = _trainer(tmp_path, nolog='True', random_seed='7')
    assert not all(torch.equal(a, b) for a, b in zip(tr.stove.parameters(), other.stove.parameters()))
    other.c.checkpoint_path = ckpt
    other.load()
    assert (other.epoch_start, other.step_start) == (0, 1)
    assert all(torch.equal(a, b) for a, b in zip(tr.stove.parameters(), other.stove.parameters()))
    lat = torch.randn(4, 3, 12, device=DEV)
    a, b = tr.train_step(data, latent=lat), other.train_step(data, latent=lat)
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(p, q) for p, q in zip(tr.stove.parameters(), other.stove.parameters()))      # the optimiser state came along
