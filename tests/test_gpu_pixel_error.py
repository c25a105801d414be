"""Pixel-space prediction error on the GPU: the run-time-sized render kernel with the fused squared error (csrc/render.hip,
stove_render_frames_any) against the float64 restatement of tests/render_ref.py, its invariants and refusals, colour
Supair.reconstruct_from_z, Trainer.pixel_error (fused against materialised) and colour clips from Trainer.long_rollout.

Bars.  Pixels: 2e-5 absolute, the project's pixel bar for fp32 bilinear sums on values in [0, 1] (tests/test_gpu_render.py); the CPU
suite shows ATen's own float32 composed render within it on the same inputs (tests/test_pixel_error_cpu.py).  sqerr against float64:
2 tol sum|frame64 - truth| + P tol^2 + 1e-6 sqerr64 -- every pixel within tol, summed in float32.  sqerr against the float64 sum
over the kernel's OWN float32 frame: 1e-6 relative, the float32 summation alone (<= 7500 terms in 4 waves of 64 lanes: partial sums
of ~30 terms, then 6 DPP levels and 3 adds, each rounding at 6e-8 relative)."""
import pickle
import zlib

import numpy as np
import pytest
import torch

import render_ref as R
from gpu_helpers import fill_analytic
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PIX_TOL = R.PIX_TOL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np64(t):
    return t.detach().double().cpu().numpy()


def _call(ops, inp, n_obj, per, geom, truth=True, want_frames=True):
    return ops.render_frames_any(_dev(inp['bg']), _dev(inp['patches']), per, _dev(inp['z']), n_obj, geom,
                                 truth=_dev(inp['truth']) if truth else None, want_frames=want_frames)


# ---------------------------------------------------------------------------------------------------- 1. kernel vs render_ref
@pytest.mark.parametrize('align_corners', [False, True])
@pytest.mark.parametrize('geom5', R.GEOMS, ids=lambda g: 'c%d_%dx%d_p%dx%d' % g)
def test_render_kernel_against_float64(geom5, align_corners):
    from stove_amd import ops
    P = geom5[0] * geom5[1] * geom5[2]
    worst = dict(pix=0.0, sq=0.0, red=0.0)
    for n_obj, nf, per, geom, inp, ref in R.kernel_cases(geom5, align_corners):
        out, sq = _call(ops, inp, n_obj, per, geom)
        assert out.shape == (nf, P) and sq.shape == (nf,) and out.dtype == sq.dtype == torch.float32
        out, sq = _np64(out), _np64(sq)
        pix = float(np.abs(out - ref).max())
        sq64 = R.sqerr(ref, inp['truth'])
        ratio = float((np.abs(sq - sq64) / R.sqerr_bound(ref, inp['truth'], PIX_TOL)).max())
        own = R.sqerr(out, inp['truth'])
        red = float((np.abs(sq - own) / own).max())
        print('n_obj %d frames %2d per %d: pixel gap %.3g, sqerr gap / bound %.3g, reduction rel %.3g' % (n_obj, nf, per, pix, ratio, red))
        worst = dict(pix=max(worst['pix'], pix), sq=max(worst['sq'], ratio), red=max(worst['red'], red))
        assert pix <= PIX_TOL, (n_obj, nf, per, pix)
        assert ratio <= 1.0, (n_obj, nf, per, ratio)
        assert red <= 1e-6, (n_obj, nf, per, red)
    print('worst', worst)


# ---------------------------------------------------------------------------------------------------- 2. invariants
@pytest.mark.parametrize('geom5', R.GEOMS, ids=lambda g: 'c%d_%dx%d_p%dx%d' % g)
def test_render_kernel_invariants(geom5):
    from stove_amd import ops
    C, W, H, pw, ph = geom5
    for ac in (False, True):
        geom = tuple(geom5) + (ac,)
        for n_obj, nf, per in ((3, 65, 1), (8, 3, 5), (1, 3, 0)):
            inp = R.draw_case(77 + n_obj, nf, n_obj, geom, per)
            out, sq = _call(ops, inp, n_obj, per, geom)
            out2, sq2 = _call(ops, inp, n_obj, per, geom)
            assert torch.equal(out, out2) and torch.equal(sq, sq2)                              # two calls, bit for bit
            none, sq_only = _call(ops, inp, n_obj, per, geom, want_frames=False)
            assert none is None and torch.equal(sq_only, sq)                                    # sqerr with and without out
            assert torch.equal(_call(ops, inp, n_obj, per, geom, truth=False), out)             # out with and without truth (tiled launch)
            blank = dict(inp, patches=np.zeros_like(inp['patches']))
            want = _dev(inp['bg']).clamp(0, 1).view(1, -1).expand(nf, -1)
            assert torch.equal(_call(ops, blank, n_obj, per, geom, truth=False), want)          # zero patches: the clamped background
        # one shared row == that row repeated for every object of every frame
        n_obj, nf = 3, 7
        inp = R.draw_case(5, nf, n_obj, geom, 0)
        rep = dict(inp, patches=np.repeat(inp['patches'], nf * n_obj, axis=0))
        a, sa = _call(ops, inp, n_obj, 0, geom)
        b, sb = _call(ops, rep, n_obj, 1, geom)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        # no frames
        empty = dict(inp, z=np.zeros((0, 4), np.float32), truth=np.zeros((0, C * W * H), np.float32))
        o, s = _call(ops, empty, n_obj, 0, geom)
        assert o.shape == (0, C * W * H) and s.shape == (0,)
        assert _call(ops, empty, n_obj, 0, geom, truth=False).shape == (0, C * W * H)


def test_render_kernel_agrees_with_the_32x32_kernel():
    from stove_amd import ops
    geom = (1, 32, 32, 10, 10, False)
    for n_obj, nf, per in ((3, 65, 1), (8, 10, 5), (1, 4, 0)):
        inp = R.draw_case(900 + n_obj, nf, n_obj, geom, per)
        new = _call(ops, inp, n_obj, per, geom, truth=False)
        old = ops.render_frames(_dev(inp['bg']), _dev(inp['patches']), per, _dev(inp['z']), n_obj)
        assert float((new - old).abs().max()) <= PIX_TOL


# ---------------------------------------------------------------------------------------------------- 3. rejections
def test_render_any_refuses_bad_arguments():
    """Every host-checkable error: a ValueError from the op, hipErrorInvalidValue from the entry point; nothing is launched -- the
    poisoned outputs keep their poison."""
    from stove_amd import _lib, ops
    lib = _lib.load()
    C, W, H, pw, ph, n_obj, nf = 3, 12, 20, 8, 12, 3, 4
    geom = (C, W, H, pw, ph, False)
    inp = R.draw_case(1, nf, n_obj, geom, 1)
    bg, pat, z, truth = (_dev(inp[k]) for k in ('bg', 'patches', 'z', 'truth'))
    for kw in (dict(n_obj=0), dict(n_obj=9), dict(geom=(0,) + geom[1:]), dict(geom=(5,) + geom[1:]), dict(geom=(C, 0, H, pw, ph, False)),
               dict(geom=(C, W, H, pw, -1, False)), dict(per=-1), dict(bg=bg[:-1]), dict(z=z[:, :3]), dict(z=z[:-1]), dict(pat=pat[:-1]),
               dict(truth=truth[:-1]), dict(truth=None, want_frames=False)):
        a = dict(bg=bg, pat=pat, per=1, z=z, n_obj=n_obj, geom=geom, truth=truth, want_frames=True)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.render_frames_any(a['bg'], a['pat'], a['per'], a['z'], a['n_obj'], a['geom'], truth=a['truth'], want_frames=a['want_frames'])
    out = torch.full((nf, C * W * H), -7.0, device=DEV)
    sq = torch.full((nf,), -7.0, device=DEV)
    S = _lib.stream()
    p = _lib.ptr

    def call(**kw):
        a = dict(bg=p(bg), pat=p(pat), per=1, z=p(z), truth=p(truth), out=p(out), sq=p(sq), nf=nf, n_obj=n_obj, C=C, W=W, H=H, pw=pw, ph=ph, ac=0)
        a.update(kw)
        return lib.stove_render_frames_any(*a.values(), S)
    bad = [dict(bg=None), dict(pat=None), dict(z=None), dict(truth=None), dict(sq=None), dict(out=None, sq=None, truth=None),
           dict(n_obj=0), dict(n_obj=9), dict(C=0), dict(C=5), dict(W=0), dict(H=-3), dict(pw=0), dict(ph=0), dict(per=-1), dict(nf=-1)]
    for kw in bad:
        assert call(**kw) == 1, kw                       # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((sq == -7.0).all())
    assert call(nf=0) == 0                               # an empty call is valid and writes nothing
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((sq == -7.0).all())
    assert call() == 0                                   # and the entry point still works
    torch.cuda.synchronize()
    ref = R.render(inp['bg'], inp['patches'], 1, inp['z'], n_obj, geom)
    assert float(np.abs(_np64(out) - ref).max()) <= PIX_TOL and bool((sq > 0).all())


# ---------------------------------------------------------------------------------------------------- 4. reconstruct_from_z
def _cfg(**kw):
    from stove_amd.video_prediction.config import StoveConfig
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = DEV, torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _states(n, T, o, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(n, T, o, 4)
    z[..., 0] = 0.1 + 0.5 * torch.rand(n, T, o, generator=g)
    z[..., 1] = z[..., 0] * (0.75 + 0.5 * torch.rand(n, T, o, generator=g))
    z[..., 2:] = 2.2 * torch.rand(n, T, o, 2, generator=g) - 1.1
    return z.to(DEV)


def test_reconstruct_from_z_colour():
    """A 3-channel 32 x 32 Supair: all three rendering modes against render_ref fed the model's own patches."""
    from stove_amd.video_prediction.supair import Supair
    sup = fill_analytic(Supair(_cfg(channels=3, debug_bw=False)), 'sup.').to(DEV)
    n, T, o = 2, 4, 3
    z = _states(n, T, o, 3)
    x = torch.rand(n, T, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(DEV) ** 2
    geom = sup.render_geom()
    assert geom == (3, 32, 32, 10, 10, False)
    bg = _np64(sup.spn_max_activation(sup.bg_spn))
    assert bg.shape == (3 * 32 * 32,)
    cases = (('max', {}, _np64(sup.spn_max_activation()).reshape(1, -1), 0),
             ('single', dict(x=x[:, 0], max_activation=False, single_image=True), _np64(sup.spn_mpe(z[:, 0], x[:, 0])).reshape(n * o, -1), T),
             ('every', dict(x=x, max_activation=False, single_image=False),
              _np64(sup.spn_mpe(z.flatten(end_dim=1), x.flatten(end_dim=1))).reshape(n * T * o, -1), 1))
    for name, kw, patches, per in cases:
        assert patches.shape[1] == 300 and patches.min() >= 0.0 and patches.max() <= 1.0 and patches.std() > 0, name
        r = sup.reconstruct_from_z(z, **kw)
        assert r.shape == (n, T, 3, 32, 32) and r.dtype == torch.float32
        ref = R.render(bg, patches, per, _np64(z).reshape(-1, 4), o, geom).reshape(n, T, 3, 32, 32)
        gap = float(np.abs(_np64(r) - ref).max())
        print(name, 'pixel gap %.3g' % gap)
        assert gap <= PIX_TOL, name
    # the MPE patches differ between glimpses and between channels (the walk depends on the input)
    assert len(np.unique(cases[2][2].round(5), axis=0)) > 1
    z18 = torch.cat([z, torch.randn(n, T, o, 14, device=DEV)], -1)
    assert torch.equal(sup.reconstruct_from_z(z18), sup.reconstruct_from_z(z))
    with pytest.raises(ValueError):
        sup.reconstruct_from_z(z, max_activation=False)


@pytest.mark.parametrize('res', [32, 50])
def test_reconstruct_from_z_against_the_reference(res):
    from stove_amd.video_prediction.supair import Supair
    g = {k[:-len('_r%d' % res)]: v for k, v in load_golden('g22_pixel_error_f64').items() if k.endswith('_r%d' % res)}
    sup = fill_analytic(Supair(_cfg(width=res, height=res)), 'sup.').to(DEV)
    z, x = _dev(g['z']).float(), _dev(g['x']).float()
    assert float(np.abs(_np64(sup.spn_max_activation(sup.bg_spn)) - g['bg_max']).max()) < 1e-6
    assert float(np.abs(_np64(sup.reconstruct_from_z(z)) - g['recon_max']).max()) <= PIX_TOL
    single = sup.reconstruct_from_z(z, x[:, 0], max_activation=False, single_image=True)
    assert float(np.abs(_np64(single) - g['recon_mpe_single']).max()) <= PIX_TOL
    # the reference's pixel error from the fused sum
    from stove_amd import ops
    n, T = z.shape[:2]
    bg, patches, per = sup.render_inputs(z)
    _, sq = ops.render_frames_any(bg, patches, per, z.reshape(-1, 4).contiguous(), 3, sup.render_geom(), truth=x.reshape(n * T, -1),
                                  want_frames=False)
    bound = R.sqerr_bound(g['recon_max'].reshape(n * T, -1), g['x'].reshape(n * T, -1), PIX_TOL).reshape(n, T).sum(0) / (n * res * res)
    assert (np.abs(_np64(sq).reshape(n, T).sum(0) / (n * res * res) - g['mse']) <= bound).all()


# ---------------------------------------------------------------------------------------------------- 5. / 6. the trainer
def _trainer(tmp_path, colour, tag):
    import model.main as M
    from stove_amd.envs import envs
    d = envs.synth_sequences('billiards', 6, 24)
    data = {'X': np.transpose(d['X'], (0, 1, 3, 4, 2)).astype(np.float64), 'y': d['y'], 'coord_lim': 10, 'r': 1.2}
    path = str(tmp_path / ('billiards_%s.pkl' % tag))
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    args = {'traindata': path, 'testdata': path, 'nolog': 'True', 'experiment_dir': str(tmp_path), 'batch_size': '4',
            'num_visible': '6', 'num_rollout': '4', 'num_workers': '0', 'dtype': 'torch.float', 'random_seed': '42',
            'print_every': '1', 'num_epochs': '1', 'long_rollout_every': '1000000', 'save_every': '1000000'}
    if colour:
        args.update(debug_bw='False', channels='3')
    trainer = M.main(sh_args=args)

    def noise(kind, shape):              # the same draws in every call: the two paths score the same states
        return torch.randn(shape, generator=torch.Generator().manual_seed(zlib.crc32(kind.encode())))
    trainer.stove.noise_fn = noise
    return trainer


@pytest.fixture(scope='module')
def trainers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('pixel_error')
    return {'bw': _trainer(tmp, False, 'bw'), 'colour': _trainer(tmp, True, 'rgb')}


@pytest.mark.parametrize('real_mpe', [False, True])
@pytest.mark.parametrize('linear', [False, True])
@pytest.mark.parametrize('kind', ['bw', 'colour'])
def test_trainer_pixel_error(trainers, kind, linear, real_mpe):
    tr = trainers[kind]
    c, sup = tr.c, tr.stove.sup
    num = 7
    fused = tr.pixel_error(linear=linear, real_mpe=real_mpe, num=num, fused=True)
    frames = tr.pixel_error(linear=linear, real_mpe=real_mpe, num=num, fused=False)
    Tn = c.num_visible - c.skip + num
    for res in (fused, frames):
        assert set(res) == {'mse', 'mse_states'}
        assert res['mse'].shape == (Tn,) and res['mse_states'].shape == (Tn,) and not res['mse'].is_cuda and not res['mse_states'].is_cuda
        assert bool(torch.isfinite(res['mse']).all()) and bool((res['mse'] > 0).all())
    # what was scored: the noise is the same in every call, so the evaluation's own helper returns the states of both calls above (the
    # float64 render of them below has to give the two results)
    tr.stove.eval()
    try:
        z_seq, true, true_states, mpe_image = tr._pixel_error_inputs(linear, real_mpe, num)
        again = tr._pixel_error_inputs(linear, real_mpe, num)[0]
    finally:
        tr.stove.train()
    assert torch.equal(z_seq, again)
    n, C = z_seq.shape[0], c.channels
    assert n == c.batch_size and true.shape == (n, Tn, C, c.width, c.height)
    assert z_seq.shape[-1] == (16 if linear else 18)
    if linear:
        lim = 0.8 if c.coord_lim == 10 else 0.9
        assert float(z_seq[..., 2:4].abs().max()) <= float(np.float32(lim))
    # the float64 render of the same states with the model's own background and patches, and the bound that follows from it
    bg, patches, per = sup.render_inputs(z_seq[..., :4], mpe_image, max_activation=not real_mpe, single_image=True)
    ref = R.render(_np64(bg), _np64(patches).reshape(-1, patches.shape[-1]), per, _np64(z_seq[..., :4]).reshape(-1, 4), c.num_obj, sup.render_geom())
    t64 = _np64(true).reshape(n * Tn, -1)
    P = t64.shape[1]
    assert P == C * c.width * c.height
    mse64 = R.sqerr(ref, t64).reshape(n, Tn).sum(0) / (n * P)
    bound = R.sqerr_bound(ref, t64, PIX_TOL).reshape(n, Tn).sum(0) / (n * P)
    gf, gm, gd = (np.abs(_np64(fused['mse']) - mse64), np.abs(_np64(frames['mse']) - mse64), np.abs(_np64(fused['mse']) - _np64(frames['mse'])))
    print('mse', _np64(fused['mse']).round(5), 'gaps / bound: fused %.3g frames %.3g fused-frames %.3g' % ((gf / bound).max(), (gm / bound).max(), (gd / bound).max()))
    assert (gd <= bound).all() and (gf <= bound).all() and (gm <= bound).all()
    # the position error: the permutation fitted on the first five frames
    pos, lab = _np64(z_seq[..., 2:4]), _np64(true_states[..., :2])
    want5, best5 = R.matched_position_error(pos, lab, 5)
    assert np.abs(_np64(fused['mse_states']) - want5).max() <= 1e-5
    assert torch.equal(fused['mse_states'], frames['mse_states'])
    # prediction_error fits on four frames: the two definitions coincide on the sequences where the fifth frame changes no choice
    _, best4 = R.matched_position_error(pos, lab, 4)
    same = np.flatnonzero(best4 == best5)
    print('sequences on which the four- and the five-frame fit choose the same permutation: %d of %d' % (len(same), n))
    assert len(same) > 0
    rows = torch.from_numpy(same).to(DEV)
    pe = tr.prediction_error(z_seq[rows][..., 2:4], true_states[rows][..., :2], return_velocity=False, return_id_swaps=False, return_full=True)
    assert np.abs(_np64(pe['error']) - R.matched_position_error(pos[same], lab[same], 5)[0]).max() <= 1e-5
    if len(same) == n:
        assert torch.allclose(pe['error'], fused['mse_states'], atol=1e-6)


def test_long_rollout_renders_colour_clips(trainers):
    tr = trainers['colour']
    out = tr.long_rollout(idx=[0, 1], num=5)
    skip, nv = tr.c.skip, tr.c.num_visible
    assert out['frames_real'].shape == (2, nv - skip, 3, 32, 32) and out['frames_real'].dtype == np.uint8
    assert out['frames_recon'].shape == (2, nv - skip, 3, 32, 32) and out['frames_recon'].dtype == np.uint8
    assert out['frames_rollout'].shape == (2, nv - skip + 5, 3, 32, 32) and out['frames_rollout'].dtype == np.uint8
    assert out['frames_recon'].std() > 0 and out['frames_real'].std() > 0
    tr.c.nolog = False
    try:
        from stove_amd.utils.utils import ExperimentLogger
        import os
        tr.logger = ExperimentLogger(tr.c)
        tr.long_rollout(idx=[0], num=3)
        files = sorted(os.listdir(tr.logger.rollout_gifs_dir))
        assert [f.split('.')[0] for f in files] == ['real', 'recon', 'rollout']
        for f in files:
            path = os.path.join(tr.logger.rollout_gifs_dir, f)
            if f.endswith('.npy'):
                assert np.load(path).shape[-1] == 3
            else:
                from PIL import Image
                assert Image.open(path).convert('RGB').size == (32, 32)
    finally:
        tr.c.nolog = True
    # single-channel clips are what they were: one plane, rendered by the 32 x 32 kernel
    bw = trainers['bw']
    out = bw.long_rollout(idx=[0, 1], num=5)
    assert out['frames_rollout'].shape == (2, nv - skip + 5, 1, 32, 32) and out['frames_real'].shape == (2, nv - skip, 1, 32, 32)
    assert (out['frames_rollout'][:, :nv - skip] == out['frames_recon']).all()
