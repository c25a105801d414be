"""Colour frames (config.channels > 1, debug_bw = False; reference supair.py:44-110, probabilistic_models.py:10,27, encoder.py:17): the
fused multi-channel scene likelihood (csrc/scene_colour.hip, stove_scene_fwd_ch / stove_scene_bwd_ch) against the float64 oracle,
against the reference's own op sequence (scene_composed), inside Stove.forward, in training (eager and replayed steps), and the C ABI's
refusals of the new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, fill_analytic
from helpers import oracle_setup, oracle_stove

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _cfg(**kw):
    from stove_amd.video_prediction.config import StoveConfig
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = DEV, torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    cfg.debug = True
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _inputs(h, w, C, n_obj, n=3, T=4, seed=0):
    gen = torch.Generator().manual_seed(1000 + 7 * h + w + 31 * C + n_obj + seed)
    x = torch.rand(n, T + 1, C, h, w, generator=gen)
    z = torch.empty(n * T * n_obj, 4)
    z[:, 0] = 0.12 + 0.3 * torch.rand(z.shape[0], generator=gen)
    z[:, 1] = z[:, 0] * (0.8 + 0.4 * torch.rand(z.shape[0], generator=gen))
    z[:, 2:] = 1.9 * torch.rand(z.shape[0], 2, generator=gen) - 0.95            # some glimpses hang over the frame's edge
    wgt = torch.randn(n * T, generator=gen)
    return x, z, wgt


# (width, height, channels, objects, extra config): frames (.., c, width, height), the last dimension is grid_sample's x
CASES = {
    '32x32_c3_n3': (32, 32, 3, 3, {}),
    '32x32_c3_n6': (32, 32, 3, 6, {}),
    '50x50_c3_n3': (50, 50, 3, 3, {}),
    '32x32_c3_ac_n5': (32, 32, 3, 5, dict(align_corners=True)),
    '40x28_c2_n3': (40, 28, 2, 3, {}),
    '8x12_glimpse_c3': (32, 32, 3, 3, dict(patch_width=8, patch_height=12, obj_spn_num_gauss=7, obj_spn_num_sums=5)),
    '136x24_c3_n2': (136, 24, 3, 2, {}),           # a side past the coverage tables' 128 entries: the mask image is kept
    '32x32_c1_n3': (32, 32, 1, 3, {}),             # one channel through the new entry point (the generic object side)
}


def _run_fused(sup, xs, z, wgt):
    zd = z.to(DEV).requires_grad_()
    # one channel: Supair.likelihood keeps its single-channel routing; the new entry point is reached directly
    lp, prop = sup.likelihood(xs, zd) if sup.c.channels > 1 else sup._likelihood_colour(xs, zd)
    (lp * wgt.to(DEV)).sum().backward()
    return lp.detach(), zd.grad.clone(), {k: float(v) for k, v in prop.items() if k in ('bg', 'patch', 'overlap')}


def _colour_supair(C, extra, regime, **kw):
    from stove_amd.video_prediction.supair import Supair
    sup = Supair(_cfg(channels=C, debug_bw=False, **extra, **kw))
    if sup.obj_spn._kind == 'obj':
        sup.obj_spn._force_general_plan()          # one channel, 10 x 10 glimpses: the generic object SPN the new entry point takes
    sup = fill_analytic(sup, 'sup.', regime=regime).to(DEV)
    sup.step_counter = 0                 # a logging step: the parts' means are exported
    return sup


@pytest.mark.parametrize('regime', ['analytic', 'init'])
@pytest.mark.parametrize('case', list(CASES))
def test_fused_colour_scene_against_the_oracle(case, regime):
    """The fused colour pipeline against O.scene_likelihood with config.channels = C: log p, its three parts, dz and every SPN
    parameter gradient; frames handed over as the x[:, 1:] view; a second run bit for bit."""
    from stove_amd import ops
    h, w, C, n_obj, extra = CASES[case]
    sup = _colour_supair(C, extra, regime, width=h, height=w, num_obj=n_obj)
    assert sup.obj_spn._kind == 'obj_any' and sup.bg_spn._kind == 'bg' and sup.bg_spn.num_dims == C * h * w
    x, z, wgt = _inputs(h, w, C, n_obj)
    xs = x.to(DEV)[:, 1:]
    calls = []
    orig = ops._SceneChFn.apply
    ops._SceneChFn.apply = lambda *a: calls.append(1) or orig(*a)
    try:
        lp, gz, parts = _run_fused(sup, xs, z, wgt)
    finally:
        ops._SceneChFn.apply = orig
    assert calls, 'the fused colour path was not taken'
    cfg, structs, params = oracle_setup(torch.float64, regime=regime, num_obj=n_obj, width=h, height=w, channels=C, debug_bw=False, **extra)
    params = {k: v for k, v in params.items() if k.startswith('sup.')}
    z64 = z.double().requires_grad_()
    ref, bg_o, pl_o, ov_o = O.scene_likelihood(cfg, params, structs, x[:, 1:].double(), z64, parts=True)
    (ref * wgt.double()).sum().backward()
    check('colour.log_p', err(lp, ref), 6e-6)
    for k, v in (('bg', bg_o), ('patch', pl_o), ('overlap', ov_o)):
        m = float(v.detach().mean())
        check('colour.part_' + k, abs(parts[k] - m) / (abs(m) + 1e-9), 6e-6)
    check_grad('colour.dz', gz, z64.grad, 3e-4, 3e-4, 5e-3)
    got = dict(sup.named_parameters())
    n = 0
    for k, v in params.items():
        if v.grad is not None and float(v.grad.abs().max()) > 0:
            check_grad('colour.grad', got[k[4:]].grad, v.grad, 3e-4, 3.5e-4, 1.5e-2)
            n += 1
    assert n >= 6
    sup.zero_grad()
    lp2, gz2, _ = _run_fused(sup, xs, z, wgt)
    assert torch.equal(lp, lp2) and torch.equal(gz, gz2)


@pytest.mark.parametrize('case', ['32x32_c3_n3', '32x32_c3_ac_n5', '8x12_glimpse_c3'])
def test_fused_colour_scene_equals_the_composed_one(case):
    """scene_composed = True (the reference's op sequence on ATen's sampler + the HIP SPN operators) against the fused path on the
    same colour inputs: log p, dz and every parameter gradient."""
    h, w, C, n_obj, extra = CASES[case]
    x, z, wgt = _inputs(h, w, C, n_obj, seed=1)
    xs = x.to(DEV)[:, 1:]
    out = []
    for composed in (False, True):
        sup = _colour_supair(C, extra, 'analytic', width=h, height=w, num_obj=n_obj, scene_composed=composed)
        lp, gz, _ = _run_fused(sup, xs, z, wgt)
        out.append((lp, gz, {k: p.grad.clone() for k, p in sup.named_parameters() if p.grad is not None}))
    (lp0, gz0, g0), (lp1, gz1, g1) = out
    # two float32 implementations, each held to the float64 oracle at the bars of the test above: twice those bars between them
    check('colour.composed.log_p', err(lp0, lp1), 1.2e-5)
    check_grad('colour.composed.dz', gz0, gz1, 6e-4, 6e-4, 1e-2)
    assert set(g0) == set(g1) and len(g0) >= 6
    for k in g0:
        check_grad('colour.composed.grad', g0[k], g1[k], 6e-4, 7e-4, 3e-2)


def test_colour_frames_are_checked_against_the_config():
    sup = _colour_supair(3, {}, 'analytic')
    x, z, _ = _inputs(32, 32, 3, 3)
    with pytest.raises(ValueError):
        sup.likelihood(x[:, 1:, :1].to(DEV), z.to(DEV))          # one plane for a three-channel model
    from stove_amd.video_prediction.stove import Stove
    with pytest.raises(ValueError, match='debug_bw'):
        Stove(_cfg(channels=3, debug_bw=True))


@pytest.mark.parametrize('objects', [(3, '3_only'), (6, 'greedy')])
@pytest.mark.parametrize('arena', [False, True])
def test_stove_forward_on_colour_frames_against_the_oracle(objects, arena):
    """Stove.forward with debug_bw = False, channels = 3 against the float64 oracle's training step: ELBO, the state props, every
    parameter gradient, with the flat parameter arena off and on (the SPN tables of the colour model are baked per tensor)."""
    from stove_amd.arena import ParamArena
    from stove_amd.envs import envs
    from stove_amd.video_prediction.stove import Stove
    n_obj, match = objects
    kw = dict(num_obj=n_obj, debug_match_objects=match, channels=3, debug_bw=False)
    st = fill_analytic(Stove(_cfg(**kw))).to(DEV)
    if arena:
        ar = ParamArena(st)
        assert ar.has_gnn and not ar.has_spn
    B, T = 3, 8
    x = torch.from_numpy(envs.synth_sequences('billiards' if n_obj == 3 else 'multibilliards', B, T, seed0=3)['X']).float()
    assert x.shape[2] == 3
    eps = O.draw_eps(B, n_obj, T, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    table = {'latent': eps['latent'][..., 0].float(), 'std': eps['std'][..., 0].float(), 'steps': torch.stack(eps['steps'], 1).float()}
    st.noise_fn = lambda kind, shape: table[kind].reshape(shape).to(DEV)
    elbo, prop, _ = st(x.to(DEV), 0, None)
    (-elbo).backward()
    ref = oracle_stove(kw, x.double(), eps)
    check('colour.stove.elbo_rel', abs(float(elbo) - float(ref['elbo'])) / abs(float(ref['elbo'])), 1.5e-6)
    for k in ('z', 'z_sup', 'log_q'):
        check('colour.stove.prop_' + k, err(prop[k], ref['info'][k]), 8e-6)
    params = dict(st.named_parameters())
    n = 0
    for k, g in ref['grads'].items():
        if float(g.abs().max()) > 0:
            check_grad('colour.stove.grad', params[k].grad, g, 3e-4, 3.5e-4, 1.5e-2)
            n += 1
    assert n > 30


def _colour_batches(n_seq, T, n_steps):
    from stove_amd.envs import envs
    d = envs.synth_sequences('billiards', n_seq * 2, T + n_steps, seed0=5)
    return [torch.from_numpy(d['X'][(s % 2) * n_seq:(s % 2) * n_seq + n_seq, s:s + T]).to(DEV).contiguous() for s in range(n_steps)]


def _colour_steps(batches, graphed):
    from stove_amd.arena import ParamArena
    from stove_amd.graphed import GraphedTrainStep
    from stove_amd.optim import FlatAdam
    from stove_amd.video_prediction.stove import Stove
    cfg = _cfg(channels=3, debug_bw=False)
    cfg.print_every, cfg.plot_every, cfg.debug = 10 ** 9, 1e19, False
    torch.manual_seed(0)
    model = Stove(cfg).to(DEV)
    table = {}

    def noise(kind, shape):
        key = (kind, tuple(shape))
        if key not in table:
            table[key] = torch.randn(shape, generator=torch.Generator().manual_seed(len(table) + 5)).to(DEV)
        return table[key]
    model.noise_fn = noise
    arena = ParamArena(model, 1)
    opt = FlatAdam(arena, lr=cfg.learning_rate, amsgrad=True)
    step = GraphedTrainStep(model, arena, opt, clip=1.0)
    out = []
    for x in batches:
        e = step(x, None, None) if graphed else step.eager(x, None, None)
        torch.cuda.synchronize()
        out.append((e.clone(), arena.grad.clone(), arena.data.clone()))
    if graphed:
        assert step.graphs is not None
    return out


def test_replayed_colour_step_equals_the_eager_step_bitwise():
    batches = _colour_batches(6, 9, 3)
    ref = _colour_steps(batches, graphed=False)
    got = _colour_steps(batches, graphed=True)
    for i, ((e0, g0, p0), (e1, g1, p1)) in enumerate(zip(ref, got)):
        assert torch.isfinite(e0) and float(g0.abs().max()) > 0
        assert torch.equal(e0, e1), ('elbo', i, float(e0), float(e1))
        assert torch.equal(g0, g1), ('gradient arena', i, float((g0 - g1).abs().max()))
        assert torch.equal(p0, p1), ('parameters', i)
    assert not torch.equal(ref[0][2], ref[-1][2])


def test_training_on_colour_billiards(tmp_path):
    """run_stove.py's path (model.main.main -> Trainer.train) with debug_bw = False, channels = 3: eager logging steps and replayed
    steps on colour frames; the parameters stay finite and move."""
    import pickle
    import model.main as M
    from stove_amd.envs import envs
    d = envs.synth_sequences('billiards', 6, 20)
    data = {'X': np.transpose(d['X'], (0, 1, 3, 4, 2)).astype(np.float64), 'y': d['y'], 'coord_lim': 10, 'r': 1.2}
    path = str(tmp_path / 'billiards_rgb.pkl')
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    args = {'traindata': path, 'testdata': path, 'nolog': 'True', 'experiment_dir': str(tmp_path), 'batch_size': '4',
            'num_visible': '6', 'num_rollout': '4', 'num_workers': '0', 'dtype': 'torch.float', 'random_seed': '42',
            'print_every': '4', 'num_epochs': '1', 'long_rollout_every': '1000000', 'save_every': '1000000',
            'debug_bw': 'False', 'channels': '3'}
    trainer = M.main(sh_args=args)
    assert trainer.c.channels == 3 and not trainer.c.debug_bw and trainer.stove.sup.bg_spn.num_dims == 3 * 32 * 32
    before = trainer.bucket.data.clone()
    trainer.train()
    assert trainer.optimizer._steps == len(trainer.dataloader) and trainer.optimizer._steps >= 8
    assert trainer._graphed is not None and trainer._graphed.graphs is not None          # non-logging steps were replayed
    assert torch.isfinite(trainer.bucket.data).all() and not torch.equal(before, trainer.bucket.data)


def test_colour_scene_entry_points_refuse_bad_arguments():
    """stove_scene_fwd_ch / stove_scene_bwd_ch: channels outside 1..4, D != channels * pw * ph, a background table of the wrong size,
    too many objects and null pointers come back as hipErrorInvalidValue before anything is launched."""
    from stove_amd import _lib
    lib = _lib.load()
    inval = 1
    C, W, H, pw, ph, n_obj, nf = 3, 32, 32, 10, 10, 3, 2
    R, G, S, Lmax = 6, 10, 10, 75
    D = C * pw * ph
    buf = torch.zeros(1 << 20, device=DEV)
    p = buf.data_ptr()
    bgf = 3 * C * W * H * 6 * 3
    stream = torch.cuda.current_stream().cuda_stream

    def fwd(**kw):
        a = dict(lscope=p, slot=p, coef=p, wsum=p, wroot=p, R=R, G=G, S=S, D=D, Lmax=Lmax, bg_side=p, bg_coef=p, bg_wroot=p, bgf=bgf,
                 frames=p, z=p, nf=nf, n_obj=n_obj, sf=0, ss=0, C=C, W=W, H=H, pw=pw, ph=ph, ac=0, beta=0.1, ll=p, parts=p, saved=p)
        a.update(kw)
        return lib.stove_scene_fwd_ch(*a.values(), stream, 1)

    def bwd(**kw):
        a = dict(lscope=p, slot=p, coef=p, wsum=p, wroot=p, R=R, G=G, S=S, D=D, Lmax=Lmax, bg_side=p, bg_coef=p, bg_wroot=p, bgf=bgf,
                 frames=p, z=p, nf=nf, n_obj=n_obj, sf=0, ss=0, C=C, W=W, H=H, pw=pw, ph=ph, ac=0, beta=0.1, saved=p, dll=p, dz=p,
                 gc=p, gw=p, gr=p, gbc=p, gbr=p, ws=p)
        a.update(kw)
        return lib.stove_scene_bwd_ch(*a.values(), stream, None)

    for f in (fwd, bwd):
        assert f(C=0, D=0 * pw * ph, bgf=0) == inval
        assert f(C=5, D=5 * pw * ph, bgf=3 * 5 * W * H * 18) == inval
        assert f(D=D - 1) == inval
        assert f(bgf=bgf - 18) == inval
        assert f(n_obj=9) == inval and f(n_obj=0) == inval
        assert f(R=9) == inval and f(G=17) == inval
        assert f(frames=None) == inval and f(z=None) == inval and f(lscope=None) == inval and f(bg_coef=None) == inval
    assert fwd(ll=None) == inval and fwd(saved=None) == inval
    assert bwd(slot=None) == inval and bwd(ws=None) == inval and bwd(dz=None) == inval and bwd(gbc=None) == inval
    assert fwd(nf=0) == 0 and bwd(nf=0) == 0
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                     # nothing was launched
    assert ctypes.sizeof(ctypes.c_size_t) == 8
