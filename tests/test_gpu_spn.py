"""GPU parity tests of the SPN / scene HIP kernels against the CPU oracle (fp64) and the
reference-generated goldens.  Tolerances are pinned a few times above what the kernels achieve on an MI355X
(tests/gpu_helpers.check records the worst case of every key): forward values 5e-6 relative (north_star bar: 1e-4),
gradients 3e-4 relative to the largest entry -- the reference's own fp32-vs-fp64 gradient gap."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, fill_analytic, ref_gap, regime_bar
from helpers import load_golden, oracle_setup, t_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FWD_TOL, GRAD_TOL = 5e-6, 3e-4       # achieved on MI355X: 8.9e-7 / 8.7e-5 (gpurun_out/parity_errors.json)


def test_wave_sum_dpp():
    from stove_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64 * 64, generator=g).to(DEV)
    out = ops.wave_sum_selftest(x).view(64, 64).cpu()
    ref = x.view(64, 64).double().sum(1, keepdim=True).expand(-1, 64).cpu()
    assert err(out, ref) < 1e-5
    # exact on small integers: every lane must carry the same total
    xi = torch.randint(-8, 8, (16 * 64,), generator=g).float().to(DEV)
    oi = ops.wave_sum_selftest(xi).view(16, 64).cpu()
    assert torch.equal(oi, xi.view(16, 64).sum(1, keepdim=True).expand(-1, 64).cpu())


def _spn_pair(kind):
    from stove_amd.spn import probabilistic_models as prob
    c, structs, params = oracle_setup(torch.float64)
    spn = (prob._get_obj_spn if kind == 'obj' else prob._get_bg_spn)(c, 42)
    fill_analytic(spn, f'sup.{kind}_spn.')
    return c, structs, params, spn.to(DEV)


def _oracle_spn(kind, c, structs, params, x, m):
    if kind == 'obj':
        args = (c.obj_spn_num_gauss, c.obj_spn_num_sums, c.obj_min_var, c.obj_max_var)
    else:
        args = (6, 3, c.bg_min_var, c.bg_max_var)
    return O.spn_forward(structs[kind], params, f'sup.{kind}_spn.', x, m, *args)


@pytest.mark.parametrize('kind', ['obj', 'bg'])
@pytest.mark.parametrize('n', [8, 1, 64, 65, 200])
def test_ratspn_operator(kind, n):
    c, structs, params, spn = _spn_pair(kind)
    d = spn.num_dims
    g = torch.Generator().manual_seed(n)
    if n == 8:
        gold = load_golden(f'g2_ratspn_{kind}_f32')
        x64, m64 = t_(gold['x']), t_(gold['marg'])
    else:
        x64 = torch.rand(n, d, generator=g, dtype=torch.float64)
        m64 = torch.rand(n, d, generator=g, dtype=torch.float64) * 1.4 - 0.2
        m64[0] = 0.0
    wsum = torch.linspace(0.5, 1.5, n, dtype=torch.float64)
    x_o, m_o = x64.clone().requires_grad_(), m64.clone().requires_grad_()
    out_o = _oracle_spn(kind, c, structs, params, x_o, m_o)
    (out_o[:, 0] * wsum).sum().backward()

    x_d = x64.float().to(DEV).requires_grad_()
    m_d = m64.float().to(DEV).requires_grad_()
    out_d = spn(x_d, m_d)
    assert out_d.shape == (n, 1)
    check('spn.fwd', err(out_d, out_o), FWD_TOL)
    (out_d[:, 0] * wsum.float().to(DEV)).sum().backward()
    check('spn.grad', err(x_d.grad, x_o.grad), GRAD_TOL)
    check('spn.grad', err(m_d.grad, m_o.grad), GRAD_TOL)
    for name, p in spn.named_parameters():
        if name.startswith('output_vector'):
            continue
        check_grad('spn.grad_param', p.grad, params[f'sup.{kind}_spn.' + name].grad, GRAD_TOL, 2.5e-4, 5e-3)
    if n == 8:   # also against the reference's own fp32 outputs
        check('spn.fwd', err(out_d, gold['out']), FWD_TOL)
        out_nm = spn(x_d.detach(), None)
        check('spn.fwd', err(out_nm, gold['out_nomarg']), FWD_TOL)


def test_ratspn_operator_empty_batch():
    c, structs, params, spn = _spn_pair('obj')
    out = spn(torch.zeros(0, 100, device=DEV), None)
    assert out.shape == (0, 1)


def test_ratspn_bitwise_reproducible():
    c, structs, params, spn = _spn_pair('obj')
    g = torch.Generator().manual_seed(5)
    x = torch.rand(300, 100, generator=g).to(DEV)
    m = torch.rand(300, 100, generator=g).to(DEV)
    outs, grads = [], []
    for _ in range(2):
        spn.zero_grad()
        xx = x.clone().requires_grad_()
        o = spn(xx, m)
        o.sum().backward()
        outs.append(o.detach().clone())
        grads.append([p.grad.clone() for p in spn.parameters()] + [xx.grad.clone()])
    assert torch.equal(outs[0], outs[1])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def _supair_pair(n_obj, regime='analytic', **extra):
    from stove_amd.video_prediction.supair import Supair
    from stove_amd.video_prediction.config import StoveConfig
    c, structs, params = oracle_setup(torch.float64, regime=regime, num_obj=n_obj, **extra)
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = n_obj, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = torch.device(DEV), torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    for k, v in extra.items():
        setattr(cfg, k, v)
    sup = fill_analytic(Supair(cfg), 'sup.', regime).to(DEV)
    return c, structs, params, sup


def gname(stem, regime):
    """fixture of a weight regime (tests/golden/analytic_weights.py): the round-1 'analytic' files carry no infix"""
    return f'{stem}_f64' if regime == 'analytic' else f'{stem}_{regime}_f64'


@pytest.mark.parametrize('n_obj,extra', [(3, {}), (6, {'overlap_beta': 100.0, 'max_obj_scale': 0.22})])
@pytest.mark.parametrize('regime', ['analytic', 'init', 'stress'])
def test_scene_likelihood_vs_reference_golden(n_obj, extra, regime):
    """Supair.likelihood against the reference's own numbers in three weight regimes: smooth mid-range weights, the reference's
    initial statistics, and a saturated model (leaf variances at their bounds, near one-hot sum weights)."""
    gold = load_golden(gname(f'g4_likelihood_n{n_obj}', regime))
    c, structs, params, sup = _supair_pair(n_obj, regime, **extra)
    x = t_(gold['x']).float().to(DEV)
    z = t_(gold['z']).float().to(DEV).requires_grad_()
    sup.step_counter = 0
    lp, prop = sup.likelihood(x, z)
    check('spn.fwd', err(lp, gold['log_p']), FWD_TOL)
    for k in ('bg', 'patch', 'overlap'):
        assert abs(float(prop[k]) - float(gold[k])) < FWD_TOL * abs(float(gold[k])) + 1e-6, k
    (lp * t_(gold['w']).float().to(DEV)).sum().backward()
    # gradients: the 'analytic' bars, or 6x the reference's own float32-vs-float64 gap on this fixture where a saturated model
    # amplifies float32 rounding beyond them (six objects, 'stress': the reference's float32 dz is 1.0e-4 off its float64 one)
    case = f'g4_n{n_obj}_{regime}'
    tag = '' if regime == 'analytic' else '.' + regime
    check('spn.grad' + tag, err(z.grad, gold['gz']), regime_bar(GRAD_TOL, ref_gap(case, 'gz')))
    n = 0
    for k, v in gold.items():
        if k.startswith('g_') and 'encoder' not in k:
            p = dict(sup.named_parameters())[k[2:]]
            check_grad('spn.grad_param' + tag, p.grad, v, regime_bar(GRAD_TOL, ref_gap(case, 'grad_param', 'max')),
                       regime_bar(2.5e-4, ref_gap(case, 'grad_param', 'l2')), regime_bar(8e-3 if regime == 'stress' else 5e-3, ref_gap(case, 'grad_param', 'small')))   # stress, six objects: 5.5e-3 on the smallest entries of two background leaf tensors
            n += 1
    assert n > 60


@pytest.mark.parametrize('n_obj', [3, 6, 1, 2])
def test_scene_likelihood_vs_oracle_ragged(n_obj):
    """n_frames not a multiple of the 64-sample tile, random and degenerate z."""
    extra = {'debug_match_objects': 'greedy'} if n_obj != 3 else {}
    c, structs, params, sup = _supair_pair(n_obj, **extra)
    g = torch.Generator().manual_seed(11 + n_obj)
    nb, t = 5, 9
    x64 = torch.rand(nb, t, 1, 32, 32, generator=g, dtype=torch.float64) ** 2
    z64 = torch.zeros(nb * t, n_obj, 4, dtype=torch.float64)
    z64[..., 0] = 0.1 + 0.6 * torch.rand(nb * t, n_obj, generator=g, dtype=torch.float64)
    z64[..., 1] = z64[..., 0] * (0.75 + 0.5 * torch.rand(nb * t, n_obj, generator=g, dtype=torch.float64))
    z64[..., 2:] = 1.9 * torch.rand(nb * t, n_obj, 2, generator=g, dtype=torch.float64) - 0.95
    z64[0, :, 2:] = z64[0, 0:1, 2:]                     # every object on top of the first
    z64 = z64.flatten(0, 1)
    w = torch.linspace(0.5, 1.5, nb * t, dtype=torch.float64)
    z_o = z64.clone().requires_grad_()
    lp_o, bg_o, pl_o, ov_o = O.scene_likelihood(c, params, structs, x64, z_o, parts=True)
    (lp_o * w).sum().backward()
    z_d = z64.float().to(DEV).requires_grad_()
    sup.step_counter = 0
    lp_d, prop = sup.likelihood(x64.float().to(DEV), z_d)
    check('spn.fwd', err(lp_d, lp_o), FWD_TOL)
    assert abs(float(prop['bg']) - float(bg_o.mean())) < FWD_TOL * abs(float(bg_o.mean())) + 1e-6
    (lp_d * w.float().to(DEV)).sum().backward()
    check('spn.grad', err(z_d.grad, z_o.grad), GRAD_TOL)
    for name, p in sup.named_parameters():
        if 'encoder' in name or name.endswith('output_vector.params'):
            continue
        check_grad('spn.grad_param', p.grad, params['sup.' + name].grad, GRAD_TOL, 2.5e-4, 5e-3)


@pytest.mark.parametrize('n_obj', [3, 6])
def test_scene_forward_with_and_without_the_unit_backward(n_obj):
    """The training forward runs the object SPN forward + backward at unit upstream gradient in one kernel
    (objspn_fwd_unit_k, csrc/spn_obj.hip) and leaves the backward scratch in `saved`; without a backward to come the plain
    forward kernel runs and `saved` is smaller: the likelihood and its parts must be the same bit for bit."""
    from stove_amd import _lib
    extra = {'debug_match_objects': 'greedy'} if n_obj != 3 else {}
    c, structs, params, sup = _supair_pair(n_obj, **extra)
    g = torch.Generator().manual_seed(23 + n_obj)
    nb, t = 3, 15                                       # 45 frames: ragged 64-glimpse batches
    x = (torch.rand(nb, t, 1, 32, 32, generator=g) ** 2).to(DEV)
    z = torch.zeros(nb * t * n_obj, 4)
    z[:, 0] = 0.1 + 0.5 * torch.rand(nb * t * n_obj, generator=g)
    z[:, 1] = z[:, 0] * (0.75 + 0.5 * torch.rand(nb * t * n_obj, generator=g))
    z[:, 2:] = 1.8 * torch.rand(nb * t * n_obj, 2, generator=g) - 0.9
    z = z.to(DEV)
    lib = _lib.load()
    assert lib.stove_scene_fwd_floats(nb * t, n_obj, 0) < lib.stove_scene_fwd_floats(nb * t, n_obj, 1) == lib.stove_scene_saved_floats(nb * t, n_obj)
    sup.step_counter = 0
    lp_g, prop_g = sup.likelihood(x, z.clone().requires_grad_())
    with torch.no_grad():
        lp_n, prop_n = sup.likelihood(x, z)
    assert lp_g.requires_grad and not lp_n.requires_grad
    assert torch.equal(lp_g.detach(), lp_n)
    for k in prop_n:
        assert torch.equal(torch.as_tensor(prop_g[k]).detach(), torch.as_tensor(prop_n[k])), k


@pytest.mark.parametrize('n_obj', [3, 6])
def test_scene_backward_with_parameter_stream(n_obj):
    """stove_scene_bwd_overlap (table gradients on a second stream: for N <= 4 held back and computed by the one-wave-per-SIMD
    objspn_tablegrad_under_k, csrc/spn_obj.hip; the background GEMM's coefficient image handed over, stove_bg_dense) against
    stove_scene_bwd (one stream, objspn_tablegrad_k) on the same inputs: same likelihood, dz and table gradients."""
    from stove_amd import ops, _lib
    extra = {'debug_match_objects': 'greedy'} if n_obj != 3 else {}
    c, structs, params, sup = _supair_pair(n_obj, **extra)
    g = torch.Generator().manual_seed(5 + n_obj)
    nf = 5462                                            # 16 386 / 32 772 glimpses (>= kLateTableGradGlimpses), ragged 64-glimpse batches
    frames = (torch.rand(nf, 1024, generator=g) ** 2).to(DEV)
    z = torch.zeros(nf, n_obj, 4)
    z[..., 0] = 0.1 + 0.6 * torch.rand(nf, n_obj, generator=g)
    z[..., 1] = z[..., 0] * (0.75 + 0.5 * torch.rand(nf, n_obj, generator=g))
    z[..., 2:] = 1.9 * torch.rand(nf, n_obj, 2, generator=g) - 0.95
    z = z.flatten(0, 1).to(DEV)
    w = torch.linspace(0.5, 1.5, nf).to(DEV)
    obj_tabs = tuple(t.detach() for t in sup.obj_spn.tables())
    bg_tabs = tuple(t.detach() for t in sup.bg_spn.tables())
    # (a) one stream, gradients through autograd
    leaves = [t.clone().requires_grad_() for t in (*obj_tabs[:3], *bg_tabs[:2])]
    za = z.clone().requires_grad_()
    ll_a, _ = ops.scene_likelihood(frames, za, (*leaves[:3], *obj_tabs[3:]), (*leaves[3:], bg_tabs[2]), n_obj, c.overlap_beta)
    (ll_a * w).sum().backward()
    # (b) parameter stream + sink, coefficient image made ahead of time
    lib = _lib.load()
    dense = torch.empty(lib.stove_bg_dense_floats(), dtype=torch.float32, device=DEV)
    _lib.check(lib.stove_bg_dense(bg_tabs[2].data_ptr(), bg_tabs[0].data_ptr(), dense.data_ptr(), _lib.stream()), 'stove_bg_dense')
    got = []
    zb = z.clone().requires_grad_()
    ll_b, _ = ops.scene_likelihood(frames, zb, obj_tabs, (*bg_tabs, dense), n_obj, c.overlap_beta, sink=lambda gr: got.extend(t.clone() for t in gr))
    (ll_b * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ll_a, ll_b)
    assert err(zb.grad, za.grad) < 1e-6
    assert len(got) == 5
    for a, b in zip(leaves, got):
        assert err(b.view_as(a), a.grad) < 1e-5, (a.shape, err(b.view_as(a), a.grad))


@pytest.mark.parametrize('n_obj', [3, 6])
def test_glimpses_and_masks(n_obj):
    gold = load_golden(f'g3_scene_n{n_obj}')
    c, structs, params, sup = _supair_pair(n_obj, **({'debug_match_objects': 'greedy'} if n_obj == 6 else {}))
    z = t_(gold['z']).float().to(DEV)
    x = t_(gold['x']).float().to(DEV)
    pat = sup.patches_from_z(x, z.flatten(0, 1))
    assert pat.shape == gold['patches'].shape
    assert err(pat, gold["patches"]) < 1e-4
    mp, bgm, ov = sup.masks_from_z(z)
    assert err(mp, gold["marg_patch"]) < 1e-4
    assert err(bgm, gold["bg_mask"]) < 1e-4
    assert err(ov, gold["overlap"]) < 1e-4


@pytest.mark.parametrize('n_obj', [3, 6])
def test_scene_glimpse_kernel(n_obj):
    """The closed-form tile kernel (glimpse + occlusion mask) against the reference's sequential masks."""
    from stove_amd import ops
    gold = load_golden(f'g3_scene_n{n_obj}')
    z = t_(gold['z']).float().to(DEV)
    x = t_(gold['x']).float().to(DEV)
    pat, keep = ops.scene_glimpses(x.flatten(1), z.flatten(0, 1), n_obj)
    assert err(pat, gold['patches'].reshape(-1, 100)) < 1e-5
    marg = np.clip(gold['marg_patch'].reshape(-1, 100), 0, 1)
    assert err(1.0 - keep, marg) < 1e-5


@pytest.mark.parametrize('n_obj,nf', [(3, 64), (3, 2301), (6, 130), (4, 77), (8, 40), (2, 50), (1, 9)])
def test_glimpse_tile_kernel_lds_staging_is_bit_identical(n_obj, nf):
    """scene_tile_fwd_t_k (stove_set_tile_lds mode 2: lane = pixel, the tile transposed through LDS, for every object count) against
    scene_tile_fwd_k (mode 0: lane = glimpse, global gathers; the kernel the goldens were first met with): glimpses and keep-weights
    bit for bit -- ragged last batches, objects leaving the frame, every object count."""
    from stove_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(nf + n_obj)
    frames = torch.rand(nf, 1024, generator=g).to(DEV)
    z = torch.rand(nf * n_obj, 4, generator=g)
    z[:, :2] = z[:, :2] * 0.7 + 0.1
    z[:, 2:] = z[:, 2:] * 2.4 - 1.2                  # some glimpses hang over the border
    z = z.to(DEV).contiguous()
    outs = []
    for mode in (0, 2):
        lib.stove_set_tile_lds(mode)
        tile = torch.full((lib.stove_objspn_tile_floats(nf * n_obj),), float('nan'), device=DEV)
        pat = torch.empty(nf * n_obj, 100, device=DEV)
        keep = torch.empty(nf * n_obj, 100, device=DEV)
        _lib.check(lib.stove_scene_glimpses(_lib.ptr(frames), _lib.ptr(z), nf, n_obj, _lib.ptr(tile), _lib.ptr(pat), _lib.ptr(keep), _lib.stream()),
                   'stove_scene_glimpses')
        torch.cuda.synchronize()
        outs.append((pat.clone(), keep.clone()))
    lib.stove_set_tile_lds(1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].abs().max()) > 0 and torch.isfinite(outs[1][1]).all()


def test_scene_forward_on_strided_clips_is_the_same_with_either_tile_kernel():
    """stove_scene_fwd on frames x[:, 1:] of longer clips handed over without a copy (seq_frames / seq_stride), LDS-staged against
    gathered tiles: identical log-likelihoods."""
    from stove_amd import _lib
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.supair import Supair
    lib = _lib.load()
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = torch.device(DEV), torch.float32, 42
    sup = Supair(cfg).to(DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(7, 9, 1, 32, 32, generator=g).to(DEV)
    z = torch.rand(7, 8, 3, 4, generator=g)
    z[..., :2] = z[..., :2] * 0.6 + 0.15
    z[..., 2:] = z[..., 2:] * 1.8 - 0.9
    z = z.to(DEV)
    res = []
    for mode in (0, 2):
        lib.stove_set_tile_lds(mode)
        with torch.no_grad():
            ll, _ = sup.likelihood(x[:, 1:], z.reshape(-1, 4))
        res.append(ll.clone())
    lib.stove_set_tile_lds(1)
    assert torch.equal(res[0], res[1])
