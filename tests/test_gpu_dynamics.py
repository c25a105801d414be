"""GPU parity tests of the GNN step, the object matchers, the fused inference recursion, the
full Stove.forward (ELBO + gradients) and Stove.rollout against reference-generated goldens."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, fill_analytic, ref_gap, regime_bar
from helpers import load_golden, oracle_setup, reference_at_codes, source_index, t_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def make_cfg(**kw):
    from stove_amd.video_prediction.config import StoveConfig
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = torch.device(DEV), torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    cfg.debug = True
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


VARIANTS = {
    'plain3': dict(num_obj=3), 'plain6': dict(num_obj=6),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
    'lim4': dict(num_obj=3),
}


def gname(stem, regime):
    """fixture of a weight regime (tests/golden/analytic_weights.py): the round-1 'analytic' files carry no infix"""
    return f'{stem}_f64' if regime == 'analytic' else f'{stem}_{regime}_f64'


REGIME_ARENA = [('analytic', False), ('analytic', True), ('init', True), ('stress', True), ('stress', False)]


@pytest.mark.parametrize('name', list(VARIANTS))
@pytest.mark.parametrize('regime,arena', REGIME_ARENA)
def test_dynamics_step(name, regime, arena):
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.dynamics import Dynamics
    gold = load_golden(gname(f'g5_dynamics_{name}', regime))
    dyn = fill_analytic(Dynamics(make_cfg(**VARIANTS[name])), 'dyn.', regime).to(DEV)
    if arena:
        assert ParamArena(dyn).has_gnn
    s = t_(gold['s']).float().to(DEV).requires_grad_()
    act = t_(gold['actions']).float().to(DEV) if 'actions' in gold else None
    app = t_(gold['app']).float().to(DEV).requires_grad_() if 'app' in gold else None
    res, rew = dyn(s, 0, act, app, lim_enc=int(gold['lim_enc']))
    check('dyn_step.result', err(res, gold['result']), 2e-6)
    loss = (res * t_(gold['w']).float().to(DEV)).sum()
    if act is not None:
        check('dyn_step.reward', err(rew, gold['reward']), 1e-6)
        loss = loss + (rew * torch.linspace(1, 2, s.shape[0], device=DEV).view(-1, 1)).sum()
    loss.backward()
    check('dyn_step.grad_s', err(s.grad, gold['gs']), 5e-6)
    if app is not None:
        check('dyn_step.grad_app', err(app.grad, gold['gapp']), 1e-5)
    params = dict(dyn.named_parameters())
    n = 0
    for k, v in gold.items():
        if k.startswith('g_'):
            assert params[k[2:]].grad is not None, k
            # ('stress': the entry-wise bar follows the reference's own float32 run, whose small entries are 1.7e-3 off its float64 ones)
            gp = lambda m: ref_gap(f'g5_{name}_{regime}', 'grad_param', m)
            check_grad('dyn_step.grad_param' + ('' if regime == 'analytic' else '.' + regime), params[k[2:]].grad, v,
                       regime_bar(2.5e-5, gp('max')), regime_bar(2e-5, gp('l2')), regime_bar(1e-3, gp('small')))
            n += 1
    assert n >= 26


def test_dynamics_step_ragged_batches_and_reproducible():
    """Batch sizes that do not fill the last workgroup; two runs must agree bitwise."""
    from stove_amd.video_prediction.dynamics import Dynamics
    c, structs, params = oracle_setup(torch.float64)
    dyn = fill_analytic(Dynamics(make_cfg()), 'dyn.').to(DEV)
    g = torch.Generator().manual_seed(3)
    for B in (1, 5, 6, 11, 64):
        s64 = torch.rand(B, 3, 16, generator=g, dtype=torch.float64) * 1.6 - 0.8
        w64 = torch.rand(B, 3, 32, generator=g, dtype=torch.float64)
        so = s64.clone().requires_grad_()
        ro, _ = O.dynamics_forward(c, params, so)
        for p in params.values():
            p.grad = None
        (ro * w64).sum().backward()
        outs = []
        for _ in range(2):
            dyn.zero_grad()
            sd = s64.float().to(DEV).requires_grad_()
            rd, _ = dyn(sd, 0)
            (rd * w64.float().to(DEV)).sum().backward()
            outs.append((rd.detach().clone(), sd.grad.clone(), dyn.out[0][0].weight.grad.clone()))
        assert err(outs[0][0], ro) < 1e-4 and err(outs[0][1], so.grad) < 1e-3
        assert err(outs[0][2], params['dyn.out.0.0.weight'].grad) < 1e-3
        for a, b in zip(*outs):
            assert torch.equal(a, b)


def _gold_idx(a):
    return torch.from_numpy(np.asarray(a)).long().to(DEV)


def test_match_3only():
    """Index work is held bit-exact: the int64 permutation stove_match_objects returns == the reference's own (recovered from its
    matched output by oracle/make_goldens.py source_index), incl. the repair branch (stove.py:273-316) and appearance features."""
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    g = load_golden('g6_match_3only')
    st = Stove(make_cfg())
    z, zs = t_(g['z']).float().to(DEV), t_(g['zstd']).float().to(DEV)
    app = t_(g['app']).float().to(DEV)
    for mode in ('3_only', '3_only_serial'):
        assert torch.equal(ops.match_objects(z[..., 2:4].contiguous(), mode)[0], _gold_idx(g['idx'])), mode
        assert torch.equal(ops.match_objects(torch.cat([z[..., 2:4], 2 * app - 1], -1), mode)[0], _gold_idx(g['idx_app'])), mode
    assert not np.array_equal(g['idx'], np.broadcast_to(np.arange(3), g['idx'].shape))            # the fixture does permute
    zm, zsm, _ = st._3_only_match_objects(z, zs, None)
    assert err(zm, g['z_matched']) < 1e-6 and err(zsm, g['zstd_matched']) < 1e-6
    st.c.debug_match_appearance = True
    zm, zsm, am = st._3_only_match_objects(z, zs, t_(g['app']).float().to(DEV))
    assert err(zm, g['z_matched_app']) < 1e-6 and err(zsm, g['zstd_matched_app']) < 1e-6
    assert err(am, g['app_matched']) < 1e-6
    # the fixture exercises the repair branch: sequence 4 has every object at one place at t=4
    assert not np.array_equal(g['z_matched'], g['z'])


@pytest.mark.parametrize('T', [2, 7, 100, 131])
def test_match_3only_collisions_and_ties(T):
    """The table-composition matcher (csrc/match.hip match3_table_k) against the oracle's frame-by-frame walk on tracks full
    of collisions and exact ties (positions on a coarse grid, objects swapping and sitting on one another), with and
    without appearance features: indices must agree exactly, so the matched tensors are bit-equal."""
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    g = torch.Generator().manual_seed(T)
    B = 48
    z = torch.rand(B, T, 3, 4, generator=g) * 2 - 1
    z[..., 2:] = torch.round(z[..., 2:] * 4) / 4                   # 9 x 9 dyadic grid of positions: collisions and EXACT ties every
                                                                   # few frames (every distance is exact in fp32 whatever the op order)
    z[: B // 2, :, :, 2:] = torch.rand(B // 2, T, 3, 2, generator=g) * 2 - 1
    zs = torch.rand(B, T, 3, 4, generator=g)
    app = torch.round(torch.rand(B, T, 3, 3, generator=g) * 2) / 2
    c, _, _ = oracle_setup(torch.float32)
    for use_app in (False, True):
        c.debug_match_appearance = use_app
        zo, zso, ao = O.match_3only(c, z.clone(), zs.clone(), app.clone() if use_app else None)
        st = Stove(make_cfg(debug_match_appearance=use_app))
        zm, zsm, am = st._3_only_match_objects(z.to(DEV), zs.to(DEV), app.to(DEV) if use_app else None)
        assert err(zm, zo) < 1e-6 and err(zsm, zso) < 1e-6, (T, use_app)
        if use_app:
            assert err(am, ao) < 1e-6
        # ... and as indices, bit-exact (rows of zs are distinct random vectors: the oracle's permutation can be read off its output)
        feat0 = torch.cat([z[..., 2:4]] + ([2 * app - 1] if use_app else []), -1).to(DEV)
        assert torch.equal(ops.match_objects(feat0, '3_only')[0].cpu(), source_index(zs, zso)), (T, use_app)
        # and against the frame-by-frame walk of lane 0 (same arithmetic, so also on the continuous half of the batch, bit for bit)
        feat = torch.cat([z[..., 2:4]] + ([2 * app - 1] if use_app else []), -1).to(DEV)
        assert torch.equal(ops.match_objects(feat, '3_only')[0], ops.match_objects(feat, '3_only_serial')[0])
    c.debug_match_appearance = False


def test_match_greedy():
    from stove_amd.video_prediction.stove import Stove
    g = load_golden('g6_match_greedy')
    st = Stove(make_cfg(num_obj=6, debug_match_objects='greedy'))
    zm, zsm, _ = st._greedy_match_objects(t_(g['z']).float().to(DEV), t_(g['zstd']).float().to(DEV), None)
    assert err(zm, g['z_matched']) < 1e-6 and err(zsm, g['zstd_matched']) < 1e-6
    from stove_amd import ops
    idx = ops.match_objects(t_(g['z']).float().to(DEV)[..., 2:4].contiguous(), 'greedy')[0]
    assert torch.equal(idx, _gold_idx(g['idx']))                       # the reference's permutation, bit-exact
    assert bool((idx.sort(-1).values == torch.arange(6, device=DEV)).all())


def test_fix_supair_stage_on_reference_fixture():
    """g6_fix_supair (crafted glitches on the scale dims, reference stove.py:516-563) straight into the state stage of
    stove_supair_state_fwd (csrc/state.hip supair_state_fwd_k): codes NULL = given states, identity matching."""
    from stove_amd import _lib
    g = load_golden('g6_fix_supair')
    z, zs = t_(g['z']).float(), t_(g['zstd']).float()
    n, T, o = z.shape[:3]
    zc = torch.cat([z, zs], -1).contiguous().to(DEV)
    idx = torch.arange(o, dtype=torch.int64).expand(n, T, o).contiguous().to(DEV)
    skip = 2
    zfix = torch.empty(n, T, o, 8, device=DEV)
    hits = torch.empty(n, T, o, dtype=torch.uint8, device=DEV)
    zl, sl, init6 = torch.empty(n, T - skip, o, 6, device=DEV), torch.empty(n, T - skip, o, 6, device=DEV), torch.empty(n, o, 6, device=DEV)
    lib = _lib.load()
    _lib.check(lib.stove_supair_state_fwd(None, None, zc.data_ptr(), None, idx.data_ptr(), zfix.data_ptr(), hits.data_ptr(), zl.data_ptr(),
                                          sl.data_ptr(), init6.data_ptr(), n, T, o, skip, 1, 0, _lib.stream()), 'stove_supair_state_fwd')
    torch.cuda.synchronize()
    check('fix_supair.z', err(zfix[..., :4], g['z_fixed']), 1e-6)
    check('fix_supair.zstd', err(zfix[..., 4:], g['zstd_fixed']), 1e-6)
    fired = (t_(g['z_fixed']) != t_(g['z'])).any(-1)
    assert torch.equal(hits.bool().cpu(), fired) and int(fired.sum()) >= 2
    # velocities of the smoothed states (stove.py:54-101)
    zf = t_(g['z_fixed']).float()
    check('fix_supair.vel', err(zl[..., 4:], (zf[:, skip:, :, 2:] - zf[:, skip - 1:-1, :, 2:])), 1e-5)


CASES = {
    'n3': dict(num_obj=3),
    'n6': dict(num_obj=6, debug_match_objects='greedy', overlap_beta=100.0, max_obj_scale=0.22),
    'ac3': dict(num_obj=3, action_conditioned=True, action_space=9, debug_core_appearance=True),
    'grav3': dict(num_obj=3),          # BASELINE.json configs[2]: gravity frames through the same path
}


def _golden_noise(gold):
    lat, sd = t_(gold['eps_lat'])[..., 0].float(), t_(gold['eps_std'])[..., 0].float()
    steps = t_(gold['eps_steps']).float().permute(1, 0, 2, 3).contiguous()
    table = {'latent': lat, 'std': sd, 'steps': steps}
    return lambda kind, shape: table[kind].reshape(shape)


REGIME_FUSED_ARENA = [('analytic', True, False), ('analytic', True, True), ('analytic', False, False), ('analytic', False, True),
                      ('init', True, True), ('init', False, False), ('stress', True, True), ('stress', False, False)]


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('regime,fused,arena', REGIME_FUSED_ARENA)
def test_stove_forward_elbo_and_grads(name, regime, fused, arena):
    """`arena`: parameters / gradients as views into the flat ParamArena buffers, tables baked and gradients sunk
    by the arena kernels -- must give the same numbers as the per-tensor autograd path.  `regime`: the weights the model is
    filled with (smooth mid-range / the reference's initial statistics / saturated), each against the reference's own run."""
    full_model_against_golden(load_golden(gname(f'g7_stove_{name}', regime)), name, regime, fused, arena, f'g7_{name}_{regime}', 'stove')


def full_model_against_golden(gold, name, regime, fused, arena, case, key, cfg=None):
    """Stove.forward + backward + rollout on a reference-generated full-model fixture (g7: T <= 8; g17: T = 100).  `case`: the
    fixture's record in g16_reference_fp32_gap.json; `key`: prefix of the recorded parity errors."""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    cfg = CASES[name] if cfg is None else cfg
    # fused=False: host time loop, PyTorch state chain and PyTorch ELBO assembly (the op-by-op restatement)
    st = fill_analytic(Stove(make_cfg(fused_dynamics=fused, fused_state=fused, fused_elbo=fused, **cfg)), '', regime).to(DEV)
    if arena:
        ar = ParamArena(st)
        assert ar.has_spn and ar.has_gnn
    st.noise_fn = _golden_noise(gold)
    x = t_(gold['x']).float().to(DEV)
    actions = t_(gold['actions']).float().to(DEV) if 'actions' in gold else None
    elbo, prop, rewards = st(x, 0, actions)
    gold_at_codes = None
    if regime == 'stress':
        # The saturated model is chaotic: swapping this implementation's float32 codes (1e-6 of the largest code off the reference's)
        # into the float64 REFERENCE moves its z by 8e-5 and its dynamics gradients by up to 1.5e-2 (tools/regime_probe.py, round 5).
        # So the recognition network is held to the reference's codes, and everything behind it to the reference evaluated at the
        # same codes (helpers.reference_at_codes: the oracle, pinned to the reference on this very fixture) with the tight bars;
        # against the fixture itself the forward quantities keep the regime bars below.
        from stove_amd.utils.utils import bw_transform
        c_o, structs_o, params_o = oracle_setup(torch.float64, requires_grad=False, regime=regime, **cfg)
        with torch.no_grad():
            codes = st.sup.encoder(bw_transform(x).flatten(end_dim=1))
            codes_ref = O.encoder_forward(c_o, params_o, O.bw_transform(t_(gold['x'])).flatten(0, 1))
        check('encoder.codes.stress', err(codes, codes_ref), 5e-6)          # achieved 1.6e-6 (fp32 library GEMMs: 1.1e-6)
        gold_at_codes = reference_at_codes(gold, regime, cfg, codes)
    # Bars: the 'analytic' ones (pinned at ~3x what the kernels achieve there) or, in the other regimes, 6x the REFERENCE's own
    # float32-vs-float64 gap on the same fixture (tests/golden/g16_reference_fp32_gap.json) where that is larger: a saturated model
    # amplifies float32 rounding (z of the 'stress' fixtures: 1.2e-5 in the reference's own float32 run).  The ELBO bar stays.
    tag = '' if regime == 'analytic' else '.' + regime
    rel = abs(float(elbo) - float(gold['elbo'])) / abs(float(gold['elbo']))
    check(key + '.elbo_rel' + tag, rel, 1.5e-6)                 # the north-star bar is 1e-4; achieved 2.5e-7
    for k in ('z', 'z_dyn', 'z_sup', 'z_std', 'z_sup_std', 'log_q', 'translik', 'bg', 'patch', 'overlap'):
        check(key + '.prop_' + k + tag, err(prop[k], gold['p_' + k]), regime_bar(8e-6 if k == 'z_sup' else 3e-6, ref_gap(case, 'prop', k)))
    check(key + '.prop_z_dyn_std' + tag, err(prop['z_dyn_std'][2:], gold['p_z_dyn_std'][2:]), 1e-6)
    gold_fixture = gold
    if gold_at_codes is not None:
        gold, tag = gold_at_codes, tag + '.at_codes'          # from here on: the reference at this implementation's codes
        check(key + '.elbo_rel' + tag, abs(float(elbo) - float(gold['elbo'])) / abs(float(gold['elbo'])), 1.5e-6)
        for k in ('z', 'z_dyn', 'z_sup', 'z_std', 'z_sup_std', 'log_q', 'translik'):
            # (log q = -((z - mean) / std)^2 / 2 - log std with z = mean + std eps: for the stress model's stds of 1e-7 the float32
            # difference z - mean is mostly rounding -- in the reference's own float32 run exactly as here: 1.78e-5 / 3.71e-5 / 8.4e-6
            # on n3 / ac3 / grav3 in BOTH -- so log q keeps the regime bar)
            # (z, z_dyn: 1e-5 -- the stress recursion doubles a float32 rounding difference per step, six steps; achieved 2.6e-6 ... 3.3e-6)
            bar = regime_bar(3e-6, ref_gap(case, 'prop', k)) if k == 'log_q' else (8e-6 if k == 'z_sup' else (1e-5 if k in ('z', 'z_dyn') else 3e-6))
            check(key + '.prop_' + k + tag, err(prop[k], gold['p_' + k]), bar)
    loss = -elbo
    if actions is not None:
        check(key + '.rewards' + tag, err(rewards, gold['rewards']), 1e-6)
        loss = loss + 3.0 * (rewards ** 2).sum()
    loss.backward()
    params = dict(st.named_parameters())
    n = 0
    gt = lambda m: ref_gap(case, 'grad_tensor', m)
    # at the reference's own codes (`gold` is the at-codes oracle here in the stress regime) the gradients keep the tight ANALYTIC bars
    # -- chaos was taken out by evaluating at equal codes; achieved 4.4e-5 / 2.9e-5 / 3.2e-4 (g7), 2.7e-5 / 2.4e-5 / 1.4e-3 (g17) --
    # and the regime bars (6 x the reference's float32 gap) only apply against the committed fixture itself
    at_codes = gold_at_codes is not None
    gbar = (lambda bar, gap: bar) if at_codes else regime_bar
    for k, v in gold.items():
        if k.startswith('gn_'):
            p = params[k[3:]]
            assert p.grad is not None, k
            check(key + '.grad_norm' + tag, abs(float(p.grad.norm()) - float(v)) / (float(v) + 1e-9), gbar(1.5e-4, ref_gap(case, 'grad_norm_rel_max')))
            if at_codes:       # ... and, loosely, against the committed fixture: the golden's own gradients stay exercised (the model is
                # chaotic in its codes: 1.6e-6 on them moves the dynamics' gradients by up to 1.5e-2, tools/regime_probe.py)
                v0 = float(gold_fixture[k])
                check(key + '.grad_norm.stress.vs_fixture', abs(float(p.grad.norm()) - v0) / (v0 + 1e-9), 5e-2)
            n += 1
        elif k.startswith('g_'):
            # the reference's own fp32-vs-fp64 gap is 3.3e-4 (max-norm) on the analytic fixtures
            check_grad(key + '.grad_tensor' + tag, params[k[2:]].grad, v, gbar(3e-4, gt('max')), gbar(3.5e-4, gt('l2')), gbar(4e-3, gt('small')))
    assert n > 50
    if arena:                                                  # cores 1-2 are never used: their gradients stay zero
        assert float(params['dyn.self_cores.1.0.weight'].grad.abs().max()) == 0.0
        ar.check()
    # rollout from the last inferred state (G8)
    with torch.no_grad():
        z_last = prop['z'][:, -1]
        fut = actions[:, :5] if actions is not None else None
        app = prop['obj_appearances'][:, -1] if actions is not None else None
        zp, rp = st.rollout(z_last, num=gold['roll_z'].shape[1], actions=fut, appearance=app)
    check(key + '.rollout_z' + tag, err(zp, gold['roll_z']), regime_bar(3e-6, ref_gap(case, 'rollout_z')))
    if actions is not None:
        check(key + '.rollout_rewards', err(rp, gold['roll_rewards']), 3e-6)      # as rollout_z (92 steps at g17: 9.3e-7)
    if 'eps_roll' in gold:
        # sampling rollout (stove.py:833-838) under the reference's draws: the sampled state feeds back
        eps_roll = [t_(e).float().to(DEV) for e in gold['eps_roll']]
        it = iter(eps_roll)
        saved = st.noise_fn
        st.noise_fn = lambda kind, shape: next(it).reshape(shape)
        with torch.no_grad():
            zs, lq, _ = st.rollout(z_last, num=len(eps_roll), sample=True)
        st.noise_fn = saved
        check(key + '.rollout_sample_z' + tag, err(zs, gold['roll_s_z']), regime_bar(2e-6, ref_gap(case, 'rollout_z')))
        check(key + '.rollout_sample_logq' + tag, err(lq, gold['roll_s_logq']), regime_bar(1.5e-5, ref_gap(case, 'prop', 'log_q')))


def test_rollout_std_and_sampling_api():
    from stove_amd.video_prediction.stove import Stove
    st = fill_analytic(Stove(make_cfg())).to(DEV)
    g = torch.Generator().manual_seed(1)
    z_last = (torch.rand(7, 3, 18, generator=g) * 0.8 + 0.1).to(DEV)
    zf, zs, _ = st.rollout(z_last, num=5, return_std=True)
    assert zf.shape == (7, 5, 3, 18) and zs.shape == (7, 5, 3, 16)
    assert torch.equal(zf[..., :2], z_last[:, None, :, :2].expand(-1, 5, -1, -1))      # scales stay fixed
    assert (zs > 0).all() and (zs[..., :2] < 0.3).all() and (zs[..., 2:] < 0.04).all()
    # the fused rollout equals a host loop of single steps
    z = z_last
    for t in range(5):
        out, _ = st.dyn(z[..., 2:], 0)
        m, _ = st.dyn.constrain_z_dyn(out[..., :16], out[..., 16:])
        z = torch.cat([z[..., :2], z[..., 2:4] + m[..., :2], m[..., 2:]], -1)
        assert err(zf[:, t], z) < 1e-5
    zsamp, lq, _ = st.rollout(z_last, num=3, sample=True)
    assert zsamp.shape == (7, 3, 3, 18) and lq.shape == (7, 3, 3, 16)


def test_encoder_lstm_against_oracle():
    """The recognition network (MFMA GEMMs of csrc/gemm_bf16.hip, gate math of csrc/lstm.hip, fused head) against the oracle's restatement of RnnStates."""
    from stove_amd.video_prediction.encoder import RnnStates
    c, structs, params = oracle_setup(torch.float64)
    enc = fill_analytic(RnnStates(make_cfg()), 'sup.encoder.').to(DEV)
    g = torch.Generator().manual_seed(9)
    x64 = torch.rand(37, 1, 32, 32, generator=g, dtype=torch.float64)
    w64 = torch.rand(37, 3, 8, generator=g, dtype=torch.float64)
    out_o = O.encoder_forward(c, params, x64)
    (out_o * w64).sum().backward()
    out_d = enc(x64.float().to(DEV))
    assert out_d.shape == (37, 3, 8)
    check('encoder.codes', err(out_d, out_o), 1.2e-5)
    (out_d * w64.float().to(DEV)).sum().backward()
    for name, p in enc.named_parameters():
        check_grad('encoder.grad', p.grad, params['sup.encoder.' + name].grad, 4e-5, 3e-5, 1.2e-3)


def test_match_volatile():
    from stove_amd.video_prediction.stove import Stove
    g = load_golden('g6_match_volatile')
    st = Stove(make_cfg(debug_match_objects='volatile'))
    zm, zsm, _ = st._volatile_match_objects(t_(g['z']).float().to(DEV), t_(g['zstd']).float().to(DEV), None)
    assert err(zm, g['z_matched']) < 1e-6 and err(zsm, g['zstd_matched']) < 1e-6
    from stove_amd import ops
    idx, _ = ops.match_objects(t_(g['z']).float().to(DEV)[..., 2:4].contiguous(), 'volatile')
    gp = _gold_idx(g['perm'])                  # the reference's 0/1 matrix: one 1 per row (stove.py:405-411), not a permutation at [4, 4]
    assert bool((gp.sum(-1) == 1).all()) and int(gp[4, 4].sum(0).max()) == 3
    assert torch.equal(idx, gp.argmax(-1))     # bit-exact


def test_supair_only_elbo():
    """Stove.forward(..., pretrain=True): the SuPAIR-only ELBO (reference supair.py:504-551)."""
    import torch.distributions.normal as tdn
    from stove_amd.video_prediction.stove import Stove
    g = load_golden('g11_supair_only_f64')
    st = fill_analytic(Stove(make_cfg())).to(DEV)
    eps = t_(g['eps']).float().to(DEV)
    saved = tdn._standard_normal
    tdn._standard_normal = lambda shape, dtype, device: eps.reshape(shape).to(dtype)
    try:
        elbo, prop, _ = st(t_(g['x']).float().to(DEV), 0, None, True)
    finally:
        tdn._standard_normal = saved
    assert abs(float(elbo.detach()) - float(g['elbo'])) < 1e-4 * abs(float(g['elbo']))
    assert err(prop['z'], g['z']) < 1e-4
    (-elbo).backward()
    params = dict(st.named_parameters())
    for k, v in g.items():
        if k.startswith('gn_'):
            assert abs(float(params[k[3:]].grad.norm()) - float(v)) <= 5e-3 * float(v) + 1e-9, k


@pytest.mark.parametrize('arena', [False, True, 'flat_adam'])
def test_three_optimiser_steps_track_the_reference(arena):
    """Adam(amsgrad) + lr schedule + clip_grad_norm_(1) on one batch (reference train.py:431-473, fp32):
    the ELBO sequence and parameter checksums after three steps."""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    g = load_golden('g9_optimiser_steps')
    cfg = make_cfg()
    st = fill_analytic(Stove(cfg)).to(DEV)
    ar = ParamArena(st) if arena else None
    if arena == 'flat_adam':       # the one-launch Adam + clip over the flat buffers
        from stove_amd.optim import FlatAdam
        opt = FlatAdam(ar, lr=cfg.learning_rate, amsgrad=cfg.debug_amsgrad)
    else:
        opt = torch.optim.Adam(st.parameters(), lr=cfg.learning_rate, amsgrad=cfg.debug_amsgrad)
    x = t_(g['x']).float().to(DEV)
    for step in range(1, 4):
        lat = t_(g['eps_lat'])[step - 1][..., 0].float()
        sd = t_(g['eps_std'])[step - 1][..., 0].float()
        steps = t_(g['eps_steps'])[step - 1].float().permute(1, 0, 2, 3).contiguous()
        table = {'latent': lat, 'std': sd, 'steps': steps}
        st.noise_fn = lambda kind, shape, _t=table: _t[kind].reshape(shape)
        for grp in opt.param_groups:
            grp['lr'] = max(cfg.learning_rate * np.exp(-step / cfg.debug_anneal_lr), cfg.min_learning_rate)
        if arena:
            ar.zero_grad()
        else:
            opt.zero_grad()
        elbo, _, _ = st(x, step, None)
        (-elbo).backward()
        if arena == 'flat_adam':
            opt.step(max_norm=1)
        elif arena:
            ar.clip_grad_norm_(1)
            opt.step()
        else:
            torch.nn.utils.clip_grad_norm_(st.parameters(), 1)
            opt.step()
        ref = float(g['elbos'][step - 1])
        assert abs(float(elbo.detach()) - ref) < 2e-4 * abs(ref), (step, float(elbo.detach()), ref)
    params = dict(st.named_parameters())
    for k, v in g.items():
        if k.startswith('p_'):
            got = float(params[k[2:]].detach().double().sum())
            assert abs(got - float(v)) < 2e-4 * abs(float(v)) + 1e-4, (k, got, float(v))
    if arena == 'flat_adam':       # checkpoint layout of torch.optim.Adam: state per parameter index, reloadable
        sd = opt.state_dict()
        assert set(sd['state'][0]) >= {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'} and float(sd['state'][0]['step']) == 3
        ref = torch.optim.Adam(st.parameters(), lr=cfg.learning_rate, amsgrad=cfg.debug_amsgrad)
        ref.load_state_dict(sd)
        m0 = opt.state[ar.params[5]]['exp_avg'].clone()
        opt2 = FlatAdam(ar, lr=cfg.learning_rate, amsgrad=cfg.debug_amsgrad)
        opt2.load_state_dict(sd)
        assert opt2._steps == 3 and torch.equal(opt2.state[ar.params[5]]['exp_avg'], m0)


@pytest.mark.parametrize('mode', ['3_only', 'greedy', 'volatile'])
def test_state_pipeline_against_torch_chain(mode):
    """Fused state pipeline (csrc/state.hip) == constrain_zp -> match -> gather -> fix_supair -> velocities done op by
    op in PyTorch, values and gradients; random codes make the smoothing stencil fire and 'volatile' pick duplicates."""
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    st = Stove(make_cfg(debug_match_objects=mode)).to(DEV)
    n, T, o, skip = 6, 11, 3, 2
    g = torch.Generator(device='cpu').manual_seed(3)
    codes = (2.0 * torch.randn(n * T * o, 8, generator=g)).to(DEV).requires_grad_()
    ws = [torch.randn(*s, generator=g).to(DEV) for s in ((n, T, o, 8), (n, T - skip, o, 6), (n, T - skip, o, 6), (n, o, 6))]
    zfix, zl, sl, init6, idx = ops.supair_state(codes, st.sup.zp_span_low(), n, T, o, skip, True, mode)
    ((zfix * ws[0]).sum() + (zl * ws[1]).sum() + (sl * ws[2]).sum() + (init6 * ws[3]).sum()).backward()
    ref = codes.detach().clone().requires_grad_()
    z, zs = st.sup.constrain_zp(ref)
    z, zs, _ = st.match_objects(z.view(n, T, o, 4), zs.view(n, T, o, 4), None)
    raw = torch.cat([z, zs], -1).detach()
    z, zs = st.fix_supair(z, zs)
    full, sfull = st.v_from_state(z), st.v_std_from_pos(zs)
    fixed = torch.cat([z, zs], -1)
    assert float((fixed.detach() - raw).abs().max()) > 0.01            # the stencil did replace something
    if mode == 'volatile':
        assert any(len(set(r)) < o for r in idx.view(-1, o).tolist())   # ... and volatile is not a permutation here
    ((fixed * ws[0]).sum() + (full[:, skip:] * ws[1]).sum() + (sfull[:, skip:] * ws[2]).sum()
     + (full[:, skip - 1] * ws[3]).sum()).backward()
    assert err(zfix, fixed) < 1e-6 and err(zl, full[:, skip:]) < 1e-6 and err(sl, sfull[:, skip:]) < 1e-6
    assert err(init6, full[:, skip - 1]) < 1e-6
    assert err(codes.grad, ref.grad) < 1e-5
    # with the latent prior draws handed over, the fourth output is the recursion's whole initial state (row stride 18) and
    # its gradient is read back at that stride
    noise = torch.randn(n, o, 12, generator=g).to(DEV)
    w18 = torch.randn(n, o, 18, generator=g).to(DEV)
    w18[..., :6] = ws[3]
    c2 = codes.detach().clone().requires_grad_()
    zfix2, zl2, sl2, init18, idx2 = ops.supair_state(c2, st.sup.zp_span_low(), n, T, o, skip, True, mode, lat_noise=noise)
    ((zfix2 * ws[0]).sum() + (zl2 * ws[1]).sum() + (sl2 * ws[2]).sum() + (init18 * w18).sum()).backward()
    assert init18.shape == (n, o, 18) and torch.equal(init18[..., :6], init6) and torch.equal(init18[..., 6:], 0.01 * noise)
    assert torch.equal(zfix2, zfix) and torch.equal(zl2, zl) and torch.equal(idx2, idx)
    assert torch.equal(c2.grad, codes.grad)


def test_elbo_assembly_against_torch():
    from stove_amd import ops
    n, T, o, skip = 4, 7, 3, 2
    g = torch.Generator(device='cpu').manual_seed(5)
    Ts = T - skip
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    zs, mean, zd = mk(n, Ts, o, 18).requires_grad_(), mk(n, Ts, o, 18).requires_grad_(), mk(n, Ts, o, 16).requires_grad_()
    std = (0.05 + torch.rand(n, Ts, o, 18, generator=g)).to(DEV).requires_grad_()
    lik = mk(n, T - 1).requires_grad_()
    tstd = [0.01] * 4 + [0.02] * 12
    elbo, stats = ops.elbo(zs, mean, std, zd, lik, tstd, n, T, o, skip)
    (3.0 * elbo).backward()
    got = [t.grad.clone() for t in (zs, mean, std, zd, lik)]
    for t in (zs, mean, std, zd, lik):
        t.grad = None
    lp = lambda x, m, s: -0.5 * ((x - m) / s) ** 2 - torch.log(s) - 0.5 * float(np.log(2 * np.pi))
    logq = lp(zs, mean, std).sum((-2, -1)).flatten()
    trans = lp(zs[..., 2:], zd, torch.tensor(tstd, device=DEV)).sum((-2, -1)).flatten()
    ref = torch.mean(trans + lik[:, skip - 1:].reshape(-1) - logq) + torch.mean(lik[:, :skip - 1])
    (3.0 * ref).backward()
    assert abs(float(elbo) - float(ref)) < 1e-5 * abs(float(ref))
    assert abs(float(stats[0]) - float(trans.mean())) < 1e-5 * abs(float(trans.mean()))
    assert abs(float(stats[1]) - float(logq.mean())) < 1e-5 * abs(float(logq.mean()))
    for a, t in zip(got, (zs, mean, std, zd, lik)):
        assert err(a, t.grad) < 1e-5


@pytest.mark.parametrize('nonlinear', ['relu', 'leaky_relu'])      # the second one selects F.elu (the reference's quirk, dynamics.py:107-110)
@pytest.mark.parametrize('n_obj,ac', [(2, False), (3, False), (4, False), (5, False), (6, False), (5, True), (6, True),
                                      (7, False), (8, False), (7, True), (8, True)])
def test_small_graph_recursion_matches_step_kernels(n_obj, ac, nonlinear):
    """The persistent time loops against the host loop over the single-step MFMA kernel + PyTorch autograd: ELBO, every gradient,
    and the rollout.  N <= 6: the small-graph kernels (csrc/gnn_small*.hip; five and six objects run two node rows per wave and two
    tiles of edge columns).  N = 7, 8: the workgroup-wide MFMA loops of csrc/gnn.hip (dyn_loop_fwd_k / dyn_loop_bwd_k /
    rollout_fwd_k), which no BASELINE configuration reaches since six objects moved to the small-graph path.  `ac`:
    action-conditioned, 23 inputs per node and the reward head.  This is a comparison of one kernel of ours with another, through the
    whole model; the counts without goldens (2, 4, 5, 7, 8, and one object) are held to the float64 oracle, step, recursion and
    rollout each on its own, by tests/test_gpu_dynamics_counts.py -- what stays particular to this test is the agreement of the two
    paths Stove.forward can take."""
    recursion_against_step_kernels(n_obj, ac, nonlinear)


def recursion_inputs(ac):
    """-> frames x (3, 6, 3, 32, 32), one-hot actions or None, the configuration entries of `ac`, a repeatable noise_fn"""
    n, T = 3, 6
    g = torch.Generator(device='cpu').manual_seed(11)
    x = (torch.rand(n, T, 3, 32, 32, generator=g) < 0.04).float().to(DEV)
    extra = dict(action_conditioned=True, action_space=9, debug_core_appearance=True) if ac else {}
    actions = torch.nn.functional.one_hot(torch.randint(0, 9, (n, T), generator=g), 9).float().to(DEV) if ac else None
    noise = {}

    def noise_fn(kind, shape):
        key = (kind, tuple(shape))
        if key not in noise:
            noise[key] = torch.randn(*shape, generator=g)
        return noise[key]
    return x, actions, extra, noise_fn


def recursion_against_step_kernels(n_obj, ac, nonlinear):
    from stove_amd.video_prediction.stove import Stove
    x, actions, extra, noise_fn = recursion_inputs(ac)
    res = []
    for fused in (True, False):
        st = fill_analytic(Stove(make_cfg(num_obj=n_obj, fused_dynamics=fused, debug_match_objects='greedy', debug_nonlinear=nonlinear, **extra))).to(DEV)
        st.noise_fn = noise_fn
        elbo, prop, rewards = st(x, 0, actions)
        loss = -elbo
        if ac:
            loss = loss + 3.0 * (rewards ** 2).sum()
        loss.backward()
        with torch.no_grad():
            zp, _ = st.rollout(prop['z'][:, -1], num=7, actions=actions[:, :4] if ac else None,
                               appearance=prop['obj_appearances'][:, -1] if ac else None)
        res.append((float(elbo.detach()), {k: p.grad.clone() for k, p in st.named_parameters() if p.grad is not None}, zp))
    (e1, g1, z1), (e2, g2, z2) = res
    assert abs(e1 - e2) < 1e-5 * abs(e2), (e1, e2)
    assert set(g1) == set(g2)
    for k in g1:
        assert err(g1[k], g2[k]) < 2e-3 or float(g2[k].abs().max()) < 1e-9, k
    assert err(z1, z2) < 1e-4


@pytest.mark.parametrize('nonlinear', ['relu', 'leaky_relu'])
@pytest.mark.parametrize('n_obj', [2, 3, 4, 5, 6, 7])
def test_recursion_without_saved_activations_and_general_backward(n_obj, nonlinear, monkeypatch):
    """What test_small_graph_recursion_matches_step_kernels leaves to chance in the choice of the recursion's instantiations, on
    its inputs.  The forward that saves nothing (torch.no_grad) returns bit for bit what the one that keeps the activations for
    the backward returns.  At three and six objects, the backward of the action-conditioned model (23 inputs per node, a gradient
    for `pred`: not the instantiations for the plain training step, which three objects otherwise always run) holds the bars of
    that test against the step kernels."""
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    x, actions, extra, noise_fn = recursion_inputs(False)
    st = fill_analytic(Stove(make_cfg(num_obj=n_obj, fused_dynamics=True, debug_match_objects='greedy', debug_nonlinear=nonlinear, **extra))).to(DEV)
    st.noise_fn = noise_fn
    calls, dyn_loop = [], ops.dyn_loop
    monkeypatch.setattr(ops, 'dyn_loop', lambda *a, **kw: calls.append((a, kw)) or dyn_loop(*a, **kw))
    st(x, 0, actions)
    monkeypatch.undo()
    (a, kw), = calls
    assert a[0].requires_grad and a[0].shape[-1] == 18 and a[1].shape[0] == 3 and a[1].shape[2] == n_obj
    saving = dyn_loop(*a, **kw)
    with torch.no_grad():
        plain = dyn_loop(*a, **kw)
    assert saving[0].grad_fn is not None and plain[0].grad_fn is None
    for name, u, v in zip(('z', 'zdyn', 'zdstd', 'mean', 'std'), saving, plain):
        assert torch.equal(u, v), name
    if n_obj in (3, 6):
        recursion_against_step_kernels(n_obj, True, nonlinear)


def test_object_embedding_kernel_against_grid_sample():
    """stove_glimpse_mean == mean over patches_from_z (PyTorch affine_grid / grid_sample) of the colour frame."""
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    st = Stove(make_cfg()).to(DEV)
    g = torch.Generator(device='cpu').manual_seed(4)
    nf, o = 37, 3
    x = torch.rand(nf, 3, 32, 32, generator=g).to(DEV)
    z = torch.cat([0.1 + 0.5 * torch.rand(nf * o, 2, generator=g), 1.6 * torch.rand(nf * o, 2, generator=g) - 0.8], 1).to(DEV)
    want = st.sup.patches_from_z(x, z).mean((-1, -2))
    got = ops.glimpse_mean(x, z, o)
    assert err(got, want) < 1e-5


@pytest.mark.parametrize('gemm', ['bf16x3', 'fp32'])
@pytest.mark.parametrize('rows,H1,OUT', [(111, 50, 8), (1, 50, 8), (64, 50, 8), (65, 64, 8), (3 * 25600, 50, 8), (200, 7, 3), (0, 50, 8),
                                         (16 * 513 + 5, 49, 8), (40, 17, 8)])
def test_encoder_head_kernels(rows, H1, OUT, gemm):
    """fc2(sigmoid(fc1(h))) (reference encoder.py:53-56) vs the op-by-op chain in float64: the one-kernel head of
    csrc/head_fused.hip (default; OUT = 8) and the library-GEMM + head_*_k pair (gemm='fp32', and any other OUT)."""
    from stove_amd import ops
    g = torch.Generator().manual_seed(rows + H1)
    h = torch.randn(rows, 256, generator=g, dtype=torch.float64)
    w1 = torch.randn(H1, 256, generator=g, dtype=torch.float64) * 0.1
    b1 = torch.randn(H1, generator=g, dtype=torch.float64)
    w2 = torch.randn(OUT, H1, generator=g, dtype=torch.float64) * 0.3
    b2 = torch.randn(OUT, generator=g, dtype=torch.float64)
    wout = torch.randn(rows, OUT, generator=g, dtype=torch.float64)
    ref_in = [t.clone().requires_grad_() for t in (h, w1, b1, w2, b2)]
    ref = torch.nn.functional.linear(torch.sigmoid(torch.nn.functional.linear(ref_in[0], ref_in[1], ref_in[2])), ref_in[3], ref_in[4])
    (ref * wout).sum().backward()
    dev_in = [t.float().to(DEV).requires_grad_() for t in (h, w1, b1, w2, b2)]
    out = ops.encoder_head(*dev_in, gemm=gemm)
    assert out.shape == (rows, OUT)
    if rows == 0:
        return
    assert err(out, ref) < 1e-5
    (out * wout.float().to(DEV)).sum().backward()
    for a, b, name in zip(dev_in, ref_in, ('h', 'w1', 'b1', 'w2', 'b2')):
        assert err(a.grad, b.grad) < (2e-4 if rows > 10000 else 2e-5), name
    # fixed summation order: bitwise reproducible
    again = [t.detach().clone().requires_grad_() for t in dev_in]
    (ops.encoder_head(*again, gemm=gemm) * wout.float().to(DEV)).sum().backward()
    for a, b in zip(dev_in, again):
        assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize('gemm', ['bf16x3', 'fp32'])
def test_encoder_head_step_major(gemm):
    """step_major: (steps, n, 256) in, (n, steps, 8) out, equal to the plain head followed by a transpose -- values and gradients."""
    from stove_amd import ops
    g = torch.Generator().manual_seed(1)
    K, n = 3, 37
    h = torch.randn(K, n, 256, generator=g).to(DEV)
    ps = [torch.randn(50, 256, generator=g) * 0.1, torch.randn(50, generator=g), torch.randn(8, 50, generator=g) * 0.3, torch.randn(8, generator=g)]
    wout = torch.randn(n, K, 8, generator=g).to(DEV)
    res = []
    for sm in (False, True):
        ins = [h.clone().requires_grad_()] + [p.to(DEV).requires_grad_() for p in ps]
        out = ops.encoder_head(*ins, gemm=gemm, step_major=sm)
        if not sm:
            out = out.transpose(0, 1)
        assert out.shape == (n, K, 8)
        (out * wout).sum().backward()
        res.append([out.detach()] + [t.grad for t in ins])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize('mode,bar', [('fp32', 1e-6), ('bf16x3', 1e-6), ('bf16', 2e-5)])
def test_encoder_gemm_variants_elbo_delta(mode, bar):
    """config.encoder_gemm: the recognition network's products on library fp32 GEMMs, on the split-bf16 MFMA kernel (default)
    and on plain bf16 operands (BASELINE.json configs[1] "bf16": reported, never the default).  ELBO against the reference's
    golden; the achieved deltas land in gpurun_out/parity_errors.json."""
    from stove_amd.video_prediction.stove import Stove
    gold = load_golden('g7_stove_n3_f64')
    st = fill_analytic(Stove(make_cfg(encoder_gemm=mode))).to(DEV)
    st.noise_fn = _golden_noise(gold)
    elbo, prop, _ = st(t_(gold['x']).float().to(DEV), 0, None)
    check('stove.elbo_rel_encoder_' + mode, abs(float(elbo) - float(gold['elbo'])) / abs(float(gold['elbo'])), bar)
    check('stove.z_sup_encoder_' + mode, err(prop['z_sup'], gold['p_z_sup']), 5e-4 if mode == 'bf16' else 3e-6)


@pytest.mark.parametrize('n_obj', [3, 6])
def test_recursion_forward_chains_domain_large_activations_small_weights(n_obj):
    """The forward edge chains of the small-graph recursion kernels (csrc/gnn_small.hip sm_split_layer_tiles: relation / attention
    layers 2 and 3 as three v_mfma_f32_16x16x32_f16 on IEEE-half hi / lo pieces) at the edge of their stated domain (stove_hip.h,
    stove_dynloop_fwd / stove_rollout_fwd): first-layer weights x 300 drive the chains' input activations to O(10^3), second-layer
    weights x 1/300 put every lo piece of a weight into half's subnormals.  Inside the domain (|activation| < 65 504) the 12-step
    rollout stays within 2e-5 of the float64 oracle (2e-6 at ordinary magnitudes: the subnormal lo pieces keep 2^-25 absolute, not
    2^-22 relative); beyond it the documented failure is inf / NaN, not a silently wrong number."""
    from stove_amd.video_prediction.stove import Stove
    kw = dict(num_obj=n_obj, debug_match_objects='3_only' if n_obj == 3 else 'greedy')
    c, structs, params = oracle_setup(torch.float64, requires_grad=False, **kw)
    st = fill_analytic(Stove(make_cfg(**kw)))
    scale = {'dyn.rel_cores.0.0.weight': 300.0, 'dyn.rel_cores.0.0.bias': 300.0, 'dyn.att_net.0.0.weight': 300.0, 'dyn.att_net.0.0.bias': 300.0,
             'dyn.rel_cores.0.1.weight': 1.0 / 300.0, 'dyn.att_net.0.1.weight': 1.0 / 300.0}
    named = dict(st.named_parameters())
    with torch.no_grad():
        for k, f in scale.items():
            named[k].mul_(f)
            params[k] = params[k] * f
    st = st.to(DEV)
    g = torch.Generator().manual_seed(n_obj)
    z_last = torch.cat([torch.rand(5, n_obj, 2, generator=g) * 0.3 + 0.2, torch.rand(5, n_obj, 16, generator=g) * 1.6 - 0.8], -1)
    with torch.no_grad():
        zo, _ = O.rollout(c, params, z_last.double(), 12)
        # the chains' inputs really are large: first relation layer of the oracle on the first state
        s0 = z_last[..., 2:].double()
        zp, _ = st.rollout(z_last.to(DEV), num=12)
    assert torch.isfinite(zp).all()
    check('dyn_loop.domain_edge.rollout_z', err(zp, zo), 2e-5)
    # beyond the domain: activations past half's range overflow to inf in the pieces; the kernel must not return finite garbage
    with torch.no_grad():
        for k in ('dyn.rel_cores.0.0.weight', 'dyn.rel_cores.0.0.bias'):
            named[k].mul_(1e4)
        zbad, _ = st.rollout(z_last.to(DEV), num=2)
    assert not torch.isfinite(zbad).all()


ABLATIONS = {'novel': dict(num_obj=3, debug_no_velocity=True), 'nolat': dict(num_obj=3, debug_no_latents=True),
             'noreuse': dict(num_obj=3, debug_no_reuse=True)}


@pytest.mark.parametrize('name', list(ABLATIONS))
@pytest.mark.parametrize('arena', [False, True])
def test_stove_forward_full_state_ablations(name, arena):
    """config.debug_no_velocity / debug_no_latents / debug_no_reuse (reference stove.py:140-160) against the reference's own runs (g19):
    ELBO, every prop_dict entry, gradients, rollout.  The first two run q(z) on the op-by-op chain (the GNN step kernel in a host time
    loop), the third is the default model (the reference overwrites what the flag sets) and stays on the fused recursion."""
    gold = load_golden(f'g19_stove_{name}_f64')
    full_model_against_golden(gold, name, 'analytic', True, arena, f'g19_{name}_analytic', 'stove_ablation', ABLATIONS[name])
