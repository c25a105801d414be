"""GPU tests of the one-launch sampling rollout (stove_rollout_sample_fwd / _cl; Stove.rollout(sample=True) with autograd off):
the reference's fixtures, the float64 oracle on shapes no fixture holds, the host loop of single steps, the untouched mean path,
the library's own noise, and the C ABI's argument checks."""
import ctypes
import functools
import math

import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, err, fill_analytic, ref_gap, regime_bar
from helpers import load_golden, oracle_setup, t_
from test_gpu_dynamics import CASES, _golden_noise, gname, make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INVALID = 1          # hipErrorInvalidValue
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def width_cfg(cl):
    return {} if cl == 32 else dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize('regime', ['analytic', 'init', 'stress'])
@pytest.mark.parametrize('name', ['n3', 'grav3'])
def test_fused_sampling_rollout_against_reference_fixture(name, regime):
    """Ten sampled steps under the reference's own draws (eps_roll) against its roll_s_z / roll_s_logq, through the fused path
    (torch.no_grad).  z_last as tests/test_gpu_dynamics.py::full_model_against_golden obtains it: the last state Stove.forward infers
    on the fixture's frames -- and, as there, the saturated 'stress' model (chaotic in its codes) is held to the reference evaluated at
    this implementation's codes.  Bars: that test's, regime_bar(2e-6, .) for z and regime_bar(1.5e-5, .) for log q."""
    from stove_amd.video_prediction.stove import Stove
    gold = load_golden(gname(f'g7_stove_{name}', regime))
    case = f'g7_{name}_{regime}'
    cfg = CASES[name]
    st = fill_analytic(Stove(make_cfg(**cfg)), '', regime).to(DEV)
    st.noise_fn = _golden_noise(gold)
    x = t_(gold['x']).float().to(DEV)
    with torch.no_grad():
        _, prop, _ = st(x, 0, None)
        z_last = prop['z'][:, -1]
    want_z, want_lq = gold['roll_s_z'], gold['roll_s_logq']
    tag = '' if regime == 'analytic' else '.' + regime
    if regime == 'stress':
        from stove_amd.utils.utils import bw_transform
        c, structs, params = oracle_setup(torch.float64, requires_grad=False, regime=regime, **cfg)
        with torch.no_grad():
            codes = st.sup.encoder(bw_transform(x).flatten(end_dim=1))
            eps = {'latent': t_(gold['eps_lat']), 'std': t_(gold['eps_std']), 'steps': [t_(e) for e in gold['eps_steps']]}
            _, _, info = O.stove_forward(c, params, structs, t_(gold['x']), eps, None, detail=True, code_values=codes.double().cpu())
            zs_o, lq_o, _ = O.rollout(c, params, info['z'][:, -1], want_z.shape[1], eps=[t_(e) for e in gold['eps_roll']])
        want_z, want_lq, tag = zs_o, lq_o, tag + '.at_codes'
    eps_roll = [t_(e).float().to(DEV) for e in gold['eps_roll']]
    assert len(eps_roll) == 10
    calls = []

    def noise(kind, shape):
        calls.append((kind, tuple(shape)))
        return eps_roll[len(calls) - 1].reshape(shape)
    st.noise_fn = noise
    with torch.no_grad():
        zs, lq, rew = st.rollout(z_last, num=10, sample=True)
    assert calls == [('rollout', (z_last.shape[0], 3, 16))] * 10               # one call per step, in order
    assert zs.shape == (z_last.shape[0], 10, 3, 18) and lq.shape == (z_last.shape[0], 10, 3, 16) and rew.shape == (10,)
    check('rollout_sample.fixture_z' + tag, err(zs, want_z), regime_bar(2e-6, ref_gap(case, 'rollout_z')))
    check('rollout_sample.fixture_logq' + tag, err(lq, want_lq), regime_bar(1.5e-5, ref_gap(case, 'prop', 'log_q')))


# ------------------------------------------------------------------------------------------------ 2. the float64 oracle on the box
@functools.lru_cache(maxsize=None)
def _oracle(cl, n_obj, dtype):
    c, _, params = oracle_setup(dtype, requires_grad=False, num_obj=n_obj, **width_cfg(cl))
    return c, params


def _oracle_sample(cl, n_obj, z_last, eps, dtype):
    """O.rollout's sampling branch on float32 inputs lifted to `dtype` -> z, log q, and the stds the draws were scaled by"""
    c, params = _oracle(cl, n_obj, dtype)
    D = cl // 2
    with torch.no_grad():
        z0 = z_last.to(dtype)
        z, lq, _ = O.rollout(c, params, z0, eps.shape[1], eps=[e.to(dtype) for e in eps.unbind(1)])
        prev = torch.cat([z0[:, None], z[:, :-1]], 1).flatten(0, 1)
        out, _ = O.dynamics_forward(c, params, prev[..., 2:])
        _, sd = O.constrain_z_dyn(c, out[..., :D], out[..., D:])
    return z, lq, sd.view(z.shape[0], z.shape[1], n_obj, D)


def _inputs(cl, n_obj, B, num, seed):
    D = cl // 2
    g = torch.Generator().manual_seed(seed)
    z_last = torch.cat([torch.rand(B, n_obj, 2, generator=g) * 0.2 + 0.1, torch.rand(B, n_obj, D, generator=g) * 1.2 - 0.6], -1)
    eps = torch.randn(B, num, n_obj, D, generator=g)
    return z_last, eps


def _dynamics(cl, n_obj, **kw):
    from stove_amd.video_prediction.dynamics import Dynamics
    return fill_analytic(Dynamics(make_cfg(num_obj=n_obj, **kw, **width_cfg(cl))), 'dyn.').to(DEV)


def _image(dyn, cl):
    from stove_amd import ops
    return ops.gnn_width(cl).image(*[t.detach().float().contiguous() for t in dyn.param_image(0)])


def _call_sample(cl, dyn, params, z_last, eps, extra=None, A=1, sin_dim=None, zstd=True, pred=False):
    """stove_rollout_sample_fwd[_cl] through the ctypes binding, nothing of ops in between -> z_pred, log_q, zstd, pred"""
    from stove_amd import _lib
    lib = _lib.load()
    B, num, N, D = eps.shape
    z_pred = torch.full((B, num, N, D + 2), float('nan'), device=DEV)
    log_q = torch.full((B, num, N, D), float('nan'), device=DEV)
    sd = torch.full((B, num, N, D), float('nan'), device=DEV) if zstd else None
    pr = torch.full((B, num, N, cl), float('nan'), device=DEV) if pred else None
    p = _lib.ptr
    ptrs = (p(z_last), p(extra), p(params), p(eps), p(z_pred), p(log_q), p(sd), p(pr))
    tail = (B, num, A, N, D if sin_dim is None else sin_dim, 2, int(dyn.use_elu), *[float(k) for k in dyn.loop_consts()], _lib.stream())
    rc = lib.stove_rollout_sample_fwd(*ptrs, *tail) if cl == 32 else lib.stove_rollout_sample_fwd_cl(*ptrs, cl, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return z_pred, log_q, sd, pr


# (cl, N): every kernel and instantiation a sampling call can reach -- cl = 32: wave per node row (N = 2), its three-object
# specialisation, half-wave per row (5, 6), the block-wise MFMA kernel (7); cl = 16 / 64: the width-generic kernel at 3 and 6
SHAPES = [(32, 2), (32, 3), (32, 5), (32, 6), (32, 7), (16, 3), (16, 6), (64, 3), (64, 6)]


@pytest.mark.parametrize('num', [1, 7])
@pytest.mark.parametrize('cl,n_obj', SHAPES)
def test_sampling_rollout_against_the_oracle_on_the_box(cl, n_obj, num):
    """B = 5 (no multiple of a workgroup's group of sequences), analytic weights, eps from a seeded CPU generator, the C ABI called
    directly.  Bars: z and the stds 3e-6, what the mean rollout's rollout_z holds at every width (tests/test_gpu_dynamics.py,
    tests/test_gpu_cl.py); log q 1.5e-5.  Each is regime_bar'ed with the ORACLE's own float32-vs-float64 gap on the same inputs,
    measured here on the CPU (6 x that gap where it is larger, gpu_helpers.regime_bar's rule) and printed next to what the kernel
    achieves.  Measured gaps at num = 7: z 1.6e-7 ... 1.2e-6, stds 8e-7 ... 3.3e-6, log q 2e-7 ... 4.1e-6, the largest of each at
    cl = 16 with six objects -- the one shape whose 6 x gap exceeds the plain bars (z 7.2e-6, stds 2.0e-5, log q 2.4e-5); the stds'
    own float32 gap is above the 3e-6 bar there, so no float32 implementation is held to it."""
    B = 5
    z_last, eps = _inputs(cl, n_obj, B, num, seed=100 * cl + 10 * n_obj + num)
    z_o, lq_o, sd_o = _oracle_sample(cl, n_obj, z_last, eps, torch.float64)
    z_f, lq_f, sd_f = _oracle_sample(cl, n_obj, z_last, eps, torch.float32)
    gaps = err(z_f, z_o), err(sd_f, sd_o), err(lq_f, lq_o)
    dyn = _dynamics(cl, n_obj)
    z, lq, sd, _ = _call_sample(cl, dyn, _image(dyn, cl), z_last.to(DEV), eps.to(DEV))
    key = f'rollout_sample.oracle.cl{cl}'
    print(f'{key} N={n_obj} num={num}: z {err(z, z_o):.3g} (oracle f32 gap {gaps[0]:.3g})  zstd {err(sd, sd_o):.3g} ({gaps[1]:.3g})  '
          f'log_q {err(lq, lq_o):.3g} ({gaps[2]:.3g})')
    assert torch.equal(z[..., :2], z_last[:, None, :, :2].expand(-1, num, -1, -1).to(DEV))         # scales stay fixed
    check(key + '.z', err(z, z_o), regime_bar(3e-6, gaps[0]))
    check(key + '.zstd', err(sd, sd_o), regime_bar(3e-6, gaps[1]))
    check(key + '.log_q', err(lq, lq_o), regime_bar(1.5e-5, gaps[2]))


def test_action_conditioned_sampling_rollout_with_appearance_against_the_oracle():
    """Stove.rollout(sample=True) under no_grad on the action-conditioned model with appearance: 23 inputs per node, A = 3 actions
    cycled (t % A) over num = 7 steps, rewards from the kernel's `pred`.  Bars: z 3e-6, log q 1.5e-5, rewards 3e-6."""
    from stove_amd.video_prediction.stove import Stove
    cfg = CASES['ac3']
    B, N, A, num = 5, 3, 3, 7
    z_last, eps = _inputs(32, N, B, num, seed=23)
    g = torch.Generator().manual_seed(24)
    actions = torch.nn.functional.one_hot(torch.randint(0, 9, (B, A), generator=g), 9).float()
    app = torch.rand(B, N, 3, generator=g)
    c, _, params = oracle_setup(torch.float64, requires_grad=False, **cfg)
    with torch.no_grad():
        z_o, lq_o, rew_o = O.rollout(c, params, z_last.double(), num, actions.double(), app.double(), eps=[e.double() for e in eps.unbind(1)])
    st = fill_analytic(Stove(make_cfg(**cfg))).to(DEV)
    it = iter(eps.to(DEV).unbind(1))
    st.noise_fn = lambda kind, shape: next(it).reshape(shape)
    with torch.no_grad():
        out = st.rollout(z_last.to(DEV), num=num, sample=True, return_std=True, actions=actions.to(DEV), appearance=app.to(DEV))
    assert len(out) == 3                                    # the reference's 3-tuple also with return_std (stove.py:855-856)
    z, lq, rew = out
    assert rew.shape == rew_o.shape and rew.shape[:2] == (B, num)
    check('rollout_sample.oracle.ac3.z', err(z, z_o), 3e-6)
    check('rollout_sample.oracle.ac3.log_q', err(lq, lq_o), 1.5e-5)
    check('rollout_sample.oracle.ac3.rewards', err(rew, rew_o), 3e-6)


# ------------------------------------------------------------------------------------------------ 3. fused against the step loop
@pytest.mark.parametrize('n_obj', [3, 6])
def test_fused_sampling_rollout_equals_the_step_loop(n_obj):
    """Same draws, same model: the one-launch rollout against single steps of Dynamics.forward + constrain_z_dyn written out here,
    and against Stove.rollout's own loop (autograd on), which stays differentiable.  z within 1e-5, the bar
    test_rollout_std_and_sampling_api applies to fused-vs-loop on the mean branch."""
    from stove_amd.video_prediction.stove import Stove
    kw = dict(debug_match_objects='greedy') if n_obj != 3 else {}
    st = fill_analytic(Stove(make_cfg(num_obj=n_obj, **kw))).to(DEV)
    num = 5
    z_last, eps = _inputs(32, n_obj, 7, num, seed=n_obj)
    z_last, eps = z_last.to(DEV), eps.to(DEV)

    def feed():
        it = iter(eps.unbind(1))
        return lambda kind, shape: next(it).reshape(shape)
    st.noise_fn = feed()
    with torch.no_grad():
        zf, lqf, _ = st.rollout(z_last, num=num, sample=True)
        z = z_last
        for t in range(num):
            out, _ = st.dyn(z[..., 2:], 0)
            m, sd = st.dyn.constrain_z_dyn(out[..., :16], out[..., 16:])
            mean = torch.cat([z[..., 2:4] + m[..., :2], m[..., 2:]], -1)
            z = torch.cat([z[..., :2], mean + sd * eps[:, t]], -1)
            check('rollout_sample.fused_vs_loop.z', err(zf[:, t], z), 1e-5)
            lq = -0.5 * eps[:, t] ** 2 - sd.log() - HALF_LOG_2PI
            check('rollout_sample.fused_vs_loop.log_q', err(lqf[:, t], lq), 1.5e-5)
    # autograd on: Stove.rollout takes its loop of single steps, and a gradient reaches the start state through the samples
    st.noise_fn = feed()
    z0 = z_last.clone().requires_grad_()
    zl, lql, _ = st.rollout(z0, num=num, sample=True)
    assert zl.requires_grad and lql.requires_grad
    check('rollout_sample.fused_vs_loop.z', err(zf, zl), 1e-5)
    zl[:, -1, :, 2:].sum().backward()
    assert z0.grad is not None and float(z0.grad[..., 2:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. the mean path is untouched
@pytest.mark.parametrize('cl,n_obj', [(32, 3), (32, 6), (32, 7), (16, 3), (64, 6)])
def test_mean_rollout_is_untouched_and_is_the_sampling_rollout_at_eps_zero(cl, n_obj):
    from stove_amd import ops
    dyn = _dynamics(cl, n_obj)
    params = _image(dyn, cl)
    B, num = 5, 4
    z_last, eps = _inputs(cl, n_obj, B, num, seed=7)
    z_last, eps = z_last.to(DEV), eps.to(DEV)

    def mean_rollout():
        return ops.rollout(z_last, None, (params, None, None), num, 2, dyn.use_elu, dyn.loop_consts(), want_std=True)[:2]
    z0, s0 = mean_rollout()
    zs, lq, sd, _ = _call_sample(cl, dyn, params, z_last, eps)
    assert not torch.equal(zs, z0)
    z1, s1 = mean_rollout()
    assert torch.equal(z0, z1) and torch.equal(s0, s1)
    zz, lqz, sdz, _ = _call_sample(cl, dyn, params, z_last, torch.zeros_like(eps))
    assert torch.equal(zz, z0) and torch.equal(sdz, s0)
    want = -sdz.double().log() - HALF_LOG_2PI
    assert float(((lqz.double() - want).abs() / want.abs()).max()) < 1e-6
    # the stds are optional
    zn, lqn, none, _ = _call_sample(cl, dyn, params, z_last, eps, zstd=False)
    assert none is None and torch.equal(zn, zs) and torch.equal(lqn, lq)


# ------------------------------------------------------------------------------------------------ 5. the library's own noise
def test_device_noise_is_standard_normal_fresh_per_call_and_follows_the_seed():
    from stove_amd import ops
    from stove_amd.video_prediction.stove import Stove
    st = fill_analytic(Stove(make_cfg())).to(DEV)
    image = st.dyn.kernel_params(0)[0]
    consts, elu = st.dyn.loop_consts(), st.dyn.use_elu
    B, N, num = 64, 3, 8
    z_last = _inputs(32, N, B, num, seed=5)[0].to(DEV)
    torch.manual_seed(1234)
    z, sd, _, lq = ops.rollout(z_last, None, image, num, 2, elu, consts, want_std=True, eps=ops.NoiseSource(DEV), want_logq=True)
    # the draws the kernel used, from its outputs: every step's mean is one mean step from the DRAWN previous state
    prev = torch.cat([z_last[:, None], z[:, :-1]], 1).flatten(0, 1).contiguous()
    mean = ops.rollout(prev, None, image, 1, 2, elu, consts)[0].view(B, num, N, 18)
    e = ((z[..., 2:] - mean[..., 2:]) / sd).double().flatten()
    assert e.numel() == 24576
    m, v = float(e.mean()), float(e.var())
    print(f'rollout_sample.device_noise: mean {m:.4f} var {v:.4f}')
    assert abs(m) < 0.03 and abs(v - 1.0) < 0.05, (m, v)                      # 4.7 and 5.5 standard errors at this count
    assert err(lq, -0.5 * e.view_as(lq) ** 2 - sd.double().log() - HALF_LOG_2PI) < 1.5e-5
    # through Stove.rollout: fresh draws per call, the same draws after the same seed
    assert st.noise_fn is None
    with torch.no_grad():
        torch.manual_seed(99)
        a = st.rollout(z_last, num=num, sample=True)
        b = st.rollout(z_last, num=num, sample=True)
        torch.manual_seed(99)
        a2 = st.rollout(z_last, num=num, sample=True)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])


# ------------------------------------------------------------------------------------------------ 6. the C ABI says no
def test_sampling_rollout_rejects_bad_arguments():
    """Mirrors tests/test_gpu_abi.py: an invalid-value code that stove_error_string() names, nothing enqueued, the stream usable."""
    from stove_amd import _lib
    lib = _lib.load()
    S = _lib.stream()
    B, N, num = 4, 3, 4
    p = _lib.ptr
    k = (0.3, 0.04, 0.04)

    def expect_invalid(code, what):
        assert code == INVALID, (what, code)
        msg = lib.stove_error_string(code)
        assert msg and b'invalid' in msg.lower(), (what, msg)
        torch.cuda.synchronize()
    for cl in (32, 16, 64):
        D = cl // 2
        n_par = lib.stove_gnn_param_floats() if cl == 32 else lib.stove_gnn_param_floats_cl(cl)
        params = torch.zeros(n_par, device=DEV)
        z1 = torch.zeros(B, N, D + 2, device=DEV)
        eps = torch.zeros(B, num, N, D, device=DEV)
        zp = torch.full((B, num, N, D + 2), 7.0, device=DEV)
        lq = torch.full((B, num, N, D), 7.0, device=DEV)

        def call(ptrs, *dims):
            if cl == 32:
                return lib.stove_rollout_sample_fwd(*ptrs, *dims, 2, 0, *k, S)
            return lib.stove_rollout_sample_fwd_cl(*ptrs, cl, *dims, 2, 0, *k, S)
        good = [p(z1), None, p(params), p(eps), p(zp), p(lq), None, None]
        for i, what in ((3, 'NULL eps'), (5, 'NULL log_q'), (0, 'NULL z_last'), (4, 'NULL z_pred')):
            bad = list(good)
            bad[i] = None
            expect_invalid(call(bad, B, num, 1, N, D), f'cl {cl}: {what}')
        expect_invalid(call(good, B, num, 1, N, D + 4), f'cl {cl}: sin_dim > D without extra')
        expect_invalid(call(good, B, -1, 1, N, D), f'cl {cl}: num = -1')
        expect_invalid(call(good, B, num, 1, 9, D), f'cl {cl}: N = 9')
        assert call([None] * 8, 0, num, 1, N, D) == 0                          # B = 0: a valid empty call
        assert float(zp.min()) == 7.0 and float(lq.min()) == 7.0               # nothing was written
        assert call(good, B, num, 1, N, D) == 0                                # and the stream still works
        torch.cuda.synchronize()
        assert bool(torch.isfinite(zp).all()) and bool(torch.isfinite(lq).all())
    if True:
        x = torch.zeros(1 << 12, device=DEV)
        q = ctypes.c_void_p(x.data_ptr())
        expect_invalid(lib.stove_rollout_sample_fwd_cl(q, None, q, q, q, q, None, None, 24, 2, 4, 1, 3, 12, 2, 0, *k, S), 'cl = 24')
